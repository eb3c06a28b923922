"""The builder sweep of tests/build_cases.py without a device: the cases are what they claim to be, the
integer operands make exactness a theorem, and they see every planted defect.

tests/test_gpu_build_exact.py holds both problem builders to the int64 products of the input under
``np.array_equal``.  That proves something only if (a) every case is a valid canonical pattern that
takes the path it declares -- its forms, formats and row pieces follow from the build rules restated
in build_cases.py --, (b) no partial sum of any pass can leave the integers float64 holds exactly,
and (c) a builder that loses, repeats or misplaces one entry changes at least one product.  Here a
NumPy stand-in for the device forms the same products from a damaged copy of the input.
"""
import numpy as np
import pytest

from tests import build_cases as B


@pytest.mark.parametrize("name", B.CASES)
def test_case_is_a_canonical_pair_on_its_declared_path(name):
    sp = B.CASES[name]
    m = B.merged(sp.data)
    (N, M), colptr, rowidx, ad, dp = m
    assert N > 0 and M > 0 and colptr.dtype == np.int64 and colptr.shape == (M + 1,)
    assert colptr[0] == 0 and colptr[-1] == rowidx.size == ad.size == dp.size and np.all(np.diff(colptr) >= 0)
    assert rowidx.dtype == ad.dtype == dp.dtype == np.int32
    assert np.all(rowidx >= 0) and np.all(rowidx < N) and np.all(ad >= 0) and np.all(dp >= 0)
    inside = np.ones(rowidx.size, bool)
    inside[colptr[:-1][colptr[:-1] < rowidx.size]] = False       # (the first entry of a column)
    assert np.all(np.diff(rowidx.astype(np.int64), prepend=-1)[inside] > 0), "rows strictly increasing in a column"
    AD, DP = B.matrices(m)
    assert AD.has_canonical_format and DP.has_canonical_format
    # the declared path follows from the restated rules
    assert B.expected_forms(m, sp.env) == (sp.cell_form, sp.var_form)
    assert B.expected_format(m, sp.env) == sp.entry_format
    for want, got in zip(sp.pieces, B.expected_pieces(m, sp.env, sp.var_form)):
        assert want is None or want == (got > 0), (sp.pieces, got)
    pairs = sp.cell_form == 0 or sp.var_form == 0
    declines = rowidx.size == 0 or (pairs and B.max_count(m) >= 2048)
    assert sp.device_built == (not declines) and (sp.declines is None) == sp.device_built
    assert sp.host_lds == (not (pairs and B.max_count(m) >= 2048) or sp.cell_form == 1)
    if sp.balance:      # balanced slabs are AD/BD streams
        assert (sp.cell_form, sp.var_form) == (1, 3)


def test_every_feature_tag_is_carried():
    carried = {t for sp in B.CASES.values() for t in sp.tags}
    assert carried == set(B.TAGS)
    on_device = {t for sp in B.CASES.values() if sp.device_built for t in sp.tags}
    assert set(B.TAGS) - on_device == set(B.FALL_BACKS)
    assert {sp.declines for sp in B.CASES.values() if not sp.device_built} != {None}


def test_cases_hold_what_their_tags_say():
    def md(name):
        (N, M), colptr, rowidx, ad, dp = B.merged(B.CASES[name].data)
        return N, M, colptr, rowidx, ad.astype(np.int64), dp.astype(np.int64)

    N, M, colptr, rowidx, ad, dp = md("zeros")
    assert ((ad == 0) & (dp == 0)).sum() > 20 and ((dp == 0) & (ad > 0)).sum() > 20
    assert ((ad == 0) & (dp > 0)).sum() > 20 and (ad > dp).sum() > 20
    assert (md("neg_bd")[4] > md("neg_bd")[5]).sum() > 100
    assert md("single")[3].size == 1 and md("one_variant")[0] == 1 and md("one_cell")[1] == 1
    N, M, colptr, rowidx, ad, dp = md("odd_cells")
    assert M % 2 == 1 and colptr[-1] - colptr[-2] > 10              # entries in the last, unpaired cell
    for L in (4095, 4096, 4097):
        N, M, colptr, rowidx, ad, dp = md("row%d_var" % L)
        assert np.bincount(rowidx, minlength=N).max() == L
        assert np.diff(md("row%d_cell" % L)[2]).max() == L
    for top in (63, 64, 2047, 2048, 32767, 32768, 65535, 65536):
        name = "top%d" % top if "top%d" % top in B.CASES else "top%d_fmt0" % top
        N, M, colptr, rowidx, ad, dp = md(name)
        assert max(ad.max(), dp.max()) == top and (ad == top).sum() >= 1 and (dp == top).sum() >= 2
    N, M, colptr, rowidx, ad, dp = md("empty_edges")
    lens, rows = np.diff(colptr), np.bincount(rowidx, minlength=N)
    assert not lens[:30].any() and not lens[-33:].any() and not rows[:40].any() and not rows[-35:].any()
    assert lens[30] and lens[-34] and rows.any()
    # the heavy-tailed input, scaled down: the smallest rung of the ladder that cuts pieces in both orientations,
    # on both forms
    cuts = [all(min(B.expected_pieces(B.merge(*B.heavy_tail(*shape)), {}, vf)) > 0 for vf in (0, 3))
            for shape in B.HEAVY_LADDER]
    assert cuts == [False] * (len(cuts) - 1) + [True] and B.HEAVY_SMALL == B.HEAVY_LADDER[-1]
    assert md("empty")[3].size == 0
    N, M = B.BAL_SHAPE
    assert N > EC_SLAB and (M + 1) // 2 > EC_SLAB


EC_SLAB = B.EC.SLAB_CELL      # the nominal slab of the cell pass and of the variant pass over virtual rows


@pytest.mark.parametrize("name", B.CASES)
def test_partial_sums_stay_below_2_53(name):
    """sum of |weight| x |count| over any output cell, in every grouping a pass may use, for every seed"""
    m = B.merged(B.CASES[name].data)
    for seed in B.SEEDS:
        top_v, top_c = B.magnitudes(m, B.operands(name, seed))
        assert top_v < 2 ** 53 and top_c < 2 ** 53, (seed, top_v, top_c)


def test_operands_are_integers_in_range():
    op = B.operands("mid", B.GPU_SEED)
    assert set(op.ID) == set(B.N_COLS)
    for K, ID in op.ID.items():
        assert ID.dtype == np.float64 and np.array_equal(ID, np.rint(ID)) and np.abs(ID).max() <= B.ID_TOP
        assert ID.min() < 0 < ID.max() and not (ID == 0).any()
    for tag, K, unit in B.CELL_OPS:
        GT, psi = op.cell[tag]
        assert GT.shape[1:] == (K, 1) and np.array_equal(GT, np.rint(GT)) and GT.min() >= 1
        assert all(np.array_equal(p, np.rint(p)) for p in psi)
        if unit is None:      # the three tables differ everywhere: no factor of AD, BD or DP vanishes
            assert psi[0].shape[0] == GT.shape[0] and min(p.min() for p in psi) < 0
            assert not (psi[0] == psi[1]).any() and not (psi[1] == psi[2]).any() and not (psi[0] == psi[2]).any()
    assert not np.array_equal(op.ID[5], B.operands("mid", 1).ID[5])
    assert not np.array_equal(op.ID[5], B.operands("many", B.GPU_SEED).ID[5][:op.ID[5].shape[0]])


@pytest.mark.parametrize("name", B.CASES)
def test_planted_defects_change_a_product(name):
    """every defect that applies to the case, for every operand seed"""
    m = B.merged(B.CASES[name].data)
    for seed in B.SEEDS:
        op = B.operands(name, seed)
        clean = B.products(m, op)
        assert not B.differs(clean, B.products(B._copy(m), op))
        for what, damage in B.DEFECTS.items():
            bad = damage(m, np.random.default_rng([seed, len(what)]))
            if bad is not None:
                assert B.differs(clean, B.products(bad, op)), (what, seed)


def test_every_defect_applies_somewhere():
    rng = np.random.default_rng(0)
    hit = {what: sum(damage(B.merged(sp.data), rng) is not None for sp in B.CASES.values())
           for what, damage in B.DEFECTS.items()}
    n = len(B.CASES)
    assert hit["wrapped_2048"] >= 3 and hit["dropped"] == hit["doubled"] == hit["last_lost"] == n - 1
    # (a swap needs two entries in one column: not the empty case, a single entry, a single variant)
    flat = sum(np.diff(B.merged(sp.data)[1]).max() < 2 for sp in B.CASES.values())
    assert hit["rows_swapped"] == n - flat and flat <= 8 and hit["ad_dp_exchanged"] == n - 1, hit


def test_the_stand_in_sees_each_unit_setting_alone():
    """(1,0,0), (0,1,0), (0,0,-1): AD.T @ GT, (DP - AD).T @ GT, DP.T @ GT"""
    m = B.merged("neg_bd")
    op = B.operands("neg_bd", B.GPU_SEED)
    AD, DP = B.matrices(m)
    want = B.products(m, op)
    for tag, X in (("AD", AD), ("BD", DP - AD), ("DP", DP)):
        g = op.cell[tag][0][:, :, 0].astype(np.int64)
        assert np.array_equal(want["cell", tag], X.T @ g)
    assert (want["cell", "BD"] < 0).any()        # negative BD reaches the products
    assert B.count_cells(want) == 2 * AD.shape[0] * sum(B.N_COLS) + AD.shape[1] * sum(k for _, k, _ in B.CELL_OPS)
    assert B.mismatches(want["cell", "AD"].astype(np.float64), want["cell", "AD"]) == 0
    off = want["cell", "AD"].astype(np.float64)
    off[3, 2] += 1.0
    assert B.mismatches(off, want["cell", "AD"]) == 1
