"""The host half of the synthetic pool (vireo_amd/synth_pool.py, vireo_amd/base_utils.py; no GPU):
sample_barcodes / pool_barcodes against files the real reference wrote (tests/golden/synth_pool, byte for byte,
and the next draw of the generator), what they do and do not mutate, their ValueErrors, pool_plan / truth()
against a few lines of plain Python (tests/synthpool_np.py), the three-source rule, get_confusion against the
reference's result and against its double loop, and the argument checks of pool_counts that need no device."""
import copy
import os

import numpy as np
import pytest

from tests import synthpool_np as SN

N_CASE = len(SN.CASES)


@pytest.fixture(scope="module")
def sp():
    from vireo_amd import synth_pool
    return synth_pool


def run_case(sp, i, out_dir):
    """our calls for case i, as the reference's main() makes them -> (barcodes_in, barcodes_out, next draw)"""
    how, n_cell, minor, seed, rate, suffix = SN.CASES[i]
    barcodes_in = SN.split(SN.barcodes_all(), how)
    if n_cell is not None:
        barcodes_in = sp.sample_barcodes(barcodes_in, n_cell, minor, seed)
    barcodes_out = sp.pool_barcodes(barcodes_in, out_dir, rate, sample_suffix=suffix, seed=seed)
    return barcodes_in, barcodes_out, float(np.random.rand())


def test_fixture_is_what_the_issue_lists():
    meta = SN.cases_json()
    assert len(meta) == N_CASE == 8 and len(SN.barcodes_all()) == 952
    for m, (how, n_cell, minor, seed, rate, suffix) in zip(meta, SN.CASES):
        assert (m["split"], m["n_cell"], m["minor_sample"], m["seed"], m["doublet_rate"], m["sample_suffix"]) == \
            (how, n_cell, minor, seed, rate, suffix)
    assert (meta[2]["n_src"], meta[2]["n_pool"], meta[2]["n_doublet"]) == (750, 748, 0)
    assert meta[4]["n_src"] == 22 + 90 + 90                           # round(22.5) = 22


@pytest.mark.parametrize("i", range(N_CASE))
def test_files_and_generator_state_equal_the_reference(sp, i, tmp_path):
    barcodes_in, barcodes_out, nxt = run_case(sp, i, str(tmp_path))
    for name in ("barcodes_pool.tsv", "cell_info.tsv"):
        want = SN.packed()["case%d_%s" % (i, name[:-4])]
        with open(tmp_path / name, "rb") as f:
            assert f.read() == want, name
    assert nxt == SN.cases_json()[i]["next_rand"]
    pool, origin, sid = SN.read_cell_info(tmp_path / "cell_info.tsv")
    assert pool == [x for b in barcodes_out for x in b] and origin == [x for b in barcodes_in for x in b]


def test_out_dir_none_writes_nothing_and_returns_the_same(sp, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    a = run_case(sp, 0, None)
    assert os.listdir(tmp_path) == []
    b = run_case(sp, 0, str(tmp_path))
    assert a[1] == b[1] and a[2] == b[2]


def test_what_is_mutated_and_what_is_not(sp):
    bc = SN.split(SN.barcodes_all(), "3")
    keep = copy.deepcopy(bc)
    inner = bc[1]
    got = sp.sample_barcodes(bc, 50, 0.5, seed=5)
    assert got is bc and [len(b) for b in bc] == [25, 50, 50]         # rewritten in place, as in the reference
    assert inner == keep[1]                                          # the samples' own lists are replaced, not edited
    assert set(bc[2]) <= set(keep[2])
    before = copy.deepcopy(bc)
    for suffix in (True, False):
        out = sp.pool_barcodes(bc, None, 0.3, sample_suffix=suffix, seed=5)
        assert bc == before and out is not bc
    # no seed: the stream goes on where it stands (reseeding happens only with a seed)
    np.random.seed(11)
    a = sp.pool_barcodes(bc, None, 0.3)
    np.random.seed(11)
    b = sp.pool_barcodes(bc, None, 0.3, seed=None)
    assert a == b and a != sp.pool_barcodes(bc, None, 0.3)


def test_names_rates_and_tags(sp):
    bc = [["AAA-1", "CCC-1", "GGG-9"], ["AAA-1", "TTT-x"]] + [["A%02d-1" % i] for i in range(9)]
    out = sp.pool_barcodes(bc, None, 0.0, seed=0)
    assert out[0] == ["AAA-1", "CCC-1", "GGG-1"] and out[1] == ["AAA-2", "TTT-2"]       # the last character, whatever
    assert out[9] == ["A07-10"] and out[10] == ["A08-11"]                                # two digits from sample 10
    n = sum(len(b) for b in bc)
    for rate, want in ((None, round(n / (1 + 1 / (n / 100000.0)))), (1.0, n // 2), (0.5, round(n / 3))):
        flat = [x for b in sp.pool_barcodes(bc, None, rate, seed=1) for x in b]
        assert sum(x[-1] in "SD" for x in flat) == 2 * want
    # S when both members carry the same text after "-", else D
    flat = [x for b in sp.pool_barcodes([["A-1", "B-1"], ["C-1", "D-1"]], None, 1.0, seed=2) for x in b]
    tags = {x[-1] for x in flat}
    assert tags <= {"S", "D"} and len(set(flat)) == 2
    for name in set(flat):
        members = [i for i, x in enumerate(flat) if x == name]
        assert len(members) == 2
        assert name[-1] == ("S" if (members[0] < 2) == (members[1] < 2) else "D")


def test_value_errors(sp):
    bc = SN.split(SN.barcodes_all(), "3")
    with pytest.raises(ValueError, match="fewer"):
        sp.sample_barcodes([list(b) for b in bc], 301, 1.0, seed=0)
    for rate in (-0.01, 1.01):
        with pytest.raises(ValueError, match="between 0 and 1"):
            sp.pool_barcodes(bc, None, rate, seed=0)
    with pytest.raises(ValueError, match="no '-'"):
        sp.pool_barcodes([["AAA1", "CCC1"], ["GGG1", "TTT1"]], None, 1.0, sample_suffix=False, seed=0)
    # without a doublet nothing looks behind the "-": the reference passes too
    assert sp.pool_barcodes([["AAA1"], ["GGG1"]], None, 0.0, seed=0) == [["AAA1"], ["GGG2"]]


@pytest.mark.parametrize("i", range(N_CASE))
def test_pool_plan_and_truth_against_plain_python(sp, i):
    pool, origin, sid = SN.cell_info(i)
    names, sources, truth = SN.plan_of(pool, sid)
    barcodes_in, barcodes_out, _ = run_case(sp, i, None)
    plan = sp.pool_plan(barcodes_in, barcodes_out)
    meta = SN.cases_json()[i]
    assert plan.n_pool == meta["n_pool"] and plan.n_src == meta["n_src"]
    assert plan.barcodes.tolist() == names
    assert plan.src0.dtype == np.int32 and plan.src1.dtype == np.int32
    assert [[a] if b < 0 else [a, b] for a, b in zip(plan.src0.tolist(), plan.src1.tolist())] == sources
    assert plan.truth().tolist() == truth and truth.count("doublet") == meta["n_doublet"]
    assert plan.sample.astype(str).tolist() == sid
    P, want = plan.matrix(), SN.pool_matrix(sources, len(pool))
    assert P.shape == want.shape and P.dtype == np.int64 and (P != want).nnz == 0
    sub = plan.subset([3, 0, plan.n_pool - 1])
    assert sub.barcodes.tolist() == [names[3], names[0], names[-1]] and sub.sizes == plan.sizes
    if i == 2:                                                       # shared names without a doublet
        two = [s for s in sources if len(s) == 2]
        assert len(two) == 2 and all(sid[a] == sid[b] for a, b in two)
        assert all(not n.endswith(("S", "D")) for n in names)


def test_s_doublets_keep_their_sample_and_three_sources_are_rejected(sp):
    plan = sp.pool_plan([["a-1", "b-1"], ["c-1"]], [["x-1S", "x-1S"], ["c-2"]])
    assert plan.truth().tolist() == ["2", "1"] and plan.src1.tolist() == [-1, 1]
    plan = sp.pool_plan([["a-1", "b-1"], ["c-1"]], [["a-1D", "b-1"], ["a-1D"]])
    assert plan.truth().tolist() == ["doublet", "1"]
    with pytest.raises(ValueError, match="'x-1D' has 3 source cells"):
        sp.pool_plan([["a-1", "b-1"], ["c-1", "d-1"]], [["x-1D", "b-1"], ["x-1D", "x-1D"]])
    with pytest.raises(ValueError, match="differ"):
        sp.pool_plan([["a-1", "b-1"]], [["a-1"]])
    empty = sp.pool_plan([[], []], [[], []])
    assert empty.n_pool == 0 and empty.truth().size == 0 and empty.matrix().shape == (0, 0)
    with pytest.raises(ValueError, match="outside"):
        sp.PoolPlan(["p"], [2], [-1], [1, 1])


def test_get_confusion_equals_the_reference_and_the_double_loop():
    import vireo_amd
    from vireo_amd.base_utils import get_confusion
    assert vireo_amd.get_confusion is get_confusion and "get_confusion" in vireo_amd.__all__
    z = SN.confusion()
    for a, b in ((z["ids1"].tolist(), z["ids2"].tolist()), (z["ids1"], z["ids2"])):
        mat, u1, u2 = get_confusion(a, b)
        assert np.array_equal(mat, z["mat"]) and u1.tolist() == z["uniq1"].tolist()
        assert u2.tolist() == z["uniq2"].tolist() and u1.dtype == z["uniq1"].dtype
        assert mat.dtype == np.zeros(1, dtype=int).dtype and mat.shape == (12, 6)
    rng = np.random.default_rng(3)
    for n, k1, k2 in ((0, 1, 1), (1, 1, 1), (500, 7, 3), (2000, 1, 40)):
        a = np.array(["id%d" % x for x in rng.integers(0, k1, n)], dtype=str)
        b = rng.integers(-5, k2 - 5, n)                              # strings against integers
        got, want = get_confusion(a, b), SN.confusion_loops(a, b)
        assert got[0].shape == want[0].shape and np.array_equal(got[0], want[0])
        assert got[1].tolist() == want[1].tolist() and got[2].tolist() == want[2].tolist()
        assert got[1].dtype == want[1].dtype and got[2].dtype == want[2].dtype
    with pytest.raises(ValueError, match="3 entries"):
        get_confusion(["a", "b", "c"], ["a", "b"])


def test_pool_counts_argument_checks_and_no_cpu_path(sp):
    import __graft_entry__ as entry
    entry.build()
    import vireo_amd
    from vireo_amd import _lib
    assert vireo_amd.pool_counts is sp.pool_counts and vireo_amd.PoolPlan is sp.PoolPlan
    X = np.arange(12).reshape(3, 4)
    plan = sp.PoolPlan(["p", "q"], [0, 2], [1, -1], [4])
    with pytest.raises(ValueError, match="variants"):
        sp.pool_counts([(X, X), (X[:2], X[:2])], sp.PoolPlan(["p"], [0], [-1], [4, 4]))
    with pytest.raises(ValueError, match="columns"):
        sp.pool_counts([(X[:, :3], X[:, :3])], plan)
    with pytest.raises(ValueError, match="no sample"):
        sp.pool_counts([], sp.PoolPlan([], [], [], []))
    with pytest.raises(ValueError, match="barcode lists"):
        sp.synth_pool([(X, X)], [["a-1"] * 4, ["b-1"]])
    with pytest.raises(ValueError, match="4 columns and 3 barcodes"):
        sp.synth_pool([(X, X)], [["a-1", "b-1", "c-1"]])
    for name in ("vrx_pool_create", "vrx_pool_run", "vrx_pool_read", "vrx_pool_destroy", "vrx_pool_wave_limit",
                 "vrx_pool_scan_block"):
        assert name in _lib.SIGNATURES and getattr(_lib.lib(), name) is not None
    W, B = _lib.lib().vrx_pool_wave_limit(), _lib.lib().vrx_pool_scan_block()
    assert W >= 64 and W % 64 == 0 and B >= 64
    if _lib.device_count() == 0:
        with pytest.raises(_lib.VrxError):                           # there is no host path to fall back to
            sp.pool_counts([(X, X)], plan)
    with pytest.raises(SystemExit) as e:
        sp.main(["-o", "somewhere"])
    assert e.value.code == 1
