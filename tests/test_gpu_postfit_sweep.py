"""Sweep of the steps that run on a FITTED model (MI355X): predict_doublet, the ambient-RNA EM
(vrx_problem_ambient), variant_ELBO_gain and the donor-read products, at the shapes the fixtures
do not have.  Python -> ctypes -> C ABI, like the rest of the suite.

* Doublets: one step from an identical state.  The oracle (pinned bit for bit to the reference's
  predict_doublet at n_GT 2 .. 5 and in ASE mode, tests/test_oracle_golden.py) fits a few
  iterations, a seeded random table is mixed into its GT_prob (30 %: the drawn counts have no donor
  structure, and a fit on the deep ones ends with every donor alike and all columns tied), that state
  is copied into a vireo_amd.Vireo, both predict doublets.  n_GT 2 .. 5,
  K 2 .. 20, ASE mode, both VIREO_LDS settings, the update flags, doublet_rate_prior, per-cell
  ID_prior.  1e-5 relative, identical argmax, no case excused.
* Ambient EM: vrx_problem_ambient directly, so that the test chooses the selection, the start,
  the stop rule; cells with an exact number of selected entries around the 64-entry chunks of
  vrx_amb_pass and around the LDS capacity `cap`; K from 1 to 130 (K > 64: the second trip of the
  lane loops); the three entry formats (asserted on the built problem).  Against tests/ambient_np.py, and bitwise equal between the
  LDS-cached and the global theta route (they read the same values in the same order).
* ELBO gain / donor reads: deep variants (millions of reads: s psi(s) cancels), 1 .. 40 columns,
  pseudocounts 1e-3 .. 10, exact zeros and ones in ID_prob; the gain is judged against a 40-digit
  mpmath evaluation, the device may be at most 4 x as far from it as float64 NumPy / SciPy is.

Shapes come from `draw_case` of tests/test_gpu_fuzz.py (empty rows, one long row and column, counts
up to 5000); the ambient problems with exact entry counts are built entry by entry.
"""
import copy
import math

import numpy as np
import pytest
from scipy.sparse import csc_matrix

from oracle import vireo_oracle as O
from tests import ambient_np as A
from tests.exact_ambient import amb_cap, amb_lds_bytes, built_ambient_problem, run_ambient
from tests.exact_ambient import id_prob as _id_prob
from tests.test_gpu_fuzz import draw_case

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-5, 1e-300


@pytest.fixture(scope="module")
def va():
    import vireo_amd
    from vireo_amd import _lib
    _lib.require_gpu()
    return vireo_amd


def close(a, b, rtol=RTOL, atol=ATOL):
    np.testing.assert_allclose(np.asarray(a), np.asarray(b), rtol=rtol, atol=atol)


# =============================================================================== doublets
# (seed of draw_case, n_GT, K, ASE mode, VIREO_LDS, doublet_rate_prior, what else)
# every (n_GT, K) of {2, 3, 4, 5} x {2, 3, 7, 16, 20}; ASE mode, VIREO_LDS and the rate alternate so that
# each n_GT meets both ASE settings on both routes (n_GT = 2 in ASE mode on the LDS-resident pass: seed 214)
DOUBLET_CASES = [
    (206, 2, 2, False, "1", None, ""), (223, 3, 2, True, "0", 0.1, ""),
    (215, 4, 2, False, "0", 0.5, ""), (249, 5, 2, True, "1", None, ""),
    (214, 2, 3, True, "1", 0.1, ""), (220, 3, 3, False, "1", 0.5, ""),
    (219, 4, 3, True, "0", None, ""), (234, 5, 3, False, "0", 0.1, ""),
    (227, 2, 7, False, "0", 0.5, ""), (250, 3, 7, True, "1", None, ""),
    (239, 4, 7, False, "1", 0.1, ""), (241, 5, 7, True, "0", 0.5, ""),
    (225, 2, 16, True, "0", None, ""), (253, 3, 16, False, "0", 0.1, ""),
    (272, 4, 16, True, "1", 0.5, ""), (282, 5, 16, False, "1", None, ""),
    (211, 2, 20, False, "1", 0.1, ""), (208, 3, 20, True, "1", 0.5, ""),
    (245, 4, 20, False, "0", None, ""), (283, 5, 20, True, "0", 0.1, ""),
    (216, 3, 4, False, "1", None, "no_update_ID"), (229, 4, 5, False, "0", 0.1, "no_update_GT"),
    (233, 3, 6, False, "0", None, "cell_prior"), (243, 5, 3, True, "1", 0.5, "cell_prior"),
]


def _oracle_doublet(st, AD, DP, update_GT, update_ID, rate):
    """O.vireo_doublet (update_GT = update_ID = True) and the reference's flags on its side effects
    (vireo_doublet.py:70-77): -> (doublet_prob, singlet block, LLR, ID_prob after, GT_prob after, printed)"""
    work = copy.deepcopy(st)
    dbl, sing, llr = O.vireo_doublet(work, AD, DP, doublet_rate_prior=rate)
    ID_after = work.ID_prob if update_ID else st.ID_prob
    GT_after = work.GT_prob if (update_GT and update_ID) else st.GT_prob
    printed = "For update_GT, please turn on update_ID.\n" if (update_GT and not update_ID) else ""
    return dbl, sing, llr, ID_after, GT_after, printed


def fitted_state(seed, T, K, ase, extra):
    """draw_case(seed) and the oracle's state after a few iterations on it.  The drawn counts carry no donor
    structure, so on the deep ones a fit ends where every donor has the same genotypes and all columns of the
    doublet step tie; a seeded random table is therefore mixed into GT_prob (30 %) before the step.
    -> AD, DP, state, per-cell ID_prior or None, VIREO_LDS_BLOCKS"""
    AD, DP, _, rng = draw_case(seed)
    N, M = AD.shape
    blocks = int(rng.choice([1, 16, 1024]))
    np.random.seed(seed)
    ref = O.vireo_new(M, N, K, n_GT=T, ASE_mode=ase)
    prior = None
    if extra == "cell_prior":
        prior = rng.dirichlet(np.ones(K) * 0.5, M) * 0.98 + 0.02 / K      # (no zeros: log prior finite)
        O.vireo_prior(ref, ID_prior=prior.copy())
    O.vireo_fit(ref, AD, DP, min_iter=2, max_iter=4, delay_fit_theta=1)
    assert ref.GT_prob.shape == (N, K, T) and ref.beta_mu.shape == (N if ase else 1, T)
    ref.GT_prob = O.unit_sum(0.7 * ref.GT_prob + 0.3 * rng.dirichlet(np.ones(T), (N, K)))
    return AD, DP, ref, prior, blocks


@pytest.mark.parametrize("seed,T,K,ase,lds,rate,extra", DOUBLET_CASES)
def test_doublet_step_vs_oracle(va, monkeypatch, capsys, seed, T, K, ase, lds, rate, extra):
    from vireo_amd.counts import DeviceCounts
    AD, DP, ref, prior, blocks = fitted_state(seed, T, K, ase, extra)
    N, M = AD.shape
    monkeypatch.setenv("VIREO_LDS", lds)
    monkeypatch.setenv("VIREO_LDS_BLOCKS", str(blocks))

    dev = va.Vireo(n_cell=M, n_var=N, n_donor=K, n_GT=T, ASE_mode=ase, ID_prob_init=ref.ID_prob.copy(),
                   GT_prob_init=ref.GT_prob.copy())
    dev.ID_prob, dev.GT_prob = ref.ID_prob.copy(), ref.GT_prob.copy()      # (the constructor renormalises)
    dev.beta_mu, dev.beta_sum = ref.beta_mu.copy(), ref.beta_sum.copy()
    if prior is not None:
        dev.set_prior(ID_prior=prior.copy())
    update_ID, update_GT = extra != "no_update_ID", extra != "no_update_GT"
    dbl0, sing0, llr0, ID0, GT0, printed0 = _oracle_doublet(ref, AD, DP, update_GT, update_ID, rate)

    counts = DeviceCounts(AD, DP)
    capsys.readouterr()
    dbl, sing, llr = va.predict_doublet(dev, counts, None, update_GT=update_GT, update_ID=update_ID,
                                        doublet_rate_prior=rate)
    assert capsys.readouterr().out == printed0
    counts.close()
    n_pair = K * (K - 1) // 2
    assert dbl.shape == (M, n_pair) and sing.shape == (M, K) and llr.shape == (M,)
    both, both0 = np.append(sing, dbl, axis=1), np.append(sing0, dbl0, axis=1)
    worst = np.max(np.abs(both - both0) / np.maximum(both0, 1e-290))
    print("seed %d n_GT %d K %d (%d x %d, %d entries): worst relative distance of the %d class posteriors %.2e, "
          "LLR %.2e absolute; %d of %d cells undecided (largest posterior < 0.999), %d called doublets"
          % (seed, T, K, N, M, DP.nnz, K + n_pair, worst, np.max(np.abs(llr - llr0)), (both0.max(1) < 0.999).sum(), M,
             (both0.argmax(1) >= K).sum()))
    close(dbl, dbl0)
    close(sing, sing0)
    close(llr, llr0, rtol=1e-5, atol=1e-8)
    assert np.array_equal(both.argmax(1), both0.argmax(1))
    assert np.array_equal(dbl.argmax(1), dbl0.argmax(1)) and np.array_equal(sing.argmax(1), sing0.argmax(1))
    # the side effects on the object
    close(dev.ID_prob, ID0)
    close(dev.GT_prob, GT0)
    if not update_ID:
        assert np.array_equal(dev.ID_prob, ref.ID_prob) and np.array_equal(dev.GT_prob, ref.GT_prob)
    elif not update_GT:
        assert np.array_equal(dev.ID_prob, sing) and np.array_equal(dev.GT_prob, ref.GT_prob)
    else:
        assert np.array_equal(dev.ID_prob, sing)
    close(dev.beta_mu, ref.beta_mu, rtol=0, atol=0)
    close(dev.beta_sum, ref.beta_sum, rtol=0, atol=0)


def test_doublet_needs_two_donors(va):
    """K = 1 has no pair: the reference fails on its empty pair list; predict_doublet says so before any
    arithmetic (no warning of a division by the zero pairs), and so does the library when called directly"""
    import warnings
    from vireo_amd import _lib
    from vireo_amd._lib import dptr
    from vireo_amd.counts import DeviceCounts
    AD, DP, _, _ = draw_case(257)
    N, M = AD.shape
    np.random.seed(0)
    dev = va.Vireo(n_cell=M, n_var=N, n_donor=1)
    counts = DeviceCounts(AD, DP)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with pytest.raises(ValueError, match="n_donor >= 2"):
            va.predict_doublet(dev, counts, None)
    GT, psi, prior, out = dev.GT_prob.copy(), np.zeros((1, 6)), np.ones((1, 1)), np.empty((M, 1))
    rc = _lib.lib().vrx_problem_doublet(counts.handle, 1, 3, dptr(GT), dptr(psi), dptr(psi), dptr(psi), 1,
                                        dptr(prior), 1, dptr(out), None)
    assert rc != 0 and b"n_donor >= 2" in _lib.lib().vrx_last_error()
    counts.close()


def test_wrap_with_a_four_class_genotype_prior(va):
    """vireo_wrap(GT_prior=<n_var x n_donor x 4>) with the default check_doublet=True: the restarts, the
    final fit and the doublet step at n_GT = 4 against the oracle's driver"""
    AD, DP = O.synth_donor(300, 200, 3, 0.05, seed=0)
    prior = np.random.default_rng(5).dirichlet(np.ones(4) * 2.0, (300, 3))
    want = O.vireo_wrap_oracle(AD, DP, GT_prior=prior.copy(), n_init=2, random_seed=2, n_GT=4)
    got = va.vireo_wrap(AD, DP, GT_prior=prior.copy(), n_init=2, random_seed=2, n_GT=4, nproc=1)
    assert got["doublet_prob"].shape == (200, 3) and got["GT_prob"].shape == (300, 3, 4)
    close(got["LB_list"], want["LB_list"])
    close(got["LB_doublet"], want["LB_doublet"])
    close(got["ID_prob"], want["ID_prob"])
    close(got["doublet_prob"], want["doublet_prob"])
    close(got["doublet_LLR"], want["doublet_LLR"], rtol=1e-5, atol=1e-8)
    close(got["GT_prob"], want["GT_prob"])
    assert np.array_equal(got["ID_prob"].argmax(1), want["ID_prob"].argmax(1))


# =============================================================================== ambient EM
# (amb_lds_bytes, amb_cap, run_ambient, built_ambient_problem: tests/exact_ambient.py)
# K, entries per constructed cell, small cap (cells with cap - 1, cap, cap + 1 entries are added; None: no
# such budget), (min_iter, max_iter, eps), VIREO_ENTRY_FMT, largest count, all-zero selection.
# Cells never have more entries than an LDS budget below 64 KiB can cache (59 at K = 130, 121 at K = 64 / 65).
CHUNKS = [0, 1, 63, 64, 65, 128]
DEFAULT_RULE, TWO_PASSES, NO_EPS, HUGE_EPS = (20, 200, 1e-3), (0, 2, 1e-3), (0, 50, 0.0), (5, 30, 1e9)
AMBIENT_CASES = [
    (1, CHUNKS, None, DEFAULT_RULE, 0, 40, False),
    (2, CHUNKS, None, TWO_PASSES, 1, 40, False),
    (3, CHUNKS, 10, NO_EPS, 2, 300, False),
    (8, CHUNKS, None, HUGE_EPS, 0, 40, False),
    (16, CHUNKS, 20, DEFAULT_RULE, 1, 5000, False),
    (33, CHUNKS, None, DEFAULT_RULE, 1, 300, False),
    (64, [0, 1, 63, 64, 65], 5, NO_EPS, 0, 40, False),
    (65, [0, 1, 63, 64, 65], None, DEFAULT_RULE, 2, 5000, False),
    (130, [0, 1, 31, 59], 10, DEFAULT_RULE, 0, 40, False),
    (130, [0, 1, 2], 3, TWO_PASSES, 1, 300, False),
    (3, CHUNKS, None, DEFAULT_RULE, 0, 40, True),
    (65, [0, 1, 64, 65], None, TWO_PASSES, 2, 40, True),
    (2, [0, 1, 128], 64, DEFAULT_RULE, 0, 40, False),        # cap edges = chunk edges: 63, 64, 65
    (33, [0, 1, 65], 128, NO_EPS, 2, 300, False),            # 127, 128, 129
    (8, [0, 64, 128], 1, HUGE_EPS, 1, 5000, False),          # cap 1: 0, 1, 2 entries
    (16, [0, 1, 63, 65], 64, TWO_PASSES, 0, 40, False),
    (130, CHUNKS, 10, DEFAULT_RULE, 0, 40, False),           # (see UNCACHEABLE)
]
# K > 64 (the second trip of the lane loops) together with the 64-entry chunk loop: cells of up to 160 entries
# at K = 130, more than any budget can cache, so this case compares the default, the global and the small-cap
# budget only
UNCACHEABLE = {16}


def ambient_reference(theta, sel, AD, DP, psi0, cells, rule):
    """the restatement in float64 and in long double; the two must agree on every cell's exit iteration
    (a stop decided by rounding could legitimately differ on the device: the seeds here have none)"""
    kw = dict(min_iter=rule[0], max_iter=rule[1], eps=rule[2])
    want = A.predict(theta, sel, AD, DP, psi0, cells=cells, **kw)
    wide = A.predict(theta, sel, AD, DP, psi0, cells=cells, dtype=np.longdouble, **kw)
    assert np.array_equal(want[3], wide[3]), np.flatnonzero(want[3] != wide[3])
    return want


def check_ambient(counts, K, theta, sel, AD, DP, psi0, cells, rule, budgets, monkeypatch, label):
    want_psi, want_var, want_llr, want_it = ambient_reference(theta, sel, AD, DP, psi0, cells, rule)
    runs = {}
    for name, budget in budgets:
        if budget is None:
            monkeypatch.delenv("VIREO_AMBIENT_LDS", raising=False)
        else:
            assert amb_lds_bytes(K, amb_cap(K, budget)) <= 64 * 1024
            monkeypatch.setenv("VIREO_AMBIENT_LDS", str(budget))
        runs[name] = run_ambient(counts, K, theta, sel, psi0, *rule)
    psi, var, llr, n_iter = runs["default"]
    ok = ~np.isnan(want_llr)
    print("%s: %d cells compared (%d without selected counts), iterations %s .. %s; psi %.2e var %.2e (rel) llr %.2e"
          % (label, len(cells), (~ok).sum(), want_it.min(), want_it.max(),
             np.max(np.abs(psi[cells] - want_psi)[ok], initial=0.0),
             np.max((np.abs(var[cells] - want_var) / want_var)[ok], initial=0.0),
             np.max(np.abs(llr[cells] - want_llr)[ok], initial=0.0)))
    # against the restatement (the tolerances of tests/test_gpu_ambient.py::_close)
    assert np.array_equal(np.isnan(psi[cells]), np.isnan(want_psi))
    assert np.array_equal(np.isnan(var[cells]), np.isnan(want_var))
    assert np.array_equal(np.isnan(llr[cells]), np.isnan(want_llr))
    np.testing.assert_allclose(psi[cells], want_psi, rtol=0, atol=1e-12)
    np.testing.assert_allclose(var[cells], want_var, rtol=1e-10)
    np.testing.assert_allclose(llr[cells], want_llr, rtol=0, atol=1e-9)
    assert np.array_equal(n_iter[cells], want_it)
    # the LDS-cached and the global theta route: the same values in the same order, every cell
    for name, res in runs.items():
        for x, y, what in zip(res, runs["default"], ("psi", "var", "llr", "n_iter")):
            assert np.array_equal(x, y, equal_nan=True), (name, what)


@pytest.mark.parametrize("case", range(len(AMBIENT_CASES)))
def test_ambient_em_exact_entry_counts(va, monkeypatch, case):
    from vireo_amd.counts import DeviceCounts
    K, targets, cap, rule, fmt, top, empty = AMBIENT_CASES[case]
    targets = list(targets) + ([cap - 1, cap, cap + 1] if cap is not None else [])
    n_max = 160 if case in UNCACHEABLE else 59 if K > 65 else 121 if K > 33 else 160
    assert max(targets) <= n_max
    shape, colptr, rowidx, ad, dp, sel, theta, psi0 = built_ambient_problem(
        case, K, targets, n_background=40, bg_max=n_max, top=top, empty_selection=empty)
    N, M = shape
    AD = csc_matrix((ad, rowidx, colptr), shape=shape)
    DP = csc_matrix((dp, rowidx, colptr), shape=shape)
    n_sel = np.array([(sel[rowidx[colptr[c]:colptr[c + 1]]]).sum() for c in range(M)])
    if not empty:
        assert list(n_sel[:len(targets)]) == targets          # the constructed cells are what they claim
    monkeypatch.setenv("VIREO_ENTRY_FMT", str(fmt))
    counts = DeviceCounts.from_merged(shape, colptr, rowidx, ad, dp)
    # the format the case asks for is the one that was built (4 B entries need counts below 64)
    assert counts.entry_format() == (fmt, fmt) and (fmt > 0 or top < 64)
    budgets = [("default", None), ("global", 0)]
    every = amb_lds_bytes(K, int(n_sel.max()))
    if case in UNCACHEABLE:
        assert every > 64 * 1024 and n_sel.max() > amb_cap(K, 16384)
    else:
        assert amb_cap(K, every) == n_sel.max() and every <= 64 * 1024
        budgets.append(("all_cached", every))
    if cap is not None:
        small = amb_lds_bytes(K, cap)
        assert amb_cap(K, small) == cap and amb_cap(K, small - 1) == cap - 1
        budgets.append(("cap_%d" % cap, small))
    label = "K %d rule %s fmt %d top %d%s" % (K, rule, fmt, top, " (nothing selected)" if empty else "")
    check_ambient(counts, K, theta, sel, AD, DP, psi0, np.arange(M), rule, budgets, monkeypatch, label)
    counts.close()


@pytest.mark.parametrize("seed,K,rule,lds", [(253, 8, DEFAULT_RULE, "1"), (211, 16, HUGE_EPS, "0")])
def test_ambient_em_on_drawn_shapes(va, monkeypatch, seed, K, rule, lds):
    """counts up to 5000, a cell with every variant, empty cells (draw_case): 64 sampled cells and the
    longest ones against the restatement, every cell between the routes"""
    from vireo_amd.counts import DeviceCounts
    AD, DP, _, rng = draw_case(seed)
    N, M = AD.shape
    monkeypatch.setenv("VIREO_LDS", lds)
    sel = np.zeros(N, bool)
    sel[rng.choice(N, 300, replace=False)] = True
    GT = rng.dirichlet(np.ones(3) * 0.3, (N, K))
    theta = np.tensordot(GT, np.array([0.01, 0.5, 0.99]), axes=(2, 0))
    psi0 = rng.dirichlet(np.ones(K), M)
    n_sel = np.asarray((DP[sel] > 0).sum(0)).ravel()
    cells = np.unique(np.concatenate([rng.choice(M, 64, replace=False), np.argsort(n_sel)[-4:],
                                      np.flatnonzero(n_sel == 0)[:4]]))
    every = amb_lds_bytes(K, int(n_sel.max()))
    budgets = [("default", None), ("global", 0), ("all_cached", every)]
    counts = DeviceCounts(AD, DP)
    check_ambient(counts, K, theta, sel, AD, DP, psi0, cells, rule, budgets, monkeypatch,
                  "seed %d K %d (%d x %d), up to %d selected entries per cell" % (seed, K, N, M, n_sel.max()))
    counts.close()


# =============================================================================== ELBO gain, donor reads
# (seed of draw_case, columns, pseudocount, VIREO_LDS, ID_prob kind); seeds 214 .. 270: counts up to 5000,
# variants of 3e6 .. 5e6 reads
GAIN_CASES = [
    (214, 1, 0.5, "1", "random"), (250, 40, 1e-3, "0", "onehot"), (253, 7, 10.0, "1", "onehot"),
    (270, 16, 0.5, "0", "zeros"), (220, 3, 1e-3, "1", "random"), (236, 20, 10.0, "0", "onehot"),
    (206, 2, 0.5, "1", "onehot"), (234, 33, 0.5, "0", "zeros"),
]


def _exact_gain(AD, DP, ID, rows, pc):
    """variant_ELBO_gain of the listed variants at 40 digits: the products with ID_prob summed exactly
    (integers), digamma / exp / log in mpmath"""
    import mpmath
    mpmath.mp.dps = 40
    SH = 1100

    def exact_int(x):                # x * 2^SH as an integer, exactly
        m, e = math.frexp(float(x))
        assert e - 53 + SH >= 0
        return int(m * (1 << 53)) << (e - 53 + SH)

    ints = [[exact_int(x) for x in ID[:, k]] for k in range(ID.shape[1])]
    ADr, DPr = AD.tocsr(), DP.tocsr()
    scale = mpmath.mpf(2) ** SH
    pc = mpmath.mpf(pc)              # (the float64 the device is given)

    def term(ad, dp):
        s1, s2, ss = ad + pc, (dp - ad) + pc, dp + 2 * pc
        return s1 * mpmath.digamma(s1) + s2 * mpmath.digamma(s2) - ss * mpmath.digamma(ss)

    out = []
    for n in rows:
        a = dict(zip(ADr.indices[ADr.indptr[n]:ADr.indptr[n + 1]].tolist(),
                     ADr.data[ADr.indptr[n]:ADr.indptr[n + 1]].tolist()))
        cells = DPr.indices[DPr.indptr[n]:DPr.indptr[n + 1]].tolist()
        dps = DPr.data[DPr.indptr[n]:DPr.indptr[n + 1]].tolist()
        ads = [a.get(c, 0) for c in cells]
        terms = []
        for col in ints:
            v = [col[c] for c in cells]
            terms.append(term(mpmath.mpf(sum(x * y for x, y in zip(ads, v))) / scale,
                              mpmath.mpf(sum(x * y for x, y in zip(dps, v))) / scale))
        mx = max(terms)
        lse = mx + mpmath.log(sum(mpmath.exp(t - mx) for t in terms))
        out.append(lse - term(mpmath.mpf(sum(ads)), mpmath.mpf(sum(dps))))
    return out


@pytest.mark.parametrize("seed,K,pc,lds,kind", GAIN_CASES)
def test_elbo_gain_and_donor_reads(va, monkeypatch, seed, K, pc, lds, kind):
    import mpmath
    from vireo_amd import variant_ELBO_gain
    from vireo_amd.counts import DeviceCounts
    AD, DP, _, rng = draw_case(seed)
    N, M = AD.shape
    monkeypatch.setenv("VIREO_LDS", lds)
    ID = _id_prob(rng, M, K, kind)
    counts = DeviceCounts(AD, DP)

    # donor reads: AD @ ID, DP @ ID
    A_dev, D_dev = counts.donor_reads(ID)
    np.testing.assert_allclose(A_dev, AD @ ID, rtol=1e-12, atol=0)
    np.testing.assert_allclose(D_dev, DP @ ID, rtol=1e-12, atol=0)

    gain = variant_ELBO_gain(ID, counts, None, pseudocount=pc)
    counts.close()
    g_np = A.elbo_gain(ID, AD, DP, pseudocount=pc)
    assert gain.shape == g_np.shape == (N,) and np.all(np.isfinite(gain))

    # a sample of variants against 40 digits: the deepest, random ones, an empty one
    depth = np.asarray(DP.sum(1)).ravel()
    rows = np.unique(np.concatenate([np.argsort(depth)[-8:], rng.choice(N, 8, replace=False),
                                     np.flatnonzero(depth == 0)[:1]]))
    exact = _exact_gain(AD, DP, ID, rows, pc)
    floor = np.array([1e-9 + 1e-12 * float(abs(x)) for x in exact])        # the tolerance of the c1 fixture
    e_dev = np.array([float(abs(mpmath.mpf(float(g)) - x)) for g, x in zip(gain[rows], exact)])
    e_np = np.array([float(abs(mpmath.mpf(float(g)) - x)) for g, x in zip(g_np[rows], exact)])
    i, j = int(np.argmax(e_dev)), int(np.argmax(e_np))
    print("seed %d, %d columns, pseudocount %g, %s ID_prob: %d variants against 40 digits; worst device error %.3g "
          "(variant of %.3g reads, gain %.6g; float64 there %.3g), worst float64 error %.3g (variant of %.3g reads); "
          "in units of the fixture tolerance: device %.3g, float64 %.3g"
          % (seed, K, pc, kind, rows.size, e_dev[i], depth[rows[i]], float(exact[i]), e_np[i], e_np[j],
             depth[rows[j]], (e_dev / floor).max(), (e_np / floor).max()))
    assert (e_dev / floor).max() <= max(1.0, 4.0 * (e_np / floor).max())

    # all variants: within that error of the restatement, and the same selection wherever the gain is not
    # within it of the threshold
    bound = (1e-9 + 1e-12 * np.abs(g_np)) * max(1.0, 5.0 * (e_np / floor).max())      # (device 4 x + float64 1 x)
    assert np.all(np.abs(gain - g_np) <= bound), np.max(np.abs(gain - g_np) / bound)
    threshold = np.sqrt(M) / 3.0
    clear = np.abs(g_np - threshold) > bound
    print("  threshold %.3f: %d of %d variants selected, %d too close to call" % (threshold, (g_np >= threshold).sum(),
                                                                              N, (~clear).sum()))
    assert np.array_equal((gain >= threshold)[clear], (g_np >= threshold)[clear])
    for r, x in zip(rows, exact):
        if abs(float(x) - threshold) > bound[r]:
            assert (gain[r] >= threshold) == (x >= threshold)
