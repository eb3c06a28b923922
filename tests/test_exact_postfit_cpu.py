"""The post-fit harness checked without a GPU: float64 NumPy stands in the device's place.

* On every output of every case of tests/exact_postfit.py the float64 side (the oracle's pieces,
  SciPy's products, tests/varmix_np.py) stays inside the a-priori bound of recursive summation --
  the longest contracted row or column plus 16 units; for a per-variant mixture the row's covered
  cells take that place.  A degenerate unit or a restatement of something else would show here.
* The rule has teeth: a copy of the float64 arithmetic, made wrong the way a kernel would be, fails
  ``exact_np.held``.  One of the changes asked of this file cannot: see
  ``test_a_start_normalised_once_is_a_rounding``.
* The exact doublet step agrees with the reference's own numbers (tests/golden/synth_dbl_*.npz).
"""
import itertools

import numpy as np
import pytest
from scipy.special import digamma
from scipy.stats import entropy

from oracle import vireo_oracle as O
from tests import exact_postfit as XP
from tests import exact_np as X
from tests import gold
from tests import varmix_np as VN


def _within(tag, name, us, limit):
    print("%s %-24s limit %6d  " % (tag, name, limit) + "  ".join("%s %.2f" % kv for kv in us.items()))
    for k, u in us.items():
        assert u <= limit, (tag, name, k, u)


@pytest.mark.parametrize("name", list(XP.DOUBLET))
def test_doublet_float64_within_a_priori_bound(name):
    p = XP.doublet_problem(name)
    _within("doublet", name, XP.distances(XP.doublet_np(p), XP.doublet_exact(p)), XP.a_priori(p.C))


@pytest.mark.parametrize("name", list(XP.CELL))
def test_cell_loglik_float64_within_a_priori_bound(name):
    p = XP.cell_problem(name)
    _within("cell", name, XP.distances(XP.cell_np(p), XP.cell_exact(p)), XP.a_priori(p.C))


@pytest.mark.parametrize("name", list(XP.READS))
def test_donor_reads_float64_within_a_priori_bound(name):
    p = XP.reads_problem(name)
    _within("reads", name, XP.distances(XP.reads_np(p), XP.reads_exact(p)), XP.a_priori(p.C))


@pytest.mark.parametrize("K", XP.VM_KS)
def test_varmix_float64_within_a_priori_bound(K):
    group = XP.varmix_rows()[2]
    for v, us in enumerate(XP.varmix_row_distances(K, XP.varmix_np(K))):
        _within("varmix K %d" % K, "row %d (%s)" % (v, group[v]), us, XP.varmix_a_priori(v))


def test_cases_are_what_they_say():
    p = XP.doublet_problem("tiny_gt")
    assert (p.GT == 1e-300).any() and (p.GT[::3, 0, 0] * p.GT[::3, 1, 0] == 0).all()      # the products underflow
    p = XP.doublet_problem("one_hot_gt")
    assert set(np.unique(p.GT)) == {0.0, 1.0} and np.all(p.GT.sum(2) == 1)
    p = XP.doublet_problem("sharp_gt_deep")
    out = XP.doublet_np(p)
    assert np.ptp(out["logLik"], axis=1).max() > 745 and (out["prob"] == 0).any()
    p = XP.doublet_problem("ase_T3")
    assert p.psi[0].shape == (p.N, 6)
    assert XP.doublet_problem("K16").n_col == 136 and XP.doublet_problem("K20").n_col == 210
    for key in ("n_col", "n_class"):               # every n_col and every n_class meets every form
        for val in {getattr(sp, key) for sp in XP.CELL.values()}:
            mine = [sp for sp in XP.CELL.values() if getattr(sp, key) == val]
            assert {sp.mode for sp in mine} == set(XP.PRIOR_MODES) and {sp.psi_full for sp in mine} == {False, True}
    for key in ("n_col", "data"):
        for val in {getattr(sp, key) for sp in XP.READS.values()}:
            assert {sp.one_hot for sp in XP.READS.values() if getattr(sp, key) == val} == {False, True}
    AD, DP, group = XP.varmix_rows()
    n = (DP > 0).sum(1)
    for depth in VN.DEPTHS:
        assert sorted(n[[g == "depth%d" % depth for g in group]]) == sorted(XP.VM_LENGTHS)
    rows = XP.varmix_np(3)
    deep = [v for v, g in enumerate(group) if g == "special"][2]
    assert rows[deep]["size"][1] == 0.0 and rows[deep]["beta_sum"][1] == 2.0        # the middle component empties
    assert DP.max() > 1000000


# ---------------------------------------------------------------- the rule has teeth
def _pair_table(GT, drop_last=False, pairs=None):
    """a copy of the oracle's doublet_GT (vireo_doublet.py:105-136) that can be made wrong"""
    T = GT.shape[2]
    gp = np.array(list(itertools.combinations(range(T), 2)))
    sp = np.array(list(itertools.combinations(range(GT.shape[1]), 2)) if pairs is None else pairs)
    g1, g2 = gp[:, 0], gp[:, 1]
    a, b = GT[:, sp[:, 0], :], GT[:, sp[:, 1], :]
    G2 = np.zeros((GT.shape[0], sp.shape[0], T + gp.shape[0]))
    G2[:, :, :T] = a * b
    G2[:, :, T:] = a[:, :, g1] * b[:, :, g2] + a[:, :, g2] * b[:, :, g1]
    G2 = G2 / np.sum(G2[:, :, :-1] if drop_last else G2, axis=2, keepdims=True)
    G1 = np.append(GT, np.zeros((GT.shape[0], GT.shape[1], gp.shape[0])), axis=2)
    return np.append(G1, G2, axis=1)


def _doublet_copy(p, psi=None, prior=None, **kw):
    L = O._cell_loglik(_pair_table(p.GT, **kw), *(x[:, None, :] for x in (psi or p.psi)), p.AD, p.DP)
    return dict(logLik=L, prob=O.softmax_log(L + np.log(p.prior_both if prior is None else prior)))


def _doublet_fails(name, keys, **kw):
    p = XP.doublet_problem(name)
    ex = XP.doublet_exact(p)
    u_orc = XP.distances(XP.doublet_np(p), ex)
    same = XP.distances(_doublet_copy(p), ex)
    assert same == u_orc                             # the copy is the float64 side, to the bit
    u = XP.distances(_doublet_copy(p, **kw), ex)
    for k in keys:
        print("%s corrupted %-7s %.3g units against float64's %.2f" % (name, k, u[k], u_orc[k]))
        assert not X.held(u[k], u_orc[k])


def test_last_mixed_class_left_out_of_the_normaliser_fails():
    _doublet_fails("K4", ("logLik", "prob"), drop_last=True)
    _doublet_fails("T8", ("logLik", "prob"), drop_last=True)          # one class of 36


def test_donor_pairs_in_another_order_fail():
    for name in ("K4", "K5"):
        K = XP.DOUBLET[name].K
        by_second = sorted(itertools.combinations(range(K), 2), key=lambda ab: (ab[1], ab[0]))
        assert by_second != list(itertools.combinations(range(K), 2))
        _doublet_fails(name, ("logLik", "prob"), pairs=by_second)


def test_doublet_prior_not_divided_by_the_pairs_fails():
    for name in ("K4", "prior_cells_rate_half"):
        p = XP.doublet_problem(name)
        prior = np.append(p.ID_prior * (1 - p.rate), np.ones((p.ID_prior.shape[0], p.n_pair)) * p.rate, axis=1)
        _doublet_fails(name, ("prob",), prior=prior)


def test_psi_of_the_neighbouring_class_fails():
    """class 2's digammas in class 1's place, the two shapes 1e-6 apart (relative)"""
    p = XP.doublet_problem("twin_classes")
    psi = [x.copy() for x in p.psi]
    for x in psi:
        assert x[0, 1] != x[0, 2] and abs(x[0, 2] - x[0, 1]) < 1e-5 * abs(x[0, 1])
        x[0, 1] = x[0, 2]
    _doublet_fails("twin_classes", ("logLik",), psi=psi)


def _fit_row_copy(ad, dp, K, max_iter, min_iter, epsilon_conv, weight=None, normalise=2):
    """a copy of tests/varmix_np.fit_row on covered cells (no stop rule: max_iter = 2) that can be made
    wrong: ``weight`` counts an entry that many times in every sum of a pass, ``normalise`` is how
    often the start is normalised"""
    assert max_iter == 2 and min_iter >= 2
    ad, dp = np.asarray(ad, dtype=np.float64), np.asarray(dp, dtype=np.float64)
    bd = dp - ad
    w = np.ones(ad.size) if weight is None else weight
    c = np.arange(K) / (K - 1)
    ID = np.maximum(0.0, 1.0 - np.abs((ad / dp)[:, None] - c[None, :]) * (K - 1)) + 1.0 / 64
    for _ in range(normalise):
        ID = ID / np.sum(ID, axis=1, keepdims=True)
    prior = np.full((ad.size, K), 1.0) / np.sum(np.full((ad.size, K), 1.0), axis=1, keepdims=True)
    trace = np.zeros(max_iter)
    for it in range(max_iter):
        t1 = (w * ad)[None, :] @ ID + 1.0
        t2 = (w * bd)[None, :] @ ID + 1.0
        mu, sm = t1 / (t1 + t2), t1 + t2
        s1, s2 = mu * sm, (1 - mu) * sm
        L = ad[:, None] @ digamma(s1) + bd[:, None] @ digamma(s2) - dp[:, None] @ digamma(s1 + s2)
        Z = L + np.log(prior)
        Z = Z - np.max(Z, axis=1, keepdims=True)
        ID = np.exp(Z)
        ID = ID / np.sum(ID, axis=1, keepdims=True)
        trace[it] = np.sum(w[:, None] * (L * ID)) - np.sum(w * entropy(ID, prior, axis=-1)) - VN._beta_kl_uniform(s1, s2)
    return dict(trace=trace, n_iter=1, warn=0, elbo=trace[0], beta_mu=mu[0], beta_sum=sm[0], size=np.sum(w[:, None] * ID, axis=0))


def test_the_varmix_copy_is_the_restatement():
    for K in (2, 5):
        for got, want in zip(XP.varmix_np(K, fit_row=_fit_row_copy), XP.varmix_np(K)):
            for k in XP.VM_OUTPUTS:
                assert np.array_equal(got[k], want[k]), k


def test_last_odd_entry_counted_twice_fails():
    """the half-filled last pair: the last entry of a row of odd length enters every sum once more,
    at weight 1e-8.  beta_sum and at least one other output show it on every such row (an entry
    without alternate reads on an all-reference row adds next to nothing to the ELBO; ``size``, whose
    unit carries the whole first iteration, shows it on the short rows only)"""
    AD, DP, group = XP.varmix_rows()
    n = (DP > 0).sum(1)
    hit = 0
    for K in (2, 7):
        u_orc = XP.varmix_distances(K, XP.varmix_np(K))
        rows = []
        for v in range(AD.shape[0]):
            cov = DP[v] > 0
            w = np.ones(n[v])
            if n[v] % 2:
                w[-1] += 1e-8
            rows.append(dict(_fit_row_copy(AD[v, cov], DP[v, cov], K, weight=w, **XP.VM_FIT),
                             elbo_one=VN.elbo_one(AD[v, cov], DP[v, cov])))
            rows[-1].update({"trace[0]": rows[-1]["trace"][0], "trace[1]": rows[-1]["trace"][1]})
        for v, us in enumerate(XP.varmix_row_distances(K, rows)):
            if n[v] % 2 and group[v] != "special":
                seen = [k for k in XP.VM_OUTPUTS if not X.held(us[k], u_orc[(group[v], k)])]
                assert "beta_sum" in seen and len(seen) >= 2, (K, v, us)
                hit += 1
    assert hit >= 2 * 3 * 8


def _varmix_start(K, normalise):
    rows = []
    AD, DP, _ = XP.varmix_rows()
    for v in range(AD.shape[0]):
        cov = DP[v] > 0
        r = _fit_row_copy(AD[v, cov], DP[v, cov], K, normalise=normalise, **XP.VM_FIT)
        rows.append({"trace[0]": r["trace"][0], "trace[1]": r["trace"][1], "beta_mu": r["beta_mu"],
                     "beta_sum": r["beta_sum"], "size": r["size"], "elbo_one": VN.elbo_one(AD[v, cov], DP[v, cov])})
    return XP.varmix_distances(K, rows)


def test_a_start_never_normalised_fails():
    for K in (2, 8):
        u_orc, u = XP.varmix_distances(K, XP.varmix_np(K)), _varmix_start(K, 0)
        for g in ("depth3", "depth20", "depth60"):
            assert not X.held(u[(g, "trace[0]")], u_orc[(g, "trace[0]")]), (K, g, u[(g, "trace[0]")])


def test_a_start_normalised_once_is_a_rounding():
    """A start normalised once instead of twice was meant to fail the rule, and cannot: the weights
    of a covered cell add up to 1 + K / 64 (the triangle weights to exactly 1), so after the first
    division the sums are 1 to within two roundings and the second division moves a start value by
    at most those -- inside the 3 EPS the exact side grants the start, and far inside a rule that
    allows four roundings of every output.  Measured on all rows at K = 2 ... 8: no output's
    distance changes by as much as one unit.  What the rule does see is a start that is never
    normalised (the test above).  This test holds the measured fact, so that a change of the units
    that made the difference visible would show."""
    for K in XP.VM_KS:
        u_orc, u = XP.varmix_distances(K, XP.varmix_np(K)), _varmix_start(K, 1)
        for key in u:
            assert abs(u[key] - u_orc[key]) <= 1.0 and X.held(u[key], u_orc[key]), (K, key, u[key], u_orc[key])


# ---------------------------------------------------------------- the restatement against the fixtures
@pytest.mark.parametrize("tag,n_gt,k,ase", [("t2k3", 2, 3, False), ("t4k3", 4, 3, False), ("t5k2", 5, 2, False),
                                            ("t4k5_ase", 4, 5, True), ("t3k4_ase", 3, 4, True)])
def test_exact_doublet_agrees_with_the_golden_fixtures(tag, n_gt, k, ase):
    """synth_dbl_* hold the reference's predict_doublet after a short fit; the extended-precision
    step, fed the fixture's fitted float64 state, lands within the rule's distance of them"""
    g = gold.load("synth_dbl_" + tag)
    AD, DP = gold.unpack(g)
    C = X.Counts(AD, DP)
    GT, mu, sm = g["end_GT_prob"], g["end_beta_mu"], g["end_beta_sum"]
    assert GT.shape == (AD.shape[0], k, n_gt) and mu.shape == (AD.shape[0] if ase else 1, n_gt)
    M, n_pair = AD.shape[1], k * (k - 1) // 2
    psi = XP.doublet_theta(mu, sm)
    prior = XP.doublet_prior(np.full((M, k), 1.0 / k), n_pair, min(0.5, M / 100000))
    ex = X.doublet(C, GT, *psi, prior)
    L = O._cell_loglik(O.doublet_GT(GT), *(x[:, None, :] for x in psi), AD, DP)
    orc = dict(logLik=L, prob=O.softmax_log(L + np.log(prior)))
    golden = np.append(g["singlet_prob"], g["doublet_prob"], axis=1)
    assert np.array_equal(orc["prob"], golden)       # (the pieces are the oracle's step, which is the fixture's)
    u_gold, u_orc = X.distance(golden, *ex["prob"]), X.distance(orc["prob"], *ex["prob"])
    # the log-likelihood ratio: the two maxima of the exact logLik, their units added
    Lx, ux = ex["logLik"]
    i, j = np.argmax(Lx[:, k:], axis=1) + k, np.argmax(Lx[:, :k], axis=1)
    r = np.arange(M)
    u_llr = X.distance(g["doublet_LLR"], Lx[r, i] - Lx[r, j], ux[r, i] + ux[r, j])
    print("synth_dbl_%s: posterior %.2f units, LLR %.2f, logLik of the pieces %.2f; longest row %d"
          % (tag, u_gold, u_llr, X.distance(L, *ex["logLik"]), C.longest))
    assert X.held(u_gold, u_orc) and u_gold <= XP.a_priori(C) and u_llr <= XP.a_priori(C)
