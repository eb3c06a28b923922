"""VireoBulkCohort on the MI355X: the reference's cohort fixture (tests/golden/make_bulk_cohort_golden.py), the
single-sample fixtures run as one cohort, and -- where the reference has nothing to say -- the NumPy restatement
tests/bulk_np.py sample by sample.  A sample's results must not depend on the rest of the cohort: the
composition tests compare bits."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests import bulk_np as B
from tests import gold

pytestmark = pytest.mark.gpu

BULK_Q = 8           # VRX_BULK_Q (vrx_bulk.h): psi vectors per log-likelihood pass
KEYS = ("psi", "theta", "logLik", "n_iter")


@pytest.fixture(scope="module")
def C():
    from vireo_amd import _lib
    return int(_lib.lib().vrx_bulk_cohort_chunk())


@pytest.fixture(scope="module")
def c1():
    return B.c1_bulk()


@pytest.fixture(scope="module")
def cohort():
    g = gold.load("c1_bulk_cohort")
    g["GT"] = B.c1_bulk()[2]
    g["logLik_all"] = np.split(g["logLik_all_flat"], np.cumsum(g["n_all"])[:-1])
    return g


def pool(n_var, K, G, S, seed):
    """S samples on one GT_prob: fresh Poisson depths and binomial counts per sample, a different planted psi
    each -> AD, DP (S, n_var) int64, GT_prob, theta (planted)"""
    _, _, GT, _, theta = B.synth_pool(n_var, K, G, seed=seed, private=False)
    rng = np.random.default_rng(1000 + seed)
    tm = np.tensordot(GT, theta, axes=(2, 0))
    AD, DP = [], []
    for _ in range(S):
        psi = rng.dirichlet(np.full(K, 2.0))
        dp = rng.poisson(30.0, size=n_var).astype(np.int64)
        AD.append(rng.binomial(dp, tm @ psi).astype(np.int64))
        DP.append(dp)
    return np.array(AD), np.array(DP), GT, theta


def model(S, K, G, psi=None, theta=None, seed=3):
    from vireo_amd import VireoBulkCohort
    np.random.seed(seed)
    m = VireoBulkCohort(S, K, n_GT=G, **({} if theta is None else dict(theta_init=list(theta))))
    if psi is not None:
        m.psi = np.array(psi)
    return m


def same_bits(a, i, b, j):
    """sample i of fitted model a and sample j of b agree in every bit"""
    for key in KEYS:
        assert np.array_equal(getattr(a, key)[i], getattr(b, key)[j], equal_nan=True), key
    assert np.array_equal(a.logLik_all[i], b.logLik_all[j], equal_nan=True)


def against_restatement(m, s, r, tag):
    assert len(m.logLik_all[s]) == len(r["logLik_all"]), tag
    np.testing.assert_allclose(m.psi[s], r["psi"], rtol=0, atol=1e-12, err_msg=str(tag))
    np.testing.assert_allclose(m.theta[s], r["theta"], rtol=0, atol=1e-12, err_msg=str(tag))
    np.testing.assert_allclose(m.logLik[s], r["logLik"], rtol=1e-12, err_msg=str(tag))


def against_fixture(m, s, g_psi, g_theta, g_ll, g_all, tag):
    print("%s: it %d (fixture %d)  max |psi - ref| %.3g  max |theta - ref| %.3g  logLik rel %.3g"
          % (tag, len(m.logLik_all[s]), len(g_all), np.nanmax(np.abs(m.psi[s] - g_psi), initial=0),
             np.nanmax(np.abs(m.theta[s] - g_theta), initial=0), abs(m.logLik[s] - g_ll) / abs(g_ll)))
    assert len(m.logLik_all[s]) == len(g_all) == m.n_iter[s]
    assert np.array_equal(np.isnan(m.psi[s]), np.isnan(g_psi))
    assert np.array_equal(np.isnan(m.theta[s]), np.isnan(g_theta))
    assert np.array_equal(np.isnan(m.logLik_all[s]), np.isnan(g_all))
    assert np.isnan(m.logLik[s]) == np.isnan(g_ll)
    np.testing.assert_allclose(m.psi[s], g_psi, rtol=0, atol=1e-12)
    np.testing.assert_allclose(m.theta[s], g_theta, rtol=0, atol=1e-12)
    np.testing.assert_allclose(m.logLik[s], g_ll, rtol=1e-12)
    np.testing.assert_allclose(m.logLik_all[s], g_all, rtol=1e-12)


def test_reference_fixture_as_one_cohort(cohort):
    """Six samples, one fit.  The ratio test takes the fixture's psi and theta as its operands, as
    test_lik_ratio_matches_fixture does (its tolerances are those of one log-likelihood pass); the figures from
    the device's own fitted values are printed beside them."""
    from vireo_amd import VireoBulkCohort, device_bulk
    g = cohort
    np.random.seed(int(g["seed"]))
    m = VireoBulkCohort(6, 4)
    assert np.random.rand() == float(g["next_rand"])
    data = device_bulk(g["AD"][0], g["DP"][0], g["GT"])
    data.set_cohort(g["AD"], g["DP"])
    m.fit(data)
    for s in range(6):
        against_fixture(m, s, g["psi"][s], g["theta"][s], g["logLik"][s], g["logLik_all"][s], "sample %d" % s)
    assert np.isnan(m.psi[5]).all() and np.isnan(m.logLik[5]) and np.isnan(m.logLik_all[5]).all()
    assert m.n_iter[5] == 199                                   # no comparison holds: the loop runs out
    assert len(set(m.n_iter.tolist())) > 2                      # the samples stopped at different iterations
    own = m.LR_test(m.psi[0], data)
    m.psi, m.theta = g["psi"], g["theta"]
    LR, p = m.LR_test(g["psi"][0], data)
    LR2, lp = m.LR_test(g["psi"][0], g["AD"], g["DP"], g["GT"], log=True)
    for s in range(6):
        print("sample %d: LR %.12g (fixture %.12g; from the device's fit %.12g)  p %.12g (%.12g)  log p %.12g (%.12g)"
              % (s, LR[s], g["LR"][s], own[0][s], p[s], g["pvalue"][s], lp[s], g["log_pvalue"][s]))
    assert LR.shape == p.shape == (6,)
    np.testing.assert_allclose(LR, g["LR"], rtol=1e-10)
    np.testing.assert_allclose(p, g["pvalue"], rtol=1e-8)
    np.testing.assert_allclose(lp, g["log_pvalue"], rtol=1e-8)
    assert np.array_equal(LR, LR2, equal_nan=True)              # the handle form and the array form
    assert LR[0] == 0.0 and np.isnan(LR[5])
    # a null per sample: each against its own psi
    LR, p = m.LR_test(g["psi"], data)
    assert np.array_equal(LR[:5], np.zeros(5)) and np.array_equal(p[:5], np.ones(5))


def test_single_sample_fixtures_as_one_cohort(c1):
    """the c1 counts five times, each from another fixture's start, every sample against its own fixture.  (All
    five fixtures run to max_iter, as the reference does from these starts with learn_theta=True; samples that
    leave the loop at different iterations are in the cohort fixture and in the frozen-sample test.)"""
    names = ["c1_bulk_seed1", "c1_bulk_seed2", "c1_bulk_seed3", "c1_bulk_thetadrawn", "c1_bulk_psiinit"]
    gs = [gold.load(n) for n in names]
    AD, DP, GT = c1
    m = model(5, 4, 3)
    m.psi = np.array([g["psi0"] for g in gs])
    m.theta = np.array([g["theta0"] for g in gs])
    m.fit(np.tile(AD, (5, 1)), np.tile(DP, (5, 1)), GT)
    for s, (name, g) in enumerate(zip(names, gs)):
        against_fixture(m, s, g["psi"], g["theta"], g["logLik"], g["logLik_all"], name)
    assert m.n_iter.tolist() == [len(g["logLik_all"]) for g in gs]


def test_composition_independence(C):
    """S = C + 1: `first` heads the first chunk, `last` sits alone in the second.  In [last, first] they share a
    chunk in other slots; [first] is a chunk of one.  Bits must not move."""
    from vireo_amd import device_bulk
    S, K, G = C + 1, 5, 3
    AD, DP, GT, theta = pool(2001, K, G, S, seed=7)
    fit = dict(max_iter=30, learn_theta=True)
    psi0 = model(S, K, G).psi

    def run(idx, data=None):
        m = model(len(idx), K, G, psi=psi0[idx])
        if data is None:
            m.fit(AD[idx], DP[idx], GT, **fit)
        else:
            m.fit(data, **fit)
        return m
    whole = run(list(range(S)))
    assert not np.array_equal(np.asarray(whole.theta[0]), [0.01, 0.5, 0.99])        # the theta sums are in play
    assert not np.array_equal(whole.psi[0], whole.psi[S - 1])
    pair = run([S - 1, 0])
    solo = run([0])
    same_bits(whole, 0, pair, 1)
    same_bits(whole, 0, solo, 0)
    same_bits(whole, S - 1, pair, 0)
    # the same cohort twice on one handle, and on a fresh handle
    data = device_bulk(AD[0], DP[0], GT)
    data.set_cohort(AD, DP)
    a, b = run(list(range(S)), data), run(list(range(S)), data)
    for s in range(S):
        same_bits(a, s, b, s)
        same_bits(a, s, whole, s)
    # a cohort set over another one replaces it
    data.set_cohort(AD[[S - 1, 0]], DP[[S - 1, 0]])
    c = run([S - 1, 0], data)
    same_bits(c, 1, whole, 0)


def test_a_stopped_sample_is_frozen():
    """One panel, its first 400 variants carried by one donor each, the other 400 shared by all.  The early sample
    has reads on the private half only and stops after about ten iterations; the late one has deep reads on the
    shared half only, where the EM of six overlapping donors gains slowly, and runs to max_iter; a zero-depth
    sample rides along as a non-finite neighbour.  epsilon_conv = 10 sits a whole unit from the early sample's
    nearest gain and sixty from the late one's (tests/bulk_np.stop_margin)."""
    from vireo_amd import device_bulk
    K, G, n = 6, 3, 400
    ad1, dp1, GT1, _, theta = B.synth_pool(n, K, G, seed=2, private=True)
    ad2, dp2, GT2, _, _ = B.synth_pool(n, K, G, seed=3, depth=3000.0, private=False)
    GT = np.concatenate([GT1, GT2])
    z = np.zeros(n, dtype=np.int64)
    AD = np.array([np.concatenate([ad1, z]), np.concatenate([z, ad2]), np.concatenate([z, z])])
    DP = np.array([np.concatenate([dp1, z]), np.concatenate([z, dp2]), np.concatenate([z, z])])
    fit = dict(max_iter=40, learn_theta=False, epsilon_conv=10.0)
    psi0 = model(3, K, G).psi
    with np.errstate(all="ignore"):
        r = [B.fit(AD[s], DP[s], GT, psi0[s], theta, **fit) for s in range(3)]
    margins = [B.stop_margin(x["logLik_all"], x["logLik"], 5, 10.0) for x in r]
    print("on the CPU: iterations %s, stop margins %s" % ([x["it"] for x in r], margins))
    assert 8 <= r[0]["it"] <= 12 and r[1]["it"] == 39 and r[2]["it"] == 39
    assert min(margins) >= 1e-6

    def run(idx):
        m = model(len(idx), K, G, psi=psi0[idx], theta=theta)
        m.fit(AD[idx], DP[idx], GT, **fit)
        return m
    mixed, solo = run([0, 1, 2]), run([0])
    assert mixed.n_iter.tolist() == [x["it"] for x in r]
    for s in range(2):
        against_restatement(mixed, s, r[s], s)
    assert np.isnan(mixed.psi[2]).all()
    same_bits(mixed, 0, solo, 0)
    same_bits(mixed, 1, run([1, 0]), 0)
    # the raw traces: nothing behind a sample's last iteration was written while the others went on
    data = device_bulk(AD[0], DP[0], GT)
    data.set_cohort(AD, DP)
    psi, th, traces, it, ms = data.fit_cohort(psi0, np.tile(theta, (3, 1)), **fit)
    assert traces.shape == (3, 40) and it.tolist() == mixed.n_iter.tolist()
    assert np.array_equal(traces[0, :it[0] + 1], np.append(solo.logLik_all[0], solo.logLik[0]))
    assert (traces[0, :it[0] + 1] != 0).all() and (traces[0, it[0] + 1:] == 0).all()
    assert np.array_equal(psi[0], solo.psi[0]) and np.array_equal(th[0], theta)


def test_shapes_off_the_fast_paths(C):
    """one donor, n_GT = 2 / 5, more columns than lanes, chunks short, full and several, more tiles than resident
    workgroups (the grid stride and the order of the partial sums)"""
    for n_var, K, G, S in [(1, 1, 2, 1), (77, 1, 3, C), (501, 3, 5, C + 1), (333, 100, 3, 2),
                           (1001, 37, 4, 2 * C + 1), (300_001, 5, 4, 3)]:
        AD, DP, GT, theta = pool(n_var, K, G, S, seed=n_var)
        m = model(S, K, G, theta=theta)
        psi0 = m.psi.copy()
        m.fit(AD, DP, GT, max_iter=12, min_iter=2)
        with ThreadPoolExecutor(min(S, 8)) as ex:              # (NumPy drops the GIL in its loops)
            ref = list(ex.map(lambda s: B.fit(AD[s], DP[s], GT, psi0[s], theta, max_iter=12, min_iter=2), range(S)))
        for s in range(S):
            against_restatement(m, s, ref[s], (n_var, K, G, S, s))


def test_loglik_cohort(C):
    """more psi vectors per sample than one pass takes, one chunk and a bit"""
    from vireo_amd import device_bulk
    S, K, G, Q = C + 1, 5, 3, BULK_Q + 3
    AD, DP, GT, theta = pool(1501, K, G, S, seed=11)
    rng = np.random.default_rng(5)
    psis = rng.dirichlet(np.ones(K), size=(S, Q))
    thetas = np.clip(theta[None, :] + rng.uniform(-0.005, 0.005, size=(S, G)), 0.001, 0.999)
    data = device_bulk(AD[0], DP[0], GT)
    data.set_cohort(AD, DP)
    got = data.loglik_cohort(psis, thetas)
    assert got.shape == (S, Q)
    want = np.array([[B.loglik(AD[s].astype(float), (DP[s] - AD[s]).astype(float), GT, psis[s, q], thetas[s])
                      for q in range(Q)] for s in range(S)])
    np.testing.assert_allclose(got, want, rtol=1e-12)
    one_by_one = np.stack([data.loglik_cohort(psis[:, q], thetas) for q in range(Q)], axis=1)
    assert one_by_one.shape == (S, Q) and np.array_equal(got, one_by_one)


def test_single_sample_calls_are_untouched_by_a_cohort(c1, cohort):
    from vireo_amd import device_bulk
    AD, DP, GT = c1
    g = gold.load("c1_bulk_seed1")
    data = device_bulk(AD, DP, GT)
    before = data.fit(g["psi0"], g["theta0"], max_iter=30)
    ll_before = data.loglik(np.stack([g["psi"], g["psi0"]]), g["theta"])
    data.set_cohort(cohort["AD"], cohort["DP"])
    data.fit_cohort(cohort["psi0"], cohort["theta0"], max_iter=10)
    after = data.fit(g["psi0"], g["theta0"], max_iter=30)
    for x, y in zip(before[:4], after[:4]):
        assert np.array_equal(x, y)
    assert np.array_equal(ll_before, data.loglik(np.stack([g["psi"], g["psi0"]]), g["theta"]))


def cohort_lds_bytes(K, G, C, T=2):
    """vrx_bulk_cohort_lds_doubles (vrx_bulk.h) for the smallest tile, in bytes"""
    L = K * G
    n_acc = L if L >= 256 else (256 // L) * L
    return 8 * (C * (4 + K + G + 3 * n_acc) + 1 + T * ((L | 1) + (K | 1) + 2))


def test_donor_count_at_and_beyond_the_lds_limit(C):
    """a chunk's accumulators bound n_donor x n_GT below what the single-sample pass takes: the
    largest donor count whose smallest tile fits 64 KiB fits and agrees with the restatement, one more fails
    when the cohort is set, with a message that says why"""
    from vireo_amd import device_bulk
    from vireo_amd._lib import VrxError
    K = max(k for k in range(1, 455) if cohort_lds_bytes(k, 3, C) <= 64 * 1024)
    assert cohort_lds_bytes(K + 1, 3, C) > 64 * 1024
    if C == 4:
        assert K == 169
    AD, DP, GT, theta = pool(51, K, 3, 2, seed=4)
    m = model(2, K, 3, theta=theta)
    psi0 = m.psi.copy()
    m.fit(AD, DP, GT, max_iter=6)
    for s in range(2):
        against_restatement(m, s, B.fit(AD[s], DP[s], GT, psi0[s], theta, max_iter=6), s)
    AD, DP, GT, theta = pool(51, K + 1, 3, 2, seed=4)
    data = device_bulk(AD[0], DP[0], GT)                        # the single-sample passes take it
    with pytest.raises(VrxError, match="bytes of LDS per workgroup"):
        data.set_cohort(AD, DP)
    with pytest.raises(ValueError):
        data.fit_cohort(np.full((2, K + 1), 1.0 / (K + 1)), np.tile(theta, (2, 1)))
