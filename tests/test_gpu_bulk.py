"""VireoBulk / LikRatio_test on the MI355X against the reference's fixtures
(tests/golden/make_bulk_golden.py) and, at full size where the reference cannot run, the NumPy
restatement tests/bulk_np.py with np.longdouble as arbiter."""
import contextlib
import io

import numpy as np
import pytest

from tests import bulk_np as B
from tests import gold

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def c1():
    return B.c1_bulk()


def _model(g, ctor):
    from vireo_amd import VireoBulk
    np.random.seed(int(g["seed"]))
    with contextlib.redirect_stdout(io.StringIO()):
        return VireoBulk(int(g["n_donor"]), n_GT=int(g["n_GT"]), **ctor)


@pytest.mark.parametrize("name", B.FIT_CASES)
def test_fit_matches_fixture(name):
    g = gold.load(name)
    AD, DP, GT, ctor, fit = B.fixture_inputs(g)
    m = _model(g, ctor)
    m.fit(AD, DP, GT, **fit)
    print("%s: it %d (fixture %d)  max |psi - ref| %.3g  max |theta - ref| %.3g  logLik rel %.3g"
          % (name, len(m.logLik_all), len(g["logLik_all"]), np.nanmax(np.abs(m.psi - g["psi"]), initial=0),
             np.nanmax(np.abs(np.asarray(m.theta, float) - g["theta"]), initial=0),
             abs(m.logLik - g["logLik"]) / abs(g["logLik"])))
    assert len(m.logLik_all) == len(g["logLik_all"])
    assert np.array_equal(np.isnan(m.psi), np.isnan(g["psi"]))
    assert np.array_equal(np.isnan(np.asarray(m.theta, float)), np.isnan(g["theta"]))
    assert np.array_equal(np.isnan(m.logLik_all), np.isnan(g["logLik_all"]))
    assert np.isnan(m.logLik) == np.isnan(g["logLik"])
    np.testing.assert_allclose(m.psi, g["psi"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(np.asarray(m.theta, float), g["theta"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(m.logLik, g["logLik"], rtol=1e-12)
    np.testing.assert_allclose(m.logLik_all, g["logLik_all"], rtol=1e-12)


def test_nan_fixture_is_nan_throughout():
    g = gold.load("c1_bulk_nan")
    AD, DP, GT, ctor, fit = B.fixture_inputs(g)
    m = _model(g, ctor)
    m.fit(AD, DP, GT, **fit)
    assert np.isnan(m.psi).all() and np.isnan(m.logLik) and np.isnan(m.logLik_all).all()
    assert len(m.logLik_all) == fit["max_iter"] - 1          # no comparison holds: the loop runs out


def test_lik_ratio_matches_fixture(c1):
    from vireo_amd import LikRatio_test, VireoBulk, device_bulk
    g = gold.load("c1_bulk_lr")
    AD, DP, GT = c1
    data = device_bulk(AD, DP, GT)
    np.random.seed(0)
    m = VireoBulk(4)
    m.psi, m.theta = g["psi"], g["theta"]
    for i, null in enumerate(g["nulls"]):
        LR, p = LikRatio_test(g["psi"], null, AD, DP, GT, g["theta"])
        LR2, lp = LikRatio_test(g["psi"], null, AD, DP, GT, g["theta"], log=True)
        print("null %d: LR %.12g (fixture %.12g)  p %.12g (%.12g)  log p %.12g (%.12g)"
              % (i, LR, g["LR"][i], p, g["pvalue"][i], lp, g["log_pvalue"][i]))
        np.testing.assert_allclose(LR, g["LR"][i], rtol=1e-10)
        np.testing.assert_allclose(p, g["pvalue"][i], rtol=1e-8)
        np.testing.assert_allclose(lp, g["log_pvalue"][i], rtol=1e-8)
        assert LR == LR2
        # the handle form, the array form and the method return the same bits
        assert LikRatio_test(g["psi"], null, data, theta=g["theta"]) == (LR, p)
        assert m.LR_test(psi_null=null, AD=AD, DP=DP, GT_prob=GT) == (LR, p)
        assert m.LR_test(psi_null=null, AD=data, log=True) == (LR, lp)
    LR, p = LikRatio_test(g["psi"], np.full(4, 0.25), data, theta=g["theta"])
    np.testing.assert_allclose(LR, g["uniform_LR"], rtol=1e-10)
    print("uniform null: LR %.12g (fixture %.12g)  p %.6g (%.6g)" % (LR, g["uniform_LR"], p, g["uniform_pvalue"]))


def test_many_nulls_in_one_call_equal_single_calls(c1):
    """more psi vectors than one log-likelihood pass takes (eight): same bits as one by one"""
    from vireo_amd import device_bulk
    g = gold.load("c1_bulk_lr")
    data = device_bulk(*c1)
    rng = np.random.default_rng(5)
    psis = rng.dirichlet(np.ones(4), size=19)
    all_at_once = data.loglik(psis, g["theta"])
    one_by_one = np.array([data.loglik(p, g["theta"]) for p in psis])
    assert np.array_equal(all_at_once, one_by_one)
    AD, DP, GT = c1
    want = np.array([B.loglik(AD.astype(float), (DP - AD).astype(float), GT, p, g["theta"]) for p in psis])
    np.testing.assert_allclose(all_at_once, want, rtol=1e-12)


def test_fits_are_bitwise_reproducible_and_set_counts(c1):
    from vireo_amd import VireoBulk, device_bulk
    AD, DP, GT = c1
    g = gold.load("c1_bulk_notheta")

    def run(data, learn_theta=False):
        m = _model(g, {})
        m.fit(data, learn_theta=learn_theta, max_iter=200 if not learn_theta else 40)
        return m
    data = device_bulk(AD, DP, GT)
    a, b = run(data), run(data)
    for key in ("psi", "logLik", "logLik_all"):
        assert np.array_equal(getattr(a, key), getattr(b, key))
    # with the theta sums in play (theta_s1, theta_s2 folded over slices and donors): the same handle
    # twice and a fresh handle, bit for bit
    t1, t2, t3 = run(data, True), run(data, True), run(device_bulk(AD, DP, GT), True)
    assert not np.array_equal(np.asarray(t1.theta, float), g["theta0"])
    for key in ("psi", "theta", "logLik", "logLik_all"):
        assert np.array_equal(getattr(t1, key), getattr(t2, key))
        assert np.array_equal(getattr(t1, key), getattr(t3, key))
    # another sample on the same genotypes, then back: equal to a fresh handle bit for bit
    AD2, DP2 = AD[::-1].copy(), DP[::-1].copy()
    data.set_counts(AD2, DP2)
    c, d = run(data), run(device_bulk(AD2, DP2, GT))
    assert not np.array_equal(c.psi, a.psi)
    for key in ("psi", "logLik", "logLik_all"):
        assert np.array_equal(getattr(c, key), getattr(d, key))
    data.set_counts(AD, DP)
    e = run(data)
    for key in ("psi", "logLik", "logLik_all"):
        assert np.array_equal(getattr(e, key), getattr(a, key))
    assert isinstance(a, VireoBulk)


def test_second_fit_continues_from_the_fitted_state(c1):
    """fit(max_iter=8) twice equals the restatement run twice from the fitted state, as in the reference"""
    AD, DP, GT = c1
    g = gold.load("c1_bulk_maxiter8")
    m = _model(g, {})
    m.fit(AD, DP, GT, max_iter=8)
    np.testing.assert_allclose(m.psi, g["psi"], rtol=0, atol=1e-12)
    m.fit(AD, DP, GT, max_iter=8)
    r = B.fit(AD, DP, GT, g["psi"], g["theta"], max_iter=8)
    np.testing.assert_allclose(m.psi, r["psi"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(m.theta, r["theta"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(m.logLik_all, r["logLik_all"], rtol=1e-12)


def test_verbose_prints_one_warning_per_decreasing_iteration(c1, capsys):
    """min_iter=0 lets the rule see the early iterations, where the reference's theta path decreases"""
    AD, DP, GT = c1
    g = gold.load("c1_bulk_seed1")
    fit = dict(min_iter=0, max_iter=30, epsilon_conv=0.0)
    m = _model(g, {})
    capsys.readouterr()
    m.fit(AD, DP, GT, verbose=True, **fit)
    out = capsys.readouterr().out
    ll = np.append(m.logLik_all, m.logLik)
    assert len(ll) == 30
    decreases = sum(1 for i in range(1, 30) if ll[i] < ll[i - 1])
    assert decreases > 0
    assert out.count("Warning: logLikelihood decreases!\n\n") == decreases
    assert out.count("Warning: VB did not converge!\n\n") == (0 if ll[29] < ll[28] else 1)
    want = B.fit(AD, DP, GT, g["psi0"], g["theta0"], **fit)["warnings"]
    assert out == "".join(w + "\n" for w in want)                # (print adds its own newline)
    m2 = _model(g, {})
    m2.fit(AD, DP, GT, **fit)
    assert capsys.readouterr().out == ""
    assert np.array_equal(m2.psi, m.psi)


def test_generic_instances_small_shapes():
    """shapes off the fast paths: one donor, n_GT = 2 / 5, more columns than lanes, an odd variant count"""
    from vireo_amd import VireoBulk
    for n_var, K, G in [(1, 1, 2), (77, 1, 3), (501, 3, 5), (333, 100, 3), (64, 2, 2), (1001, 37, 4)]:
        AD, DP, GT, psi, theta = B.synth_pool(n_var, K, G, seed=n_var, private=False)
        np.random.seed(3)
        m = VireoBulk(K, n_GT=G, theta_init=list(theta))
        psi0 = m.psi.copy()
        m.fit(AD, DP, GT, max_iter=12, min_iter=2)
        r = B.fit(AD, DP, GT, psi0, theta, max_iter=12, min_iter=2)
        assert len(m.logLik_all) == len(r["logLik_all"]), (n_var, K, G)
        np.testing.assert_allclose(m.psi, r["psi"], rtol=0, atol=1e-12)
        np.testing.assert_allclose(np.asarray(m.theta, float), r["theta"], rtol=0, atol=1e-12)
        np.testing.assert_allclose(m.logLik, r["logLik"], rtol=1e-12)


def test_verbose_at_iteration_zero_with_negative_min_iter(c1, capsys):
    """min_iter < 0: the reference's rule also looks at iteration 0, against logLik[-1] (still 0 there);
    the device's stop rule and the replayed warnings must agree with the restatement on it"""
    AD, DP, GT = c1
    g = gold.load("c1_bulk_seed1")
    fit = dict(min_iter=-1, max_iter=10, epsilon_conv=0.0)
    m = _model(g, {})
    capsys.readouterr()
    m.fit(AD, DP, GT, verbose=True, **fit)
    out = capsys.readouterr().out
    r = B.fit(AD, DP, GT, g["psi0"], g["theta0"], **fit)
    assert len(m.logLik_all) == len(r["logLik_all"])
    assert r["warnings"][0] == "Warning: logLikelihood decreases!\n"      # (a negative logLik[0] < 0)
    assert out == "".join(w + "\n" for w in r["warnings"])


def test_donor_count_at_and_beyond_the_lds_limit():
    """n_donor x n_GT is bounded by the 64 KiB of LDS a workgroup takes: 454 donors at n_GT = 3
    fit and agree with the restatement, 455 fail at create with a message that says why"""
    from vireo_amd import VireoBulk, device_bulk
    from vireo_amd._lib import VrxError
    AD, DP, GT, psi, theta = B.synth_pool(51, 454, 3, seed=4, private=False)
    np.random.seed(3)
    m = VireoBulk(454, theta_init=list(theta))
    psi0 = m.psi.copy()
    m.fit(AD, DP, GT, max_iter=6)
    r = B.fit(AD, DP, GT, psi0, theta, max_iter=6)
    np.testing.assert_allclose(m.psi, r["psi"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(m.theta, r["theta"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(m.logLik, r["logLik"], rtol=1e-12)
    AD, DP, GT, psi, theta = B.synth_pool(51, 455, 3, seed=4, private=False)
    with pytest.raises(VrxError, match="bytes of LDS per workgroup"):
        device_bulk(AD, DP, GT)


# ---- full size --------------------------------------------------------------------------------------
# (n_var, n_donor, n_GT, seed of the pool).  The arbiter is tests/bulk_np.fit_chunked in np.longdouble; the
# same code in float64 gives the error a float64 evaluation in another summation order has.
FULL = [(1_000_000, 16, 3, 0), (300_001, 37, 3, 1), (200_003, 5, 4, 2)]


def _errors(dev, f64, arb):
    """(device error, float64-NumPy error) against the arbiter for psi, theta, relative logLik"""
    out = {}
    for key in ("psi", "theta"):
        a = np.asarray(arb[key], np.longdouble)
        out[key] = (float(np.abs(np.asarray(dev[key], np.longdouble) - a).max()),
                    float(np.abs(np.asarray(f64[key], np.longdouble) - a).max()))
    a = np.longdouble(arb["logLik"])
    out["logLik"] = (float(abs((np.longdouble(dev["logLik"]) - a) / a)),
                     float(abs((np.longdouble(f64["logLik"]) - a) / a)))
    return out


def _full(n_var, K, G, seed, **fit):
    from vireo_amd import VireoBulk, device_bulk
    AD, DP, GT, psi, theta = B.synth_pool(n_var, K, G, seed=seed, private=False)
    np.random.seed(1)
    m = VireoBulk(K, n_GT=G, theta_init=list(theta))
    psi0 = m.psi.copy()
    m.fit(device_bulk(AD, DP, GT), **fit)
    dev = dict(psi=m.psi, theta=np.asarray(m.theta, float), logLik=m.logLik, it=len(m.logLik_all))
    arb = B.fit_chunked(AD, DP, GT, psi0, theta, dtype=np.longdouble, **fit)
    f64 = B.fit_chunked(AD, DP, GT, psi0, theta, dtype=np.float64, **fit)
    return dev, f64, arb, (AD, DP, GT, psi, theta)


@pytest.mark.parametrize("n_var,K,G,seed", FULL)
def test_full_size_eight_iterations(n_var, K, G, seed):
    dev, f64, arb, _ = _full(n_var, K, G, seed, max_iter=8)
    assert dev["it"] == arb["it"] == 7
    for key, (e_dev, e_np) in _errors(dev, f64, arb).items():
        print("%d x %d x %d max_iter=8 %s: err_gpu %.3g  err_float64_numpy %.3g" % (n_var, K, G, key, e_dev, e_np))
        assert e_dev <= max(1e-12, 4 * e_np), key


@pytest.mark.parametrize("n_var,K,G,seed", FULL)
def test_full_size_fixed_theta_to_convergence(n_var, K, G, seed):
    """learn_theta=False until the stop rule fires, against the arbiter.  epsilon_conv is the default's
    tolerance per variant on the c1 fixtures (1e-3 on 3 784 variants) scaled to the pool: the EM of many
    overlapping donors gains slowly, and the arbiter's np.longdouble passes are what bounds this test."""
    eps = 1e-3 * n_var / 3784
    fit = dict(learn_theta=False, epsilon_conv=eps, max_iter=2000)
    dev, f64, arb, _ = _full(n_var, K, G, seed, **fit)
    margin = B.stop_margin(np.asarray(arb["logLik_all"], float), float(arb["logLik"]), 5, eps)
    print("%d x %d x %d converged: it gpu %d arbiter %d float64 %d, arbiter stop margin %.3g"
          % (n_var, K, G, dev["it"], arb["it"], f64["it"], margin))
    assert arb["it"] < 1999 and margin >= 1e-6
    assert dev["it"] == arb["it"]
    for key, (e_dev, e_np) in _errors(dev, f64, arb).items():
        print("  %s: err_gpu %.3g  err_float64_numpy %.3g" % (key, e_dev, e_np))
        assert e_dev <= max(1e-12, 4 * e_np), key


def test_full_size_planted_psi_recovered():
    """learn_theta=False with the planting theta and the default epsilon_conv, on the device alone (thousands
    of passes): the planted abundances within 3 standard errors of the binomial sampling noise at the
    planted depths."""
    from vireo_amd import VireoBulk
    n_var, K, G, seed = FULL[0]
    AD, DP, GT, psi, theta = B.synth_pool(n_var, K, G, seed=seed, private=False)
    np.random.seed(1)
    m = VireoBulk(K, n_GT=G, theta_init=list(theta))
    m.fit(AD, DP, GT, learn_theta=False, max_iter=20000)
    se = B.psi_standard_error(DP, GT, psi, theta)
    z = np.abs(m.psi - psi) / se
    print("planted psi: %d iterations, max |psi - planted| / se = %.3f (se %.3g .. %.3g), %.1f ms"
          % (len(m.logLik_all), z.max(), se.min(), se.max(), m.fit_ms_))
    assert len(m.logLik_all) < 19999                     # the stop rule fired
    assert z.max() <= 3.0
