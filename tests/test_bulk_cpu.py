"""VireoBulk / LikRatio_test without a GPU: the fixtures' own condition, the NumPy restatement
(tests/bulk_np.py) against every fixture, the package surface, the constructor's random draws and
the argument checks that run before any device call."""
import contextlib
import io

import numpy as np
import pytest

from tests import bulk_np as B
from tests import gold


@pytest.fixture(scope="module")
def c1():
    return B.c1_bulk()


@pytest.mark.parametrize("name", B.FIT_CASES)
def test_fixture_stop_margin(name):
    """a fixture in which the stop rule fires cannot flip its iteration count on rounding alone"""
    g = gold.load(name)
    fit = B.fixture_inputs(g)[4]
    margin = B.stop_margin(g["logLik_all"], g["logLik"], fit.get("min_iter", 5), fit.get("epsilon_conv", 1e-3))
    if np.isfinite(g["stop_margin"]):
        assert margin == g["stop_margin"]
    stopped = len(g["logLik_all"]) < fit.get("max_iter", 200) - 1
    assert stopped == bool(g["stopped"])
    if stopped:
        assert g["stop_margin"] >= 1e-6


def test_both_paths_are_fixtures():
    """the stop rule fires in some fixtures and the loop runs to max_iter in others"""
    stopped = [bool(gold.load(n)["stopped"]) for n in B.FIT_CASES]
    assert any(stopped) and not all(stopped)


@pytest.mark.parametrize("name", B.FIT_CASES)
def test_restatement_reproduces_fixture(name):
    g = gold.load(name)
    AD, DP, GT, ctor, fit = B.fixture_inputs(g)
    np.random.seed(int(g["seed"]))
    psi0, theta0 = B.init(int(g["n_donor"]), int(g["n_GT"]), **ctor)
    assert np.array_equal(psi0, g["psi0"]) and np.array_equal(theta0, g["theta0"])
    assert np.random.rand() == float(g["next_rand"])
    r = B.fit(AD, DP, GT, psi0, theta0, **fit)
    assert len(r["logLik_all"]) == len(g["logLik_all"])
    assert np.array_equal(np.isnan(r["psi"]), np.isnan(g["psi"]))
    for key in ("psi", "theta", "logLik", "logLik_all"):
        want = np.asarray(g[key])
        ok = np.array_equal(r[key], want, equal_nan=True) or \
            np.allclose(r[key], want, rtol=1e-13, atol=1e-13, equal_nan=True)
        assert ok, key


def test_restatement_one_pass_schedule_matches(c1):
    """the chunked one-pass schedule (what the device runs) gives the literal loop's iteration count"""
    g = gold.load("c1_bulk_notheta")
    AD, DP, GT = c1
    for dtype in (np.float64, np.longdouble):
        r = B.fit_chunked(AD, DP, GT, g["psi0"], g["theta0"], learn_theta=False, dtype=dtype, chunk=1000, threads=2)
        assert r["it"] == len(g["logLik_all"])
        np.testing.assert_allclose(r["psi"].astype(float), g["psi"], rtol=0, atol=1e-12)
        np.testing.assert_allclose(np.asarray(r["logLik_all"], float), g["logLik_all"], rtol=1e-12)


def test_restatement_one_pass_schedule_with_theta_matches(c1):
    """the arbiter's learn_theta=True branch (the full-size max_iter=8 tests use it) against a fixture"""
    g = gold.load("c1_bulk_maxiter8")
    AD, DP, GT = c1
    for dtype in (np.float64, np.longdouble):
        r = B.fit_chunked(AD, DP, GT, g["psi0"], g["theta0"], max_iter=8, dtype=dtype, chunk=1000, threads=2)
        assert r["it"] == len(g["logLik_all"]) == 7
        np.testing.assert_allclose(r["psi"].astype(float), g["psi"], rtol=0, atol=1e-12)
        np.testing.assert_allclose(r["theta"].astype(float), g["theta"], rtol=0, atol=1e-12)
        np.testing.assert_allclose(float(r["logLik"]), g["logLik"], rtol=1e-12)
        np.testing.assert_allclose(np.asarray(r["logLik_all"], float), g["logLik_all"], rtol=1e-12)
    g = gold.load("c1_bulk_delay3")
    r = B.fit_chunked(AD, DP, GT, g["psi0"], g["theta0"], delay_fit_theta=3, max_iter=12, dtype=np.float64,
                      chunk=1000, threads=2)
    np.testing.assert_allclose(np.asarray(r["logLik_all"], float), g["logLik_all"][:11], rtol=1e-12)


def test_restatement_lik_ratio(c1):
    g = gold.load("c1_bulk_lr")
    AD, DP, GT = c1
    for i, null in enumerate(g["nulls"]):
        LR, p = B.lik_ratio(g["psi"], null, AD, DP, GT, g["theta"])
        _, lp = B.lik_ratio(g["psi"], null, AD, DP, GT, g["theta"], log=True)
        assert 0.0 < g["pvalue"][i] < 1.0
        np.testing.assert_allclose(LR, g["LR"][i], rtol=1e-10)
        np.testing.assert_allclose(p, g["pvalue"][i], rtol=1e-8)
        np.testing.assert_allclose(lp, g["log_pvalue"][i], rtol=1e-8)
    LR, _ = B.lik_ratio(g["psi"], np.full(4, 0.25), AD, DP, GT, g["theta"])
    np.testing.assert_allclose(LR, g["uniform_LR"], rtol=1e-10)


def test_package_surface():
    import vireo_amd
    for name in ("VireoBulk", "LikRatio_test"):
        assert hasattr(vireo_amd, name) and name in vireo_amd.__all__
    assert callable(vireo_amd.VireoBulk.fit) and callable(vireo_amd.VireoBulk.LR_test)


@pytest.mark.parametrize("name", B.FIT_CASES)
def test_constructor_draws_equal_reference(name):
    """psi, theta and the RNG state after the constructor equal the reference's (host only)"""
    from vireo_amd import VireoBulk
    g = gold.load(name)
    ctor = B.fixture_inputs(g)[3]
    np.random.seed(int(g["seed"]))
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        m = VireoBulk(int(g["n_donor"]), n_GT=int(g["n_GT"]), **ctor)
    assert np.array_equal(np.asarray(m.psi, float), g["psi0"])
    assert np.array_equal(np.asarray(m.theta, float), g["theta0"])
    assert np.random.rand() == float(g["next_rand"])
    assert out.getvalue() == str(g["ctor_warning"])
    assert (m.n_donor, m.n_GT) == (int(g["n_donor"]), int(g["n_GT"]))


def test_constructor_warnings_text():
    g = gold.load("c1_bulk_badinit")
    assert str(g["ctor_warning"]) == "Warning: n_donor != len(psi_init)\nWarning: n_GT != len(theta_init)\n"


def test_argument_errors_before_any_device_call(c1, monkeypatch):
    import vireo_amd
    from vireo_amd import _lib, VireoBulk, LikRatio_test, device_bulk

    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(_lib, "lib", no_device)
    monkeypatch.setattr(_lib, "require_gpu", no_device)
    AD, DP, GT = c1
    np.random.seed(0)
    m = VireoBulk(4)
    bad = [
        dict(AD=AD[:-1], DP=DP, GT_prob=GT),                       # lengths differ
        dict(AD=AD, DP=DP, GT_prob=GT[:-1]),                       # variants differ
        dict(AD=AD, DP=DP, GT_prob=GT[:, :3]),                     # donors differ from the model
        dict(AD=AD, DP=DP, GT_prob=GT[:, :, :2]),                  # genotypes differ from the model
        dict(AD=AD, DP=DP, GT_prob=GT[:, :, 0]),                   # not 3-D
        dict(AD=AD[:, None], DP=DP[:, None], GT_prob=GT),          # not vectors
        dict(AD=AD.astype(str), DP=DP, GT_prob=GT),                # dtype
        dict(AD=AD, DP=DP, GT_prob=GT.astype(complex)),            # dtype
        dict(AD=AD, DP=None, GT_prob=None),                        # arrays need all three
        dict(AD=AD, DP=DP, GT_prob=GT, max_iter=0),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            m.fit(**kw)
    psi, theta = np.full(4, 0.25), [0.01, 0.5, 0.99]
    for kw in [dict(psi=psi[:3], psi_null=psi, AD=AD, DP=DP, GT_prob=GT, theta=theta),
               dict(psi=psi, psi_null=psi[:3], AD=AD, DP=DP, GT_prob=GT, theta=theta),
               dict(psi=psi, psi_null=psi, AD=AD, DP=DP, GT_prob=GT, theta=theta[:2]),
               dict(psi=psi, psi_null=psi, AD=AD, DP=DP[:-1], GT_prob=GT, theta=theta),
               dict(psi=psi, psi_null=psi, AD=AD, DP=DP, GT_prob=None, theta=theta)]:
        with pytest.raises(ValueError):
            LikRatio_test(**kw)
    with pytest.raises(ValueError):
        m.LR_test(psi_null=psi[:2], AD=AD, DP=DP, GT_prob=GT)
    with pytest.raises(ValueError):
        device_bulk(AD, DP, GT[:5])
    assert vireo_amd.BulkData is not None
