"""VireoBulkCohort without a GPU: the cohort fixture's own condition (tests/golden/make_bulk_cohort_golden.py),
the NumPy restatement (tests/bulk_np.py) sample by sample against it, the constructor's random draws, the
package surface, the argument checks that run before any device call and the new names of the C ABI."""
import contextlib
import io
import os
import re

import numpy as np
import pytest

from tests import bulk_np as B
from tests import gold

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COHORT_ABI = {"vrx_bulk_set_cohort": 4, "vrx_bulk_cohort_chunk": 0, "vrx_bulk_fit_cohort": 11,
              "vrx_bulk_loglik_cohort": 5, "vrx_bulk_info": 2}


@pytest.fixture(scope="module")
def cohort():
    g = gold.load("c1_bulk_cohort")
    g["GT"] = B.c1_bulk()[2]
    cuts = np.cumsum(g["n_all"])[:-1]
    g["logLik_all"] = np.split(g["logLik_all_flat"], cuts)
    return g


def test_fixture_shape_and_stop_margin(cohort):
    """six samples, the last of zero depth; every finite sample's stop rule cannot flip on rounding alone"""
    g = cohort
    assert g["AD"].shape == g["DP"].shape == (6, 3784) and g["GT"].shape == (3784, 4, 3)
    assert (g["DP"][:5].sum(1) > 0).all() and not g["DP"][5].any()
    assert [len(x) for x in g["logLik_all"]] == g["n_all"].tolist()
    stopped = g["n_all"][:5] < 199
    assert stopped.any() and not stopped.all()          # the samples leave the loop at different iterations
    for s in range(5):
        margin = B.stop_margin(g["logLik_all"][s], g["logLik"][s], 5, 1e-3)
        assert margin == g["stop_margin"][s] and margin >= 1e-6, (s, margin)
    assert np.isnan(g["psi"][5]).all() and np.isnan(g["logLik"][5]) and g["n_all"][5] == 199


def test_restatement_reproduces_fixture_sample_by_sample(cohort):
    g = cohort
    for s in range(6):
        r = B.fit(g["AD"][s], g["DP"][s], g["GT"], g["psi0"][s], g["theta0"][s])
        assert len(r["logLik_all"]) == g["n_all"][s]
        assert np.array_equal(np.isnan(r["psi"]), np.isnan(g["psi"][s]))
        for key, want in (("psi", g["psi"][s]), ("theta", g["theta"][s]), ("logLik", g["logLik"][s]),
                          ("logLik_all", g["logLik_all"][s])):
            ok = np.array_equal(r[key], want, equal_nan=True) or \
                np.allclose(r[key], want, rtol=1e-13, atol=1e-13, equal_nan=True)
            assert ok, (s, key)


def test_restatement_lik_ratio_against_sample_zero(cohort):
    g = cohort
    with np.errstate(all="ignore"):
        for s in range(6):
            LR, p = B.lik_ratio(g["psi"][s], g["psi"][0], g["AD"][s], g["DP"][s], g["GT"], g["theta"][s])
            _, lp = B.lik_ratio(g["psi"][s], g["psi"][0], g["AD"][s], g["DP"][s], g["GT"], g["theta"][s], log=True)
            np.testing.assert_allclose(LR, g["LR"][s], rtol=1e-10)
            np.testing.assert_allclose(p, g["pvalue"][s], rtol=1e-8)
            np.testing.assert_allclose(lp, g["log_pvalue"][s], rtol=1e-8)
    assert g["LR"][0] == 0.0 and np.isnan(g["LR"][5])


def test_constructor_draws_equal_a_loop_of_the_reference(cohort):
    """psi, theta and the RNG state after the constructor equal those of six VireoBulk(4) in a row"""
    from vireo_amd import VireoBulk, VireoBulkCohort
    g = cohort
    np.random.seed(int(g["seed"]))
    m = VireoBulkCohort(6, int(g["n_donor"]), n_GT=int(g["n_GT"]))
    assert m.psi.shape == (6, 4) and m.theta.shape == (6, 3)
    assert np.array_equal(m.psi, g["psi0"]) and np.array_equal(m.theta, g["theta0"])
    assert np.random.rand() == float(g["next_rand"])
    assert (m.n_sample, m.n_donor, m.n_GT) == (6, 4, 3)
    # every constructor argument: the same draws as the loop, the warnings once
    for ctor in (dict(theta_init=None), dict(psi_init=[0.1, 0.2, 0.3, 0.4]),
                 dict(psi_init=[0.5, 0.5], theta_init=[0.1, 0.9])):
        np.random.seed(7)
        with contextlib.redirect_stdout(io.StringIO()) as loop_out:
            loop = [VireoBulk(4, **ctor) for _ in range(3)]
        after = np.random.rand()
        np.random.seed(7)
        with contextlib.redirect_stdout(io.StringIO()) as out:
            m = VireoBulkCohort(3, 4, **ctor)
        assert np.random.rand() == after
        assert np.array_equal(m.psi, np.array([x.psi for x in loop]))
        assert np.array_equal(m.theta, np.array([np.asarray(x.theta, float) for x in loop]))
        assert out.getvalue() * 3 == loop_out.getvalue()


def test_package_surface():
    import vireo_amd
    assert hasattr(vireo_amd, "VireoBulkCohort") and "VireoBulkCohort" in vireo_amd.__all__
    assert "VireoBulkCohort" in vireo_amd.vireo_bulk.__all__
    for name in ("fit", "LR_test"):
        assert callable(getattr(vireo_amd.VireoBulkCohort, name))
    for name in ("set_cohort", "fit_cohort", "loglik_cohort"):
        assert callable(getattr(vireo_amd.BulkData, name))


def test_argument_errors_before_any_device_call(cohort, monkeypatch):
    from vireo_amd import _lib, VireoBulkCohort

    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(_lib, "lib", no_device)
    monkeypatch.setattr(_lib, "require_gpu", no_device)
    g = cohort
    AD, DP, GT = g["AD"], g["DP"], g["GT"]
    np.random.seed(0)
    m = VireoBulkCohort(6, 4)
    bad = [
        dict(AD=AD[0], DP=DP[0], GT_prob=GT),                       # 1-D AD
        dict(AD=AD, DP=DP[:5], GT_prob=GT),                         # shapes differ
        dict(AD=AD[:, :-1], DP=DP, GT_prob=GT),                     # shapes differ
        dict(AD=AD[:5], DP=DP[:5], GT_prob=GT),                     # samples differ from the model
        dict(AD=AD, DP=DP, GT_prob=GT[:-1]),                        # variants differ from GT_prob
        dict(AD=AD, DP=DP, GT_prob=GT[:, :3]),                      # donors differ from the model
        dict(AD=AD, DP=DP, GT_prob=GT[:, :, :2]),                   # genotypes differ from the model
        dict(AD=AD.astype(str), DP=DP, GT_prob=GT),                 # dtype
        dict(AD=AD, DP=DP.astype(complex), GT_prob=GT),             # dtype
        dict(AD=AD, DP=DP, GT_prob=GT.astype(complex)),             # dtype
        dict(AD=AD, DP=None, GT_prob=None),                         # arrays need all three
        dict(AD=AD, DP=DP, GT_prob=GT, max_iter=0),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            m.fit(**kw)
    for null in (np.full(3, 1 / 3), np.full((5, 4), 0.25), np.full((6, 4, 1), 0.25), np.full(4, "a")):
        with pytest.raises(ValueError):
            m.LR_test(null, AD, DP, GT)
    for kw in bad[:11]:
        with pytest.raises(ValueError):
            m.LR_test(np.full(4, 0.25), **kw)
    m.psi = m.psi[:5]
    with pytest.raises(ValueError):
        m.fit(AD, DP, GT)
    with pytest.raises(ValueError):
        VireoBulkCohort(0, 4)


def test_cohort_abi_is_declared_with_matching_arity():
    from vireo_amd import _lib
    text = open(os.path.join(ROOT, "include", "vireo_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, arity in COHORT_ABI.items():
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, text)
        assert m, name + " is not declared in vireo_hip.h"
        args = m.group(1).strip()
        n = 0 if args in ("", "void") else len(args.split(","))
        assert n == arity, (name, n)
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == arity, name
