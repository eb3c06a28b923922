"""Bulk donor-abundance fixtures from the REAL reference (build container only, /root/reference):

    python tests/golden/make_bulk_golden.py

  c1_bulk_*.npz    VireoBulk on the pseudo-bulk of c1 (AD.sum(1), DP.sum(1), 3 784 variants) with the
                   GT_prob of c1_wrap_seed2_init4 (4 donors), or with synthetic genotypes (n_GT = 2; 7
                   donors): the seed, the constructor's psi / theta and the next np.random.rand() after it,
                   the fit's arguments, psi, theta, logLik, logLik_all, and stop_margin = the smallest
                   |gain - epsilon_conv| over the iterations where the stop rule is evaluated
  c1_bulk_nan.npz  a variant whose GT_prob row is all zero and whose depth is positive: NaN throughout
  c1_bulk_lr.npz   LikRatio_test, log=False and log=True, for nulls a few per cent away from a fit
                   (0 < p < 1) and for the uniform null (the statistic only: p = 0 there)

Every fixture in which the stop rule fires must have stop_margin >= 1e-6 (checked here and again by
tests/test_bulk_cpu.py); a case that falls below it gets another seed.  Pure data: numbers only.
Follows make_ambient_golden.py (which it does not change)."""
import contextlib
import io
import os
import sys

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import vireoSNP                                                  # noqa: E402
from vireoSNP import VireoBulk, LikRatio_test                    # noqa: E402
from tests import bulk_np as B                                   # noqa: E402
from tests import gold                                           # noqa: E402

MIN_MARGIN = 1e-6


def save(name, **arrs):
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **arrs)
    size = os.path.getsize(path)
    assert size < 618 * 1024, (name, size)
    print("%-24s %8.1f KB" % (name, size / 1024), end="  ")


def fit_case(name, seed, AD, DP, GT, ctor=None, fit=None, **extra):
    ctor = dict(ctor or {})
    fit = dict(fit or {})
    n_donor, n_GT = GT.shape[1:]
    np.random.seed(seed)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        m = VireoBulk(n_donor, n_GT=n_GT, **ctor)
    psi0, theta0 = np.array(m.psi, float), np.array(m.theta, float)
    next_rand = np.random.rand()
    with np.errstate(all="ignore"):
        m.fit(AD, DP, GT, **fit)
    max_iter, min_iter = fit.get("max_iter", 200), fit.get("min_iter", 5)
    eps = fit.get("epsilon_conv", 1e-3)
    it = len(m.logLik_all)
    stopped = it < max_iter - 1
    margin = B.stop_margin(m.logLik_all, m.logLik, min_iter, eps)
    if stopped:
        assert margin >= MIN_MARGIN, (name, margin)
    rec = dict(seed=np.int64(seed), psi0=psi0, theta0=theta0, next_rand=np.float64(next_rand),
               ctor_warning=np.array(out.getvalue()),
               psi=np.asarray(m.psi, float), theta=np.asarray(m.theta, float), logLik=np.float64(m.logLik),
               logLik_all=np.asarray(m.logLik_all, float), stop_margin=np.float64(margin),
               stopped=np.bool_(stopped), n_donor=np.int64(n_donor), n_GT=np.int64(n_GT))
    for k, v in ctor.items():
        rec["ctor_" + k] = np.array(-1.0) if v is None else np.asarray(v, float)
        rec["ctor_" + k + "_is_none"] = np.bool_(v is None)
    for k, v in fit.items():
        rec["fit_" + k] = np.asarray(v)
    save(name, **rec, **extra)
    print("it %3d  stopped %d  margin %.3g  logLik %.6f" % (it, stopped, margin, m.logLik))
    return m


def synth_gt(n_var, n_donor, n_GT, seed, sharp=0.9):
    """-> (gt_index int8 (n_var, n_donor), sharp): the fixture stores these, B.gt_from_index rebuilds GT_prob"""
    rng = np.random.RandomState(seed)
    return rng.randint(0, n_GT, size=(n_var, n_donor)).astype(np.int8), sharp


def main():
    assert vireoSNP.__version__ == "0.5.9", vireoSNP.__version__
    AD, DP, GT = B.c1_bulk()
    assert AD.shape == (3784,) and GT.shape == (3784, 4, 3)

    for seed in (1, 2, 3):
        fit_case("c1_bulk_seed%d" % seed, seed, AD, DP, GT)
    fit_case("c1_bulk_notheta", 1, AD, DP, GT, fit=dict(learn_theta=False))
    fit_case("c1_bulk_delay3", 1, AD, DP, GT, fit=dict(delay_fit_theta=3))
    fit_case("c1_bulk_maxiter8", 1, AD, DP, GT, fit=dict(max_iter=8))
    fit_case("c1_bulk_min0_eps1", 1, AD, DP, GT, fit=dict(min_iter=0, epsilon_conv=1.0))
    fit_case("c1_bulk_thetadrawn", 1, AD, DP, GT, ctor=dict(theta_init=None))
    fit_case("c1_bulk_psiinit", 1, AD, DP, GT, ctor=dict(psi_init=[0.1, 0.2, 0.3, 0.4]))
    fit_case("c1_bulk_badinit", 1, AD, DP, GT, ctor=dict(psi_init=[0.5, 0.5], theta_init=[0.1, 0.9]),
             fit=dict(learn_theta=False))

    idx, sharp = synth_gt(3784, 4, 2, seed=11)
    fit_case("c1_bulk_gt2", 1, AD, DP, B.gt_from_index(idx, 2, sharp), ctor=dict(theta_init=[0.05, 0.95]),
             fit=dict(learn_theta=False), gt_index=idx, gt_sharp=np.float64(sharp))
    idx, sharp = synth_gt(3784, 7, 3, seed=12)
    fit_case("c1_bulk_k7", 1, AD, DP, B.gt_from_index(idx, 3, sharp), fit=dict(learn_theta=False),
             gt_index=idx, gt_sharp=np.float64(sharp))

    # NaN: variant `row` has an all-zero GT_prob row and positive depth
    row = int(np.flatnonzero(DP > 0)[10])
    GTn = GT.copy()
    GTn[row] = 0.0
    m = fit_case("c1_bulk_nan", 1, AD, DP, GTn, fit=dict(max_iter=12), zero_row=np.int64(row))
    assert np.isnan(m.psi).all() and np.isnan(m.logLik)

    # likelihood ratio: the learn_theta=False fit, nulls a few per cent away from it
    np.random.seed(1)
    m = VireoBulk(4)
    m.fit(AD, DP, GT, learn_theta=False)
    psi, theta = np.asarray(m.psi, float), np.asarray(m.theta, float)
    d = np.array([1.0, -1.0, 0.5, -0.5])
    nulls, LR, pv, lpv = [], [], [], []
    for s in (0.01, 0.02, 0.03, 0.05):
        null = psi * (1 + s * d)
        null = null / null.sum()
        r, p = LikRatio_test(psi, null, AD, DP, GT, theta)
        r2, lp = LikRatio_test(psi, null, AD, DP, GT, theta, log=True)
        assert r == r2
        print("\n  null %.2f: LR %.6f p %.6g log p %.6f" % (s, r, p, lp), end="")
        if 1e-250 < p < 0.999:
            nulls.append(null), LR.append(r), pv.append(p), lpv.append(lp)
    assert len(nulls) >= 2
    uni = np.full(4, 0.25)
    r_uni, p_uni = LikRatio_test(psi, uni, AD, DP, GT, theta)
    r_obj, p_obj = m.LR_test(psi_null=nulls[0], AD=AD, DP=DP, GT_prob=GT)
    assert (r_obj, p_obj) == (LR[0], pv[0])
    print()
    save("c1_bulk_lr", psi=psi, theta=theta, nulls=np.array(nulls), LR=np.array(LR), pvalue=np.array(pv),
         log_pvalue=np.array(lpv), uniform_LR=np.float64(r_uni), uniform_pvalue=np.float64(p_uni))
    print()


if __name__ == "__main__":
    main()
