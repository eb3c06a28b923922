"""Bulk cohort fixture from the REAL reference (build container only, /root/reference):

    python tests/golden/make_bulk_cohort_golden.py

  c1_bulk_cohort.npz   six bulk samples on one donor panel, fitted the way users of the reference fit a
                       cohort: a loop of VireoBulk over the samples.  The cells of c1 are split at random
                       (split_seed) into five groups; each group's pseudo-bulk AD / DP is one sample of 3 784
                       variants on the GT_prob of c1_wrap_seed2_init4 (4 donors).  The sixth sample has zero
                       depth everywhere: its psi is 0 / 0 after the first update, NaN throughout.  Under
                       np.random.seed(seed) six VireoBulk(4) are constructed in order, then each is fitted with
                       the default arguments.  Per sample: psi0, theta0, psi, theta, logLik, logLik_all (ragged:
                       logLik_all_flat cut by n_all), stop_margin, and LR_test against sample 0's fitted psi,
                       log=False and log=True; next_rand is np.random.rand() after the last constructor.

Every finite sample must have stop_margin >= 1e-6 (checked here and again by tests/test_bulk_cohort_cpu.py): the
split seed is the first one from SPLIT_SEED0 on that meets it.  Pure data: numbers only.  Follows
make_bulk_golden.py (which it does not change)."""
import os
import sys

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import vireoSNP                                                  # noqa: E402
from vireoSNP import VireoBulk                                   # noqa: E402
from tests import bulk_np as B                                   # noqa: E402
from tests import gold                                           # noqa: E402

MIN_MARGIN = 1e-6
SEED = 1
SPLIT_SEED0 = 0
N_GROUP = 5


def samples(split_seed):
    """-> AD, DP (6, n_var) int64: the pseudo-bulk of five random groups of cells, then a zero-depth sample"""
    AD, DP = gold.c1()
    group = np.random.RandomState(split_seed).randint(0, N_GROUP, size=AD.shape[1])
    ad = [np.asarray(AD[:, group == g].sum(1)).ravel() for g in range(N_GROUP)]
    dp = [np.asarray(DP[:, group == g].sum(1)).ravel() for g in range(N_GROUP)]
    zero = np.zeros_like(ad[0])
    return np.array(ad + [zero], dtype=np.int64), np.array(dp + [zero], dtype=np.int64)


def fit_loop(AD, DP, GT):
    np.random.seed(SEED)
    models = [VireoBulk(GT.shape[1]) for _ in range(AD.shape[0])]
    next_rand = np.random.rand()
    start = [(np.array(m.psi, float), np.array(m.theta, float)) for m in models]
    with np.errstate(all="ignore"):
        for m, ad, dp in zip(models, AD, DP):
            m.fit(ad, dp, GT)
    return models, start, next_rand


def main():
    assert vireoSNP.__version__ == "0.5.9", vireoSNP.__version__
    GT = B.c1_bulk()[2]
    for split_seed in range(SPLIT_SEED0, SPLIT_SEED0 + 20):
        AD, DP = samples(split_seed)
        assert AD.shape == (N_GROUP + 1, 3784) and (DP[:N_GROUP].sum(1) > 0).all() and DP[N_GROUP].sum() == 0
        models, start, next_rand = fit_loop(AD, DP, GT)
        margins = np.array([B.stop_margin(m.logLik_all, m.logLik, 5, 1e-3) for m in models])
        finite = np.array([bool(np.isfinite(m.logLik)) for m in models])
        print("split seed %d: it %s  margins %s" % (split_seed, [len(m.logLik_all) for m in models], margins))
        if (margins[finite] >= MIN_MARGIN).all():
            break
    else:
        raise SystemExit("no split seed meets the stop margin")
    assert finite.tolist() == [True] * N_GROUP + [False]
    stopped = [len(m.logLik_all) < 199 for m in models[:N_GROUP]]
    assert any(stopped) and not all(stopped)             # both ends of the loop, at different iterations
    assert len(models[N_GROUP].logLik_all) == 199 and np.isnan(models[N_GROUP].psi).all()

    null = np.asarray(models[0].psi, float)
    LR, pv, lpv = [], [], []
    with np.errstate(all="ignore"):
        for m, ad, dp in zip(models, AD, DP):
            r, p = m.LR_test(psi_null=null, AD=ad, DP=dp, GT_prob=GT)
            r2, lp = m.LR_test(psi_null=null, AD=ad, DP=dp, GT_prob=GT, log=True)
            assert r == r2 or (np.isnan(r) and np.isnan(r2))
            LR.append(r), pv.append(p), lpv.append(lp)
            print("  LR %.6f  p %.6g  log p %.6f" % (r, p, lp))
    path = os.path.join(HERE, "c1_bulk_cohort.npz")
    np.savez_compressed(
        path, seed=np.int64(SEED), split_seed=np.int64(split_seed), n_donor=np.int64(GT.shape[1]),
        n_GT=np.int64(GT.shape[2]), AD=AD.astype(np.int32), DP=DP.astype(np.int32),
        psi0=np.array([s[0] for s in start]), theta0=np.array([s[1] for s in start]),
        next_rand=np.float64(next_rand), psi=np.array([np.asarray(m.psi, float) for m in models]),
        theta=np.array([np.asarray(m.theta, float) for m in models]),
        logLik=np.array([float(m.logLik) for m in models]),
        logLik_all_flat=np.concatenate([np.asarray(m.logLik_all, float) for m in models]),
        n_all=np.array([len(m.logLik_all) for m in models], dtype=np.int64), stop_margin=margins,
        LR=np.array(LR, float), pvalue=np.array(pv, float), log_pvalue=np.array(lpv, float))
    size = os.path.getsize(path)
    assert size < 618 * 1024, size
    print("c1_bulk_cohort %.1f KB" % (size / 1024))


if __name__ == "__main__":
    main()
