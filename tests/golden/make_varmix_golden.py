"""Per-variant mixture fixture from the REAL reference (build container only, /root/reference):

    python tests/golden/make_varmix_golden.py

  c1_varmix.npz   40 generated rows (tests/varmix_np.gen_rows, 300 cells) and what
                  BinomMixtureVB(n_cell, 1, K, ID_prob_init=id_init(row))._fit_BV(row) leaves behind for
                  K = 2, 3, 5 -- ELBO_iters (= ELBO[:it], zero padded), it, beta_mu, beta_sum, ID_prob.sum(0)
                  -- and ELBO_iters[-1] of the same call with n_donor = 1.

Pure data: the counts and the arrays the reference returns.  Follows make_ambient_golden.py."""
import os
import sys

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import vireoSNP                                                   # noqa: E402
from vireoSNP import BinomMixtureVB                               # noqa: E402
from tests import varmix_np as VN                                 # noqa: E402

KS = (2, 3, 5)
MAX_ITER, MIN_ITER, EPS = 60, 2, 1e-2
LENGTHS = [300, 257, 129, 128, 65, 64, 63, 40, 17, 9, 5, 2, 1, 0, 211, 150, 100, 77, 33, 300,
           290, 180, 128, 90, 64, 45, 30, 12, 3, 250, 199, 140, 111, 70, 50, 25, 8, 300, 160, 20]


def main():
    assert vireoSNP.__version__ == "0.5.9", vireoSNP.__version__
    AD, DP = VN.gen_rows(LENGTHS, seed=2024, n_cell=VN.N_CELL)
    n_var, n_cell = AD.shape
    out = dict(AD=AD.astype(np.int32), DP=DP.astype(np.int32), Ks=np.array(KS), max_iter=np.int64(MAX_ITER),
               min_iter=np.int64(MIN_ITER), epsilon_conv=np.float64(EPS))
    kw = dict(max_iter=MAX_ITER, min_iter=MIN_ITER, epsilon_conv=EPS, verbose=False)
    one = np.zeros(n_var)
    for v in range(n_var):
        a, d = AD[v:v + 1].astype(np.float64), DP[v:v + 1].astype(np.float64)
        m = BinomMixtureVB(n_cell=n_cell, n_var=1, n_donor=1)
        m._fit_BV(a, d, **kw)
        assert np.all(m.ELBO_iters == m.ELBO_iters[0])
        one[v] = m.ELBO_iters[-1]
    out["elbo_one"] = one
    for K in KS:
        trace = np.zeros((n_var, MAX_ITER))
        n_iter = np.zeros(n_var, dtype=np.int32)
        mu, sm, size = np.zeros((n_var, K)), np.zeros((n_var, K)), np.zeros((n_var, K))
        for v in range(n_var):
            a, d = AD[v:v + 1].astype(np.float64), DP[v:v + 1].astype(np.float64)
            m = BinomMixtureVB(n_cell=n_cell, n_var=1, n_donor=K, ID_prob_init=VN.id_init(AD[v], DP[v], K))
            m._fit_BV(a, d, **kw)
            n_iter[v] = len(m.ELBO_iters)
            trace[v, :n_iter[v]] = m.ELBO_iters
            mu[v], sm[v], size[v] = m.beta_mu[0], m.beta_sum[0], m.ID_prob.sum(0)
        out.update({"trace_K%d" % K: trace, "n_iter_K%d" % K: n_iter, "elbo_K%d" % K: trace[np.arange(n_var), n_iter - 1],
                    "beta_mu_K%d" % K: mu, "beta_sum_K%d" % K: sm, "size_K%d" % K: size})
        print("K = %d: it %d .. %d" % (K, n_iter.min(), n_iter.max()))
    path = os.path.join(HERE, "c1_varmix.npz")
    np.savez_compressed(path, **out)
    print("c1_varmix %.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
