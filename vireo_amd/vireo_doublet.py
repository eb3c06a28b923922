"""Doublet prediction and ambient-RNA estimation with a fitted Vireo model, drop-in for
vireoSNP/utils/vireo_doublet.py:11-273 (``predict_doublet``, its two table builders and
``predit_ambient``).

The K + K(K-1)/2 column cell log-likelihood -- 3*6 transposed sparse products in the
reference (:53-62) -- is one cell pass on the GPU (``vrx_problem_doublet``); the genotype
table of the donor pairs (653 MB at N=100k, K=16 in the reference) is formed on the fly in
the kernel for every n_GT a model can have, and the T + T(T-1)/2 class thetas are host-side
arithmetic on T numbers.  ``add_doublet_GT`` is kept as a public helper; nothing here calls it.

``predit_ambient`` (the reference's spelling) fits one small EM per cell; here every cell is fitted
in one launch (``vrx_problem_ambient``, vireo_amd/csrc/vrx_ambient.h).
"""
import ctypes as C
import itertools
import timeit

import numpy as np
from scipy.special import digamma

from . import _lib
from ._lib import dptr, f64
from .counts import device_counts
from .variant_select import variant_ELBO_gain
from .vireo_base import normalize

LAST_AMBIENT = {}    # the split of the last predit_ambient call (read by tests/perf/ambient_bench.py)


def add_doublet_theta(beta_mu, beta_sum):
    """theta of the mixed genotypes 0&1, 0&2, 1&2: mean of the means, geometric mean of
    the concentrations (vireo_doublet.py:85-102)."""
    pairs = np.array(list(itertools.combinations(range(beta_mu.shape[1]), 2)))
    a, b = pairs[:, 0], pairs[:, 1]
    mu_db = (beta_mu[:, a] + beta_mu[:, b]) / 2.0
    sum_db = np.sqrt(beta_sum[:, a] * beta_sum[:, b])
    return np.append(beta_mu, mu_db, axis=-1), np.append(beta_sum, sum_db, axis=-1)


def add_doublet_GT(GT_prob):
    """Genotype table of all donor pairs over T + T(T-1)/2 classes, appended to the singlet
    table padded with zero mixed classes (vireo_doublet.py:105-136)."""
    n_gt = GT_prob.shape[2]
    gt_pairs = np.array(list(itertools.combinations(range(n_gt), 2)))
    dn_pairs = np.array(list(itertools.combinations(range(GT_prob.shape[1]), 2)))
    g1, g2 = gt_pairs[:, 0], gt_pairs[:, 1]
    P = GT_prob[:, dn_pairs[:, 0], :]
    Q = GT_prob[:, dn_pairs[:, 1], :]
    both = np.zeros((GT_prob.shape[0], dn_pairs.shape[0], n_gt + gt_pairs.shape[0]))
    both[:, :, :n_gt] = P * Q
    both[:, :, n_gt:] = P[:, :, g1] * Q[:, :, g2] + P[:, :, g2] * Q[:, :, g1]
    both = normalize(both, axis=2)
    single = np.append(
        GT_prob, np.zeros((GT_prob.shape[0], GT_prob.shape[1], gt_pairs.shape[0])), axis=2)
    return np.append(single, both, axis=1)


def predict_doublet(vobj, AD, DP, update_GT=True, update_ID=True,
                    doublet_rate_prior=None):
    """-> (doublet_prob (n_cell, K(K-1)/2), singlet ID_prob (n_cell, K), logLik_ratio)
    exactly as vireo_doublet.py:11-82, including its side effects on ``vobj``
    (ID_prob <- un-renormalised singlet block, then update_GT_prob)."""
    counts = device_counts(AD, DP)
    K, T = vobj.GT_prob.shape[1], vobj.GT_prob.shape[2]
    if K < 2:
        raise ValueError("predict_doublet needs n_donor >= 2 (a doublet is a pair of donors), got %d" % K)
    n_pair = K * (K - 1) // 2
    C_ = K + n_pair
    beta_mu_both, beta_sum_both = add_doublet_theta(vobj.beta_mu, vobj.beta_sum)
    if doublet_rate_prior is None:
        doublet_rate_prior = min(0.5, counts.n_cell / 100000)
    ID_prior_both = np.append(
        vobj.ID_prior * (1 - doublet_rate_prior),
        np.ones((vobj.n_cell, n_pair)) / n_pair * doublet_rate_prior, axis=1)

    # T + T(T-1)/2 digamma values per theta row: O(T') host work (vireo_doublet.py:55-57)
    psi1 = f64(digamma(beta_sum_both * beta_mu_both))
    psi2 = f64(digamma(beta_sum_both * (1 - beta_mu_both)))
    psis = f64(digamma(beta_sum_both))
    logLik_ID = np.empty((counts.n_cell, C_))
    ID_prob_both = np.empty((counts.n_cell, C_))
    prior = f64(ID_prior_both)
    # the pair genotype table (add_doublet_GT) is formed inside the kernel, never in memory
    GT = f64(vobj.GT_prob)
    _lib.check(_lib.lib().vrx_problem_doublet(
        counts.handle, K, T, dptr(GT), dptr(psi1), dptr(psi2), dptr(psis), psi1.shape[0],
        dptr(prior), prior.shape[0], dptr(logLik_ID), dptr(ID_prob_both)))

    logLik_ratio = (logLik_ID[:, vobj.n_donor:].max(1) -
                    logLik_ID[:, :vobj.n_donor].max(1))
    if update_ID:
        vobj.ID_prob = ID_prob_both[:, :vobj.n_donor]
    if update_GT:
        if update_ID:
            vobj.update_GT_prob(counts, None)
        else:
            print("For update_GT, please turn on update_ID.")
    return (ID_prob_both[:, vobj.n_donor:], ID_prob_both[:, :vobj.n_donor], logLik_ratio)


def predit_ambient(vobj, AD, DP, nproc=10, min_ELBO_gain=None):
    """-> (Psi_mat (n_cell, K), Psi_var (n_cell, K), Psi_logLik_ratio (n_cell,)): the fraction of
    each donor's RNA in every cell, its Cramer-Rao variance and the log-likelihood ratio against
    the cell's main donor alone (vireo_doublet.py:213-273).  Variants are selected by
    ``variant_ELBO_gain >= min_ELBO_gain`` (default sqrt(n_cell) / 3); each cell's EM starts
    from ``np.random.dirichlet`` draws of the global stream, cell after cell -- the reference's
    ``nproc=1`` sequence.  ``nproc`` is accepted and ignored."""
    start = timeit.default_timer()
    counts = device_counts(AD, DP)
    n_cell, K = counts.n_cell, vobj.GT_prob.shape[1]
    theta_mat = f64(np.tensordot(vobj.GT_prob, vobj.beta_mu[0, :], axes=(2, 0)))
    if min_ELBO_gain is None:
        min_ELBO_gain = np.sqrt(n_cell) / 3.0
    t0 = timeit.default_timer()
    gain = variant_ELBO_gain(vobj.ID_prob, counts, None)
    sel = gain >= min_ELBO_gain
    print("[vireo] %d out %d SNPs selected for ambient RNA detection: "
          "ELBO_gain > %.1f" % (sum(sel), len(sel), min_ELBO_gain))
    t1 = timeit.default_timer()
    psi0 = f64(np.random.dirichlet([1] * K, size=n_cell))
    t2 = timeit.default_timer()
    psi, var = np.empty((n_cell, K)), np.empty((n_cell, K))
    llr, n_iter, ms = np.empty(n_cell), np.empty(n_cell, np.int32), np.zeros(3)
    mask = np.ascontiguousarray(sel, dtype=np.uint8)
    _lib.check(_lib.lib().vrx_problem_ambient(
        counts.handle, K, dptr(theta_mat), mask.ctypes.data_as(C.POINTER(C.c_uint8)), dptr(psi0),
        20, 200, 1e-3, dptr(psi), dptr(var), dptr(llr), n_iter.ctypes.data_as(C.POINTER(C.c_int32)),
        dptr(ms)))
    stop = timeit.default_timer()
    LAST_AMBIENT.clear()
    LAST_AMBIENT.update(gain_s=t1 - t0, draws_s=t2 - t1, compaction_ms=ms[0], em_ms=ms[1],
                        download_ms=ms[2], call_s=stop - t2, total_s=stop - start,
                        n_selected=int(sel.sum()), n_iter=n_iter)
    print('[vireo] Ambient RNA time: %.1f sec' % (stop - start))
    return psi, var, llr
