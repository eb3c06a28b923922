"""Host-side helpers with the reference's names (vireoSNP/utils/vireo_base.py).

Only what the host needs to prepare the initial state and priors lives here; the
per-iteration normalisation / amplification / Beta-KL arithmetic of the reference runs
inside the HIP kernels (vireo_amd/csrc/vrx_kernels.h).
"""
import ctypes as C

import numpy as np

from . import _lib
from .counts import default_device, device_counts


def normalize(X, axis=-1):
    """X / X.sum(axis) (vireo_base.py:44-55).  Host NumPy: used on the freshly drawn
    random initial state, whose RNG order must match the reference's legacy stream."""
    return X / np.sum(X, axis=axis, keepdims=True)


def tensor_normalize(X, axis=1):
    """vireo_base.py:58-59."""
    return normalize(X, axis)


def loglik_amplify(X, axis=-1):
    """X - X.max(axis) (vireo_base.py:62-74)."""
    return X - np.max(X, axis=axis, keepdims=True)


def get_binom_coeff(AD, DP, max_val=700, is_log=True):
    """float32 log C(DP, AD) of every entry with DP > 0, clamped at max_val -- the per-entry
    helper the reference exports (vireo_base.py:7-22; ``is_log`` is ignored there too).  Host
    NumPy/SciPy: the fits never call it, they add the GPU-reduced sum (``binom_coeff_sum``).
    Entry order follows the reference's boolean indexing ``X[DP > 0]``: row-major (variant by
    variant) for every input format; sparse input gives a (1, n) array like the reference's
    np.matrix, dense input a 1-D array."""
    from scipy.sparse import issparse
    from scipy.special import binom
    from .counts import merge_counts
    if issparse(DP):
        _, _, _, ad, dp = merge_counts(AD.T, DP.T)      # columns of the transpose = rows
        keep = dp > 0
        ad, dp = ad[keep].astype(np.int64), dp[keep].astype(np.int64)
    else:
        keep = np.asarray(DP) > 0
        ad, dp = np.asarray(AD)[keep].astype(np.int64), np.asarray(DP)[keep].astype(np.int64)
    coeff = np.minimum(np.log(binom(dp, ad)), max_val).astype(np.float32)
    return coeff[None, :] if issparse(DP) else coeff


def beta_entropy(X, X_prior=None, axis=None):
    """Entropy of Beta(X[:, 0], X[:, 1]) distributions, or with X_prior their KL divergence
    from Beta(X_prior[:, 0], X_prior[:, 1]), summed over ``axis`` (vireo_base.py:77-127).  Host
    helper with the reference's name; inside the fits the same arithmetic is ``vrx_beta_kl``
    (vireo_amd/csrc/vrx_kernels.h)."""
    from scipy.special import betaln, digamma

    def cross(p, q):        # -E_p[log q]
        return (betaln(q[:, 0], q[:, 1]) - (q[:, 0] - 1) * digamma(p[:, 0])
                - (q[:, 1] - 1) * digamma(p[:, 1]) + (q.sum(axis=1) - 2) * digamma(p.sum(axis=1)))

    X = np.asarray(X)
    if X.ndim == 1:
        if X.shape[0] != 2:
            print("Error: unsupported shape. Make sure it's (N, 2)")
        X = X.reshape(-1, 2)
    if X_prior is None:
        return np.sum(cross(X, X), axis=axis)
    return np.sum(cross(X, np.asarray(X_prior)) - cross(X, X), axis=axis)


def binom_coeff_sum(AD, DP):
    """np.sum(get_binom_coeff(AD, DP)) of the reference (vireo_base.py:7-22 summed at
    vireo_model.py:313 / bmm_model.py:239): a float32 scalar, computed on the GPU."""
    return device_counts(AD, DP).binom_const()


# ---- small host-side K x K logic around the fits (not on the GPU path) -----------------
def match(ref_ids, new_ids, uniq_ref_only=True):
    """Index of each ref_id in new_ids (None when absent); ref_ids may repeat
    (vireo_base.py:130-184).  A sort-merge like the reference, so ties and the
    ``uniq_ref_only`` switch behave identically."""
    order_ref = np.argsort(ref_ids)
    order_new = np.argsort(new_ids)
    found = [None] * len(order_ref)
    j = 0
    for i in order_ref:
        while j < len(order_new) and new_ids[order_new[j]] < ref_ids[i]:
            j += 1
        if j < len(order_new) and new_ids[order_new[j]] == ref_ids[i]:
            found[i] = order_new[j]
            if uniq_ref_only:
                j += 1
    return np.array(found)


def optimal_match(X, Z, axis=1, return_delta=False):
    """Hungarian alignment of the slices of Z to those of X along ``axis`` by mean absolute
    difference (vireo_base.py:187-206)."""
    from scipy.optimize import linear_sum_assignment
    nx, nz = X.shape[axis], Z.shape[axis]
    delta = np.zeros((nx, nz))
    for i in range(nx):
        xi = np.take(X, i, axis=axis)
        for j in range(nz):
            delta[i, j] = np.mean(np.abs(xi - np.take(Z, j, axis=axis)))
    idx0, idx1 = linear_sum_assignment(delta)
    return (idx0, idx1, delta) if return_delta else (idx0, idx1)


MAX_GT_MATCH = 64      # genotype classes per donor that genotype_distance accepts


def _canonical_genotypes(A, axis, name):
    """(n_var, K, n_gt) float64 C-contiguous view of a 2-D or 3-D array whose donors lie along ``axis``
    (no copy when it already is one); ValueError otherwise"""
    A = np.asarray(A)
    if A.dtype.kind not in "iufb":
        raise ValueError("%s has unsupported dtype %s" % (name, A.dtype))
    if A.ndim not in (2, 3):
        raise ValueError("%s must be 2-D or 3-D, got shape %s" % (name, A.shape))
    if not -A.ndim <= axis < A.ndim:
        raise ValueError("axis %d is out of range for %s of shape %s" % (axis, name, A.shape))
    A = np.moveaxis(A, axis, 1)
    if A.ndim == 2:
        A = A[:, :, None]
    return np.ascontiguousarray(A, dtype=np.float64)


def genotype_distance(X, Z=None, axis=1, block_vars=None):
    """(K1, K2) matrix of the mean absolute difference between every slice of X and every slice of Z along
    ``axis`` -- the ``diff_mat`` that optimal_match fills pair by pair (vireo_base.py:197-201) -- in one
    streaming pass on the GPU (``vrx_geno_dist``).  ``Z=None`` compares X with itself (the matrix of
    donor_select, :230-234).  X and Z are 2-D or 3-D and agree on every axis but ``axis``; float64
    C-contiguous (n_var, K, n_gt) inputs are used as they are, anything else is moved and copied once on
    the host.  ``block_vars``: variants per upload slab (default: 256 MiB per operand).  No variants at
    all: all NaN, like np.mean of an empty array.  There is no CPU fallback."""
    Xc = _canonical_genotypes(X, axis, "X")
    Zc = None if Z is None else _canonical_genotypes(Z, axis, "Z")
    n_var, k1, n_gt = Xc.shape
    k2 = k1
    if Zc is not None:
        if Zc.shape[0] != n_var or Zc.shape[2] != n_gt:
            raise ValueError("X %s and Z %s differ off axis %d" % (np.shape(X), np.shape(Z), axis))
        k2 = Zc.shape[1]
    if k1 < 1 or k2 < 1 or n_gt < 1:
        raise ValueError("X %s and Z %s need at least one slice along axis %d and one genotype"
                         % (np.shape(X), np.shape(Z) if Z is not None else None, axis))
    if n_gt > MAX_GT_MATCH:
        raise ValueError("%d genotype classes per donor (at most %d)" % (n_gt, MAX_GT_MATCH))
    block_vars = 0 if block_vars is None else int(block_vars)
    if block_vars < 0:
        raise ValueError("block_vars must be positive (or None / 0 for the default)")
    if n_var == 0:
        return np.full((k1, k2), np.nan)
    return _geno_dist(Xc, Zc, block_vars)[0]


def _geno_dist(Xc, Zc, block_vars=0):
    """-> (D, kernel ms) of canonical operands (n_var, K, n_gt), float64 C-contiguous; Zc None: Xc itself"""
    _lib.require_gpu()
    n_var, k1, n_gt = Xc.shape
    k2 = k1 if Zc is None else Zc.shape[1]
    D = np.empty((k1, k2))
    ms = C.c_double(0.0)
    _lib.check(_lib.lib().vrx_geno_dist(default_device(), n_var, k1, k2, n_gt, _lib.dptr(Xc), _lib.dptr(Zc),
                                        block_vars, _lib.dptr(D), C.byref(ms)))
    return D, ms.value


def donor_match(X, Z, axis=1, return_delta=False):
    """optimal_match with the distance matrix from the GPU: Hungarian alignment of the slices of Z to those
    of X along ``axis`` by ``genotype_distance``; the same return values as optimal_match."""
    from scipy.optimize import linear_sum_assignment
    delta = genotype_distance(X, Z, axis=axis)
    idx0, idx1 = linear_sum_assignment(delta)
    return (idx0, idx1, delta) if return_delta else (idx0, idx1)


def donor_select(GT_prob, ID_prob, n_donor, mode="distance"):
    """Keep n_donor of the donors found with extra donors: by size, or greedily the most
    mutually distant genotypes starting from the largest (vireo_base.py:217-254)."""
    size = np.sum(ID_prob, axis=0)
    K = GT_prob.shape[1]
    if mode == "size":
        keep = np.argsort(size)[::-1]
    else:
        dist = np.zeros((K, K))
        for i in range(K):
            for j in range(K):
                dist[i, j] = np.mean(np.abs(GT_prob[:, i, :] - GT_prob[:, j, :]))
        keep = [np.argmax(size)]
        left = np.delete(np.arange(K), keep)
        dist = np.delete(dist, keep, axis=1)
        while len(keep) < dist.shape[0]:
            nxt = np.argmax(np.min(dist[keep, :], axis=0))
            keep.append(left[nxt])
            left = np.delete(left, nxt)
            dist = np.delete(dist, nxt, axis=1)
    print("[vireo] donor size with searching extra %d donors:" % (K - n_donor))
    print("\t".join(["donor%d" % x for x in keep]))
    print("\t".join(["%.0f" % size[x] for x in keep]))
    out = ID_prob[:, keep[:n_donor]]
    out[out < 10**-10] = 10**-10
    return out
