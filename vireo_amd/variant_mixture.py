"""Per-variant clone mixtures: is a variant's allele fraction across cells better described by K binomial
components than by one?

The step both clone notebooks of the reference open with -- "call clonal informed mtDNA variants" -- stated in
the reference's own formulas: ``BinomMixtureVB._fit_BV`` (vireoSNP/utils/bmm_model.py:178-201) fitted to each
variant ALONE, the 1 x n_cell problem made of its row, once with ``n_clone`` components and once with one, and
the two evidence lower bounds compared.  It is the "M1 multiple donors vs M0 single donor" of
``variant_ELBO_gain`` (variant_select.py:66-106) with the assignment learned per variant instead of given, so
it needs no fit beforehand.  Every variant's whole loop runs on the GPU in one launch (vrx_varmix_fit).

Per variant, over its covered cells (``DP >= min_DP``): default priors (Beta(1, 1) on theta, uniform ID
prior), ``fix_beta_sum=False``, and the deterministic start

    ID_init[i, k] = w_k / sum_k w_k,   w_k = max(0, 1 - |AD_i / DP_i - k / (K - 1)| (K - 1)) + 1/64

in place of random draws; ``elbo`` is the reference's ``ELBO_iters[-1]`` (``ELBO[it - 1]``, what its
``ELBO_inits`` compare), ``elbo_one`` the closed form of the same bound with ``n_donor = 1``, and
``gain = elbo - elbo_one``.  The binomial coefficient is in neither bound.  ``gain > 0`` is the natural cut.

Out of scope: random restarts per variant, ``fix_beta_sum``, non-default priors, and MQuad's knee-point
cut-off and delta-BIC.  This is the reference's VB bound, not a re-implementation of MQuad: the numbers are
not MQuad's, only the purpose and the names of the output files of ``python -m vireo_amd.variant_gain`` are.
"""
import ctypes as C

import numpy as np

from . import _lib
from .counts import default_device, merge_counts

MIN_CLONE, MAX_CLONE = 2, 8


def covered_csr(AD, DP, min_DP=1):
    """-> (shape, rowptr int64[n_var + 1], cell int32[nnz], ad int32[nnz], dp int32[nnz]): the entries with
    DP >= max(min_DP, 1) by variant, in increasing cell index.  Accepts what ``merge_counts`` accepts; raises
    ValueError on negative or fractional counts and on AD > DP."""
    from scipy.sparse import issparse
    if not issparse(AD):
        AD = np.asarray(AD)
    if not issparse(DP):
        DP = np.asarray(DP)
    if AD.ndim != 2 or DP.ndim != 2:
        raise ValueError("AD and DP must be 2-D matrices")
    # the columns of the transposes are the variants: the merged CSC of (AD.T, DP.T) is the CSR asked for
    (n_cell, n_var), rowptr, cell, ad, dp = merge_counts(AD.T, DP.T)
    bad = np.flatnonzero(ad > dp)
    if bad.size:
        v = int(np.searchsorted(rowptr, bad[0], side="right") - 1)
        raise ValueError("AD > DP at variant %d, cell %d (%d > %d)" % (v, cell[bad[0]], ad[bad[0]], dp[bad[0]]))
    keep = dp >= max(int(min_DP), 1)
    if not keep.all():
        kept = np.concatenate(([0], np.cumsum(keep, dtype=np.int64)))
        rowptr, cell, ad, dp = kept[rowptr], cell[keep], ad[keep], dp[keep]
    return (n_var, n_cell), np.ascontiguousarray(rowptr, dtype=np.int64), np.ascontiguousarray(cell), \
        np.ascontiguousarray(ad), np.ascontiguousarray(dp)


def _check_fit_args(n_clone, max_iter, min_iter):
    if not MIN_CLONE <= int(n_clone) <= MAX_CLONE:
        raise ValueError("n_clone = %s: %d ... %d components are built" % (n_clone, MIN_CLONE, MAX_CLONE))
    if int(max_iter) < 2:
        raise ValueError("max_iter = %s: the bound returned is ELBO[it - 1], which needs max_iter >= 2" % max_iter)
    if int(min_iter) < 0:
        raise ValueError("min_iter must not be negative")


class VariantMixtures(_lib.Handle):
    """The covered (AD, DP) entries of every variant resident on one GPU (C handle ``vrx_varmix``);
    ``fit`` may be called any number of times, so sweeping ``n_clone`` reuses one upload."""

    def __init__(self, AD, DP, min_DP=1, device=None):
        (self.n_var, self.n_cell), rowptr, _cell, ad, dp = covered_csr(AD, DP, min_DP)
        self.n_covered = np.diff(rowptr)
        self.nnz = int(ad.size)
        _lib.require_gpu()
        self.device = default_device() if device is None else device
        i32 = C.POINTER(C.c_int32)
        L = _lib.lib()
        super().__init__("VariantMixtures", lambda out: L.vrx_varmix_create(
            self.device, self.n_var, self.nnz, rowptr.ctypes.data_as(C.POINTER(C.c_int64)),
            ad.ctypes.data_as(i32), dp.ctypes.data_as(i32), out), L.vrx_varmix_destroy)
        self.kernel_ms = 0.0

    def fit(self, n_clone=2, max_iter=200, min_iter=20, epsilon_conv=1e-2, return_trace=False):
        """-> dict(gain, elbo, elbo_one, beta_mu, beta_sum, size, n_iter, warn, n_covered [, trace]).
        ``size`` counts covered cells only (the reference's ``ID_prob.sum(0)`` exceeds it by the uncovered
        cells / n_clone); ``warn`` bit 0: the bound decreased by more than 1e-6, bit 1: not converged;
        ``trace``: a list of ELBO[0 .. n_iter] per variant."""
        _check_fit_args(n_clone, max_iter, min_iter)
        N, K = self.n_var, int(n_clone)
        elbo, one = np.zeros(N), np.zeros(N)
        mu, sm, size = np.zeros((N, K)), np.zeros((N, K)), np.zeros((N, K))
        n_iter, warn = np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int32)
        trace = np.zeros((N, int(max_iter))) if return_trace else None
        ms = C.c_double(0.0)
        i32 = C.POINTER(C.c_int32)
        _lib.check(_lib.lib().vrx_varmix_fit(
            self._h, K, int(max_iter), int(min_iter), float(epsilon_conv), _lib.dptr(elbo), _lib.dptr(one),
            _lib.dptr(mu), _lib.dptr(sm), _lib.dptr(size), n_iter.ctypes.data_as(i32), warn.ctypes.data_as(i32),
            _lib.dptr(trace), C.byref(ms)))
        self.kernel_ms = ms.value
        out = dict(gain=elbo - one, elbo=elbo, elbo_one=one, beta_mu=mu, beta_sum=sm, size=size, n_iter=n_iter,
                   warn=warn, n_covered=self.n_covered.copy())
        if return_trace:
            out["trace"] = [trace[v, :n_iter[v] + 1].copy() for v in range(N)]
        return out


def variant_mixture_gain(AD, DP, n_clone=2, max_iter=200, min_iter=20, epsilon_conv=1e-2, min_DP=1,
                         return_fit=False, device=None):
    """``gain`` (n_var,): the evidence lower bound of an ``n_clone``-component binomial mixture fitted to each
    variant alone, minus that of one component (see the module text; > 0 favours the mixture).  AD, DP:
    variants x cells, sparse of any format or dense, integer or float dtype.  ``return_fit=True`` returns the
    dict of ``VariantMixtures.fit`` instead."""
    _check_fit_args(n_clone, max_iter, min_iter)
    vm = VariantMixtures(AD, DP, min_DP=min_DP, device=device)
    try:
        fit = vm.fit(n_clone=n_clone, max_iter=max_iter, min_iter=min_iter, epsilon_conv=epsilon_conv)
    finally:
        vm.close()
    return fit if return_fit else fit["gain"]
