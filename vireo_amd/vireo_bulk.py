"""Donor abundance in a multiplexed bulk sample (vireoSNP/utils/vireo_bulk.py): ``VireoBulk`` and
``LikRatio_test`` on the device.

The per-variant counts and the donors' genotype probabilities stay resident behind a ``BulkData``
handle (C handle ``vrx_bulk``); the EM loop, its log-likelihood trace and its stop rule run in
``vrx_bulk_fit`` (one pass over GT_prob per iteration plus one), the log-likelihoods of the ratio test
in ``vrx_bulk_loglik`` (alternative and null in one pass).  As with ``DeviceCounts``, a handle may be
passed in place of ``AD`` (with ``DP=None, GT_prob=None``) so that a fit and its tests share one
upload.  There is no CPU fallback.
"""
import ctypes as C
import weakref

import numpy as np

from . import _lib
from .counts import default_device

__all__ = ["VireoBulk", "LikRatio_test", "BulkData", "device_bulk"]


def _counts(x, name):
    a = np.asarray(x)
    if a.dtype.kind not in "iufb":
        raise ValueError("%s has unsupported dtype %s" % (name, a.dtype))
    if a.ndim != 1:
        raise ValueError("%s must be a vector of per-variant counts, got shape %s" % (name, a.shape))
    return np.ascontiguousarray(a, dtype=np.float64)


def _check_inputs(AD, DP, GT_prob=None):
    """float64 C-order copies (or views) of the reference's operands; ValueError on a bad shape or dtype"""
    AD, DP = _counts(AD, "AD"), _counts(DP, "DP")
    if AD.shape != DP.shape:
        raise ValueError("AD %s and DP %s differ in shape" % (AD.shape, DP.shape))
    if AD.size < 1:
        raise ValueError("AD and DP are empty")
    if GT_prob is None:
        return AD, DP, None
    GT = np.asarray(GT_prob)
    if GT.dtype.kind not in "iufb":
        raise ValueError("GT_prob has unsupported dtype %s" % GT.dtype)
    if GT.ndim != 3:
        raise ValueError("GT_prob must be (n_variant, n_donor, n_GT), got shape %s" % (GT.shape,))
    if GT.shape[0] != AD.size:
        raise ValueError("GT_prob has %d variants, AD and DP %d" % (GT.shape[0], AD.size))
    if GT.shape[1] < 1 or GT.shape[2] < 2:
        raise ValueError("GT_prob needs n_donor >= 1 and n_GT >= 2, got shape %s" % (GT.shape,))
    return AD, DP, np.ascontiguousarray(GT, dtype=np.float64)


def _vector(x, n, name):
    a = np.asarray(x)
    if a.dtype.kind not in "iufb":
        raise ValueError("%s has unsupported dtype %s" % (name, a.dtype))
    if a.shape != (n,):
        raise ValueError("%s must have shape (%d,), got %s" % (name, n, a.shape))
    return np.array(a, dtype=np.float64)        # (a copy: the library writes the fit into it)


class BulkData:
    """(AD, DP, GT_prob) of a bulk sample on one GPU (C handle ``vrx_bulk``)."""

    def __init__(self, AD, DP, GT_prob, device=None):
        AD, DP, GT = _check_inputs(AD, DP, GT_prob)
        if GT is None:
            raise ValueError("GT_prob is required")
        _lib.require_gpu()
        if device is None:
            device = default_device()
        self.n_var, self.n_donor, self.n_GT = (int(x) for x in GT.shape)
        self.device = device
        self._h = C.c_void_p()
        _lib.check(_lib.lib().vrx_bulk_create(device, self.n_var, self.n_donor, self.n_GT, _lib.dptr(GT),
                                              _lib.dptr(AD), _lib.dptr(DP), C.byref(self._h)))
        self._fin = weakref.finalize(self, _lib.lib().vrx_bulk_destroy, self._h)

    @property
    def handle(self):
        return self._h

    def set_counts(self, AD, DP):
        """another sample on the same genotypes: GT_prob stays on the device"""
        AD, DP, _ = _check_inputs(AD, DP)
        if AD.size != self.n_var:
            raise ValueError("AD and DP have %d variants, the handle %d" % (AD.size, self.n_var))
        _lib.check(_lib.lib().vrx_bulk_set_counts(self._h, _lib.dptr(AD), _lib.dptr(DP)))

    def fit(self, psi, theta, max_iter=200, min_iter=5, epsilon_conv=1e-3, learn_theta=True,
            delay_fit_theta=0):
        """-> (psi, theta, logLik[0 .. it], it, device ms): the EM loop of VireoBulk.fit from (psi, theta)"""
        psi = _vector(psi, self.n_donor, "psi")
        theta = _vector(theta, self.n_GT, "theta")
        max_iter = int(max_iter)
        if max_iter < 1:
            raise ValueError("max_iter must be >= 1")
        trace = np.zeros(max_iter)
        it = C.c_int32(0)
        ms = C.c_double(0.0)
        _lib.check(_lib.lib().vrx_bulk_fit(self._h, _lib.dptr(psi), _lib.dptr(theta), max_iter, int(min_iter),
                                           float(epsilon_conv), int(bool(learn_theta)), int(delay_fit_theta),
                                           _lib.dptr(trace), C.byref(it), C.byref(ms)))
        return psi, theta, trace[:it.value + 1], it.value, ms.value

    def loglik(self, psi, theta):
        """log-likelihood of every row of psi (n_psi x n_donor, or one vector) under theta"""
        P = np.asarray(psi)
        if P.dtype.kind not in "iufb":
            raise ValueError("psi has unsupported dtype %s" % P.dtype)
        one = P.ndim == 1
        P = np.ascontiguousarray(np.atleast_2d(P), dtype=np.float64)
        if P.ndim != 2 or P.shape[1] != self.n_donor or P.shape[0] < 1:
            raise ValueError("psi must be (n_psi, %d), got %s" % (self.n_donor, np.shape(psi)))
        theta = _vector(theta, self.n_GT, "theta")
        out = np.empty(P.shape[0])
        _lib.check(_lib.lib().vrx_bulk_loglik(self._h, P.shape[0], _lib.dptr(P), _lib.dptr(theta),
                                              _lib.dptr(out)))
        return out[0] if one else out

    def close(self):
        self._fin()


def device_bulk(AD, DP=None, GT_prob=None, device=None):
    """A ``BulkData`` (returned as is) or the reference's three operands, uploaded."""
    if isinstance(AD, BulkData):
        if DP is not None or GT_prob is not None:
            raise ValueError("with a BulkData handle in place of AD, DP and GT_prob must be None")
        return AD
    if DP is None or GT_prob is None:
        raise ValueError("AD, DP and GT_prob are all required (or a BulkData handle in place of AD)")
    return BulkData(AD, DP, GT_prob, device=device)


def _draw_start(n_donor, n_GT, redraw_psi):
    """The reference's draws from the legacy global stream, in its order (vireo_bulk.py:29-36): a flat
    Dirichlet for psi, n_GT uniforms for theta, and -- when the caller handed in a psi_init of the right
    length -- a second flat Dirichlet that replaces the first."""
    flat = [1] * n_donor
    psi = np.random.dirichlet(flat)
    theta = np.random.rand(n_GT)
    if redraw_psi:
        psi = np.random.dirichlet(flat)
    return psi, theta


class VireoBulk:
    """Donor shares of a pooled bulk sample (the reference's class of this name, vireo_bulk.py:8-117).

    psi (n_donor,): share of the sample's reads that each donor contributes; theta (n_GT,): probability of
    reading the alternative allele under each genotype.  Both are attributes, set here and updated by
    ``fit``; assign them to start from chosen values.

    ``psi_init`` only decides whether psi is drawn a second time: as in the reference its VALUES are not
    used.  ``theta_init`` of length n_GT is kept as given.  A wrong length prints the
    reference's warning and keeps the random draw.
    """

    def __init__(self, n_donor, n_GT=3, psi_init=None, theta_init=[0.01, 0.5, 0.99]):
        self.n_donor, self.n_GT = n_donor, n_GT
        psi_fits = psi_init is not None and len(psi_init) == n_donor
        theta_fits = theta_init is not None and len(theta_init) == n_GT
        self.psi, self.theta = _draw_start(n_donor, n_GT, redraw_psi=psi_fits)
        if psi_init is not None and not psi_fits:
            print("Warning: n_donor != len(psi_init)")
        if theta_fits:
            self.theta = theta_init
        elif theta_init is not None:
            print("Warning: n_GT != len(theta_init)")

    def fit(self, AD, DP=None, GT_prob=None, max_iter=200, min_iter=5, epsilon_conv=1e-3,
            learn_theta=True, delay_fit_theta=0, model="EM", verbose=False):
        """The EM of vireo_bulk.py:44-108 on the device, from the current psi and theta.

        AD, DP: (n_variant,) alternative-allele and total counts; GT_prob: (n_variant, n_donor, n_GT); or a
        ``BulkData`` in place of AD.  ``model`` is accepted for compatibility (there is only the EM).
        Leaves psi, theta, logLik (the last value of the trace) and logLik_all (the trace WITHOUT that
        last value, as the reference's ``logLik[:it]``)."""
        if not isinstance(AD, BulkData):
            if DP is None or GT_prob is None:
                raise ValueError("AD, DP and GT_prob are all required (or a BulkData handle in place of AD)")
            AD, DP, GT_prob = _check_inputs(AD, DP, GT_prob)
            shape = GT_prob.shape[1:]
        else:
            shape = (AD.n_donor, AD.n_GT)
        if shape != (self.n_donor, self.n_GT):
            raise ValueError("GT_prob is for %d donors x %d genotypes, the model for %d x %d"
                             % (shape + (self.n_donor, self.n_GT)))
        psi0 = _vector(self.psi, self.n_donor, "psi")
        theta0 = _vector(self.theta, self.n_GT, "theta")
        max_iter, min_iter = int(max_iter), int(min_iter)
        if max_iter < 1:
            raise ValueError("max_iter must be >= 1")
        data = device_bulk(AD, DP, GT_prob)
        psi, theta, trace, it, ms = data.fit(psi0, theta0, max_iter, min_iter, epsilon_conv, learn_theta,
                                             delay_fit_theta)
        if verbose:
            _replay_warnings(trace, it, min_iter, max_iter)
        self.psi = psi
        if learn_theta and it >= delay_fit_theta:     # (otherwise no update ran: theta stays as given)
            self.theta = theta
        self.logLik = trace[it]
        self.logLik_all = trace[:it]
        self.fit_ms_ = ms

    def LR_test(self, **kwargs):
        """``LikRatio_test`` with this model's psi as the alternative and its theta (vireo_bulk.py:110-117);
        keywords: psi_null, AD, DP, GT_prob (or a ``BulkData`` as AD), log."""
        return LikRatio_test(self.psi, theta=self.theta, **kwargs)


def _replay_warnings(trace, it, min_iter, max_iter):
    """The two messages of the reference's loop (vireo_bulk.py:97-103), one per iteration that earns one, from
    the trace the device kept.  Iteration 0 (reached with min_iter < 0) compares with ``logLik[-1]`` there:
    the array's last entry, still 0, or the value itself when max_iter is 1 -- vrx_bulk_finish does the same."""
    for i in range(max(min_iter + 1, 0), it + 1):
        before = trace[i - 1] if i >= 1 else (trace[0] if max_iter == 1 else 0.0)
        if trace[i] < before:
            print("Warning: logLikelihood decreases!\n")
        elif i == max_iter - 1:
            print("Warning: VB did not converge!\n")


def LikRatio_test(psi, psi_null, AD, DP=None, GT_prob=None, theta=None, log=False):
    """Chi-square test of the abundances ``psi`` against ``psi_null`` (vireo_bulk.py:120-167): twice the gap
    between their log-likelihoods under ``theta`` -- both from one pass on the device -- referred to a
    chi-square law with one degree of freedom per free component of the null.

    -> (statistic, upper-tail p-value), the p-value as its logarithm when ``log``."""
    from scipy.stats import chi2

    if theta is None:
        raise ValueError("theta is required")
    if not isinstance(AD, BulkData):
        if DP is None or GT_prob is None:
            raise ValueError("AD, DP and GT_prob are all required (or a BulkData handle in place of AD)")
        AD, DP, GT_prob = _check_inputs(AD, DP, GT_prob)
        K, G = GT_prob.shape[1:]
    else:
        K, G = AD.n_donor, AD.n_GT
    pair = np.stack([_vector(psi, K, "psi"), _vector(psi_null, K, "psi_null")])
    theta = _vector(theta, G, "theta")
    ll_alt, ll_null = device_bulk(AD, DP, GT_prob).loglik(pair, theta)
    statistic = 2 * (ll_alt - ll_null)
    tail = chi2.logsf if log else chi2.sf
    return statistic, tail(statistic, K - 1)
