"""Donor abundance in a multiplexed bulk sample (vireoSNP/utils/vireo_bulk.py): ``VireoBulk`` and
``LikRatio_test`` on the device.

The per-variant counts and the donors' genotype probabilities stay resident behind a ``BulkData``
handle (C handle ``vrx_bulk``); the EM loop, its log-likelihood trace and its stop rule run in
``vrx_bulk_fit`` (one pass over GT_prob per iteration plus one), the log-likelihoods of the ratio test
in ``vrx_bulk_loglik`` (alternative and null in one pass).  As with ``DeviceCounts``, a handle may be
passed in place of ``AD`` (with ``DP=None, GT_prob=None``) so that a fit and its tests share one
upload.  There is no CPU fallback.

``VireoBulkCohort`` fits many samples genotyped against the same donors at once: their counts stay
resident next to one ``GT_prob`` (``BulkData.set_cohort``), every pass reads a tile of ``GT_prob`` once
for a chunk of samples (``vrx_bulk_fit_cohort``) and the stop rule runs per sample on the device.
"""
import ctypes as C

import numpy as np

from . import _lib
from .counts import default_device

__all__ = ["VireoBulk", "VireoBulkCohort", "LikRatio_test", "BulkData", "device_bulk"]


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


def _check_cohort(AD, DP, n_var=None):
    """float64 C-order (n_sample, n_var) copies (or views) of a cohort's counts; ValueError otherwise"""
    out = []
    for x, name in ((AD, "AD"), (DP, "DP")):
        a = np.asarray(x)
        if a.dtype.kind not in "iufb":
            raise ValueError("%s has unsupported dtype %s" % (name, a.dtype))
        if a.ndim != 2:
            raise ValueError("%s must be (n_sample, n_variant) counts, got shape %s" % (name, a.shape))
        out.append(np.ascontiguousarray(a, dtype=np.float64))
    AD, DP = out
    if AD.shape != DP.shape:
        raise ValueError("AD %s and DP %s differ in shape" % (AD.shape, DP.shape))
    if AD.shape[0] < 1 or AD.shape[1] < 1:
        raise ValueError("AD and DP are empty")
    if n_var is not None and AD.shape[1] != n_var:
        raise ValueError("AD and DP have %d variants, GT_prob %d" % (AD.shape[1], n_var))
    return AD, DP


def _matrix(x, shape, name):
    a = np.asarray(x)
    if a.dtype.kind not in "iufb":
        raise ValueError("%s has unsupported dtype %s" % (name, a.dtype))
    if a.shape != shape:
        raise ValueError("%s must have shape %s, got %s" % (name, shape, a.shape))
    return np.array(a, dtype=np.float64)        # (a C-order copy: the library writes the fit into it)


def _vector(x, n, name):
    a = np.asarray(x)
    if a.dtype.kind not in "iufb":
        raise ValueError("%s has unsupported dtype %s" % (name, a.dtype))
    if a.shape != (n,):
        raise ValueError("%s must have shape (%d,), got %s" % (name, n, a.shape))
    return np.array(a, dtype=np.float64)        # (a copy: the library writes the fit into it)


class BulkData(_lib.Handle):
    """(AD, DP, GT_prob) of a bulk sample on one GPU (C handle ``vrx_bulk``)."""

    def __init__(self, AD, DP, GT_prob, device=None):
        AD, DP, GT = _check_inputs(AD, DP, GT_prob)
        if GT is None:
            raise ValueError("GT_prob is required")
        _lib.require_gpu()
        if device is None:
            device = default_device()
        self.n_var, self.n_donor, self.n_GT = (int(x) for x in GT.shape)
        self.n_sample = 0                           # (of the cohort: none yet)
        self.device = device
        L = _lib.lib()
        super().__init__("BulkData", lambda out: L.vrx_bulk_create(device, self.n_var, self.n_donor, self.n_GT,
                                                                   _lib.dptr(GT), _lib.dptr(AD), _lib.dptr(DP), out),
                         L.vrx_bulk_destroy)

    @property
    def handle(self):
        return self._h

    def info(self):
        """variants per tile and workgroups of the four passes, as the handle launches them: T, n_wg (fit),
        T_ll, n_wg_ll (log-likelihood), T_co, n_wg_co, T_co_ll, n_wg_co_ll (the cohort's)"""
        out = np.zeros(8, dtype=np.int32)
        _lib.check(_lib.lib().vrx_bulk_info(self._h, out.ctypes.data_as(C.POINTER(C.c_int32))))
        return dict(zip(("T", "n_wg", "T_ll", "n_wg_ll", "T_co", "n_wg_co", "T_co_ll", "n_wg_co_ll"),
                        (int(x) for x in out)))

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

    def set_cohort(self, AD, DP):
        """(n_sample, n_var) counts of a cohort on the same genotypes; replaces an earlier cohort and
        leaves the handle's single-sample counts alone"""
        AD, DP = _check_cohort(AD, DP, self.n_var)
        self.n_sample = 0
        _lib.check(_lib.lib().vrx_bulk_set_cohort(self._h, AD.shape[0], _lib.dptr(AD), _lib.dptr(DP)))
        self.n_sample = int(AD.shape[0])

    def _need_cohort(self):
        if self.n_sample < 1:
            raise ValueError("no cohort set on this handle (set_cohort)")

    def fit_cohort(self, psi, theta, max_iter=200, min_iter=5, epsilon_conv=1e-3, learn_theta=True,
                   delay_fit_theta=0):
        """-> (psi (S, K), theta (S, G), traces (S, max_iter), it (S,), device ms): the EM loop of
        VireoBulk.fit for every sample of the cohort, each from its row of (psi, theta).  Row s of
        traces holds logLik[0 .. it[s]] of that sample and zeros behind it."""
        self._need_cohort()
        psi = _matrix(psi, (self.n_sample, self.n_donor), "psi")
        theta = _matrix(theta, (self.n_sample, self.n_GT), "theta")
        max_iter = int(max_iter)
        if max_iter < 1:
            raise ValueError("max_iter must be >= 1")
        traces = np.zeros((self.n_sample, max_iter))
        it = np.zeros(self.n_sample, dtype=np.int32)
        ms = C.c_double(0.0)
        _lib.check(_lib.lib().vrx_bulk_fit_cohort(
            self._h, _lib.dptr(psi), _lib.dptr(theta), max_iter, int(min_iter), float(epsilon_conv),
            int(bool(learn_theta)), int(delay_fit_theta), _lib.dptr(traces),
            it.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(ms)))
        return psi, theta, traces, it.astype(np.int64), ms.value

    def loglik_cohort(self, psi, theta):
        """log-likelihoods of psi (S, K) -> (S,), or (S, Q, K) -> (S, Q), each sample under its row of
        theta (S, G) and its own counts"""
        self._need_cohort()
        P = np.asarray(psi)
        if P.dtype.kind not in "iufb":
            raise ValueError("psi has unsupported dtype %s" % P.dtype)
        one = P.ndim == 2
        if one:
            P = P[:, None, :]
        if P.ndim != 3 or P.shape[0] != self.n_sample or P.shape[2] != self.n_donor or P.shape[1] < 1:
            raise ValueError("psi must be (%d, %d) or (%d, n_psi, %d), got %s"
                             % (self.n_sample, self.n_donor, self.n_sample, self.n_donor, np.shape(psi)))
        P = np.ascontiguousarray(P, dtype=np.float64)
        theta = _matrix(theta, (self.n_sample, self.n_GT), "theta")
        out = np.empty(P.shape[:2])
        _lib.check(_lib.lib().vrx_bulk_loglik_cohort(self._h, P.shape[1], _lib.dptr(P), _lib.dptr(theta),
                                                     _lib.dptr(out)))
        return out[:, 0] if one else out


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


class VireoBulkCohort:
    """``n_sample`` bulk samples on one donor panel, fitted together: what a loop of ``VireoBulk`` over the
    samples computes, with one read of ``GT_prob`` per chunk of samples and pass instead of one per sample.

    The constructor draws sample by sample from the legacy global stream exactly as ``n_sample`` successive
    ``VireoBulk(n_donor, n_GT, psi_init, theta_init)`` would, so under one seed the cohort starts where that
    loop starts.  psi (n_sample, n_donor) and theta (n_sample, n_GT) are attributes; assign them to start
    from chosen values.  The reference's warnings about ``psi_init`` / ``theta_init`` are printed once."""

    def __init__(self, n_sample, n_donor, n_GT=3, psi_init=None, theta_init=[0.01, 0.5, 0.99]):
        n_sample = int(n_sample)
        if n_sample < 1:
            raise ValueError("n_sample must be >= 1")
        self.n_sample, self.n_donor, self.n_GT = n_sample, n_donor, n_GT
        psi_fits = psi_init is not None and len(psi_init) == n_donor
        theta_fits = theta_init is not None and len(theta_init) == n_GT
        draws = [_draw_start(n_donor, n_GT, redraw_psi=psi_fits) for _ in range(n_sample)]
        self.psi = np.array([d[0] for d in draws])
        self.theta = np.array([d[1] for d in draws])
        if psi_init is not None and not psi_fits:
            print("Warning: n_donor != len(psi_init)")
        if theta_fits:
            self.theta = np.tile(np.asarray(theta_init, dtype=np.float64), (n_sample, 1))
        elif theta_init is not None:
            print("Warning: n_GT != len(theta_init)")

    def _data(self, AD, DP, GT_prob):
        """the checks that need no device, then the handle with its cohort set"""
        if isinstance(AD, BulkData):
            if DP is not None or GT_prob is not None:
                raise ValueError("with a BulkData handle in place of AD, DP and GT_prob must be None")
            if AD.n_sample < 1:
                raise ValueError("the BulkData handle has no cohort set (set_cohort)")
            shape, n_sample = (AD.n_donor, AD.n_GT), AD.n_sample
        else:
            if DP is None or GT_prob is None:
                raise ValueError("AD, DP and GT_prob are all required (or a BulkData handle in place of AD)")
            AD, DP = _check_cohort(AD, DP)
            _, _, GT_prob = _check_inputs(AD[0], DP[0], GT_prob)
            shape, n_sample = GT_prob.shape[1:], AD.shape[0]
        if shape != (self.n_donor, self.n_GT):
            raise ValueError("GT_prob is for %d donors x %d genotypes, the model for %d x %d"
                             % (tuple(shape) + (self.n_donor, self.n_GT)))
        if n_sample != self.n_sample:
            raise ValueError("the counts hold %d samples, the model %d" % (n_sample, self.n_sample))
        return AD, DP, GT_prob

    @staticmethod
    def _upload(AD, DP, GT_prob):
        if isinstance(AD, BulkData):
            return AD
        data = BulkData(AD[0], DP[0], GT_prob)
        data.set_cohort(AD, DP)
        return data

    def fit(self, AD, DP=None, GT_prob=None, max_iter=200, min_iter=5, epsilon_conv=1e-3, learn_theta=True,
            delay_fit_theta=0):
        """The EM of vireo_bulk.py:44-108 for every sample, from the current psi and theta.

        AD, DP: (n_sample, n_variant); GT_prob: (n_variant, n_donor, n_GT); or a ``BulkData`` whose cohort is
        set in place of AD.  Leaves psi, theta, logLik (n_sample,), logLik_all (a list of n_sample arrays, each
        the reference's ``logLik[:it]`` of that sample), n_iter (n_sample,) and fit_ms_.  A sample's theta is
        replaced only if an update ran for it, as in ``VireoBulk.fit``."""
        AD, DP, GT_prob = self._data(AD, DP, GT_prob)
        psi0 = _matrix(self.psi, (self.n_sample, self.n_donor), "psi")
        theta0 = _matrix(self.theta, (self.n_sample, self.n_GT), "theta")
        max_iter, min_iter = int(max_iter), int(min_iter)
        if max_iter < 1:
            raise ValueError("max_iter must be >= 1")
        data = self._upload(AD, DP, GT_prob)
        psi, theta, traces, it, ms = data.fit_cohort(psi0, theta0, max_iter, min_iter, epsilon_conv, learn_theta,
                                                     delay_fit_theta)
        self.psi = psi
        if learn_theta:
            ran = it >= delay_fit_theta                # (otherwise no update ran: theta stays as given)
            theta0[ran] = theta[ran]
        self.theta = theta0
        self.logLik = traces[np.arange(self.n_sample), it]
        self.logLik_all = [traces[s, :it[s]].copy() for s in range(self.n_sample)]
        self.n_iter = it
        self.fit_ms_ = ms

    def LR_test(self, psi_null, AD, DP=None, GT_prob=None, log=False):
        """``LikRatio_test`` (vireo_bulk.py:120-167) of every sample's psi against ``psi_null`` -- (n_donor,) for
        one null shared by all samples, or (n_sample, n_donor) -- under that sample's theta, from one cohort
        log-likelihood pass.  -> (statistic (n_sample,), p-value (n_sample,)), n_donor - 1 degrees of freedom."""
        from scipy.stats import chi2

        AD, DP, GT_prob = self._data(AD, DP, GT_prob)
        null = np.asarray(psi_null)
        if null.dtype.kind not in "iufb":
            raise ValueError("psi_null has unsupported dtype %s" % null.dtype)
        if null.shape == (self.n_donor,):
            null = np.tile(null, (self.n_sample, 1))
        null = _matrix(null, (self.n_sample, self.n_donor), "psi_null")
        psi = _matrix(self.psi, (self.n_sample, self.n_donor), "psi")
        theta = _matrix(self.theta, (self.n_sample, self.n_GT), "theta")
        ll = self._upload(AD, DP, GT_prob).loglik_cohort(np.stack([psi, null], axis=1), theta)
        statistic = 2 * (ll[:, 0] - ll[:, 1])
        tail = chi2.logsf if log else chi2.sf
        return statistic, tail(statistic, self.n_donor - 1)


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
