"""NumPy restatement of the bulk donor-abundance EM (VireoBulk.fit / LikRatio_test of vireoSNP 0.5.9).

``fit`` is an exact float64 restatement: to reproduce the reference's fixtures bit for bit it has to form the
same NumPy expressions in the same order (vireo_bulk.py:77-96, cited per helper), so its arithmetic follows the
reference's closely by necessity; it is organised as this project's own helpers (responsibilities, the two
M steps, the log-likelihood, the stop rule).  ``fit_chunked`` is written independently: the one-pass schedule
the device runs, over chunks of variants on a thread pool (partial sums added in chunk order), in float64 or
np.longdouble -- the arbiter of the full-size GPU tests, where a pool of 1 M variants must stay within minutes.

The CPU tests pin both to the reference's fixtures; the GPU tests use them where the reference cannot run.
Test infrastructure: the product never imports it."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np


def init(n_donor, n_GT=3, psi_init=None, theta_init=(0.01, 0.5, 0.99)):
    """the constructor's draws, in its order -> (psi, theta)"""
    psi = np.random.dirichlet([1] * n_donor)
    theta = np.random.rand(n_GT)
    if psi_init is not None and len(psi_init) == n_donor:
        psi = np.random.dirichlet([1] * n_donor)       # (the values of psi_init are not used)
    if theta_init is not None and len(theta_init) == n_GT:
        theta = np.array(theta_init, dtype=float)
    return psi, theta


def loglik(AD, BD, GT_prob, psi, theta):
    tv = np.dot(np.dot(GT_prob, theta), psi)
    return np.sum(AD * np.log(tv) + BD * np.log(1 - tv))


def stop_rule(ll, it, min_iter, max_iter, eps):
    """the reference's rule in its order -> (stop, warning or None)"""
    if it > min_iter:
        if ll[it] < ll[it - 1]:
            return False, "Warning: logLikelihood decreases!\n"
        elif it == max_iter - 1:
            return False, "Warning: VB did not converge!\n"
        elif ll[it] - ll[it - 1] < eps:
            return True, None
    return False, None


def stop_margin(ll_all, ll_last, min_iter, eps):
    """smallest |gain - eps| over the iterations where the rule is evaluated (inf if none)"""
    ll = np.append(np.asarray(ll_all, float), ll_last)
    gains = [abs((ll[i] - ll[i - 1]) - eps) for i in range(max(min_iter + 1, 1), len(ll))]
    gains = [g for g in gains if np.isfinite(g)]
    return min(gains) if gains else np.inf


def responsibilities(GT, psi, theta):
    """E step (vireo_bulk.py:77-82): per variant and donor, the share of an alternative read (Z1) and of a
    reference read (Z0) that the donor explains, each row normalised"""
    rate = np.tensordot(GT, theta, axes=(2, 0))
    share = []
    for r in (rate, 1 - rate):
        z = r * np.expand_dims(psi, 0)
        share.append(z / np.sum(z, axis=1, keepdims=True))
    return share


def psi_step(AD, BD, Z1, Z0):
    """vireo_bulk.py:85-86: expected reads per donor, normalised"""
    raw = np.dot(AD, Z1) + np.dot(BD, Z0)
    return raw / np.sum(raw)


def theta_step(AD, BD, GT, Z1, Z0):
    """vireo_bulk.py:89-91: expected alternative reads per genotype over all expected reads of it"""
    alt, ref = (np.dot(cnt, np.sum(GT * np.expand_dims(Z, 2), axis=1)) for cnt, Z in ((AD, Z1), (BD, Z0)))
    return alt / (alt + ref)


def fit(AD, DP, GT_prob, psi, theta, max_iter=200, min_iter=5, epsilon_conv=1e-3, learn_theta=True,
        delay_fit_theta=0, dtype=np.float64):
    """The reference's loop: E step, psi, theta (from the OLD responsibilities), logLik of the new
    parameters, stop rule.  -> dict(psi, theta, logLik, logLik_all, it, warnings)"""
    AD = np.asarray(AD).astype(dtype)
    BD = np.asarray(DP).astype(dtype) - AD
    GT = np.asarray(GT_prob).astype(dtype)
    psi = np.asarray(psi).astype(dtype)
    theta = np.asarray(theta).astype(dtype)
    ll = np.zeros(max_iter, dtype=dtype)
    warns = []
    with np.errstate(all="ignore"):
        for it in range(max_iter):
            Z1, Z0 = responsibilities(GT, psi, theta)
            psi = psi_step(AD, BD, Z1, Z0)
            if learn_theta and it >= delay_fit_theta:
                theta = theta_step(AD, BD, GT, Z1, Z0)
            ll[it] = loglik(AD, BD, GT, psi, theta)
            stop, w = stop_rule(ll, it, min_iter, max_iter, epsilon_conv)
            if w:
                warns.append(w)
            if stop:
                break
    return dict(psi=psi, theta=theta, logLik=ll[it], logLik_all=ll[:it], it=it, warnings=warns)


def _chunk_sums(AD, BD, GT, psi, theta, dtype, want_theta=True, tm=None):
    """one chunk of one pass: psi_raw, s1, s2 of the update from (psi, theta), logLik OF (psi, theta).
    tm: the chunk's (GT . theta, 1 - GT . theta) where theta is fixed (computed once by the caller); the
    sums are then taken in factored form, psi_k sum_n tm_nk AD_n / t1_n + ..., which needs no n x k
    temporary."""
    AD = AD.astype(dtype)
    BD = BD.astype(dtype)
    with np.errstate(all="ignore"):
        if tm is not None:
            tm, om = tm
            if dtype is np.float64:          # (BLAS)
                t1 = tm @ psi
                t0 = om @ psi
                raw = psi * ((AD / t1) @ tm + (BD / t0) @ om)
            else:                            # (NumPy's matrix products of other types are slow loops)
                q1, q0 = tm * psi[None, :], om * psi[None, :]
                t1, t0 = q1.sum(1), q0.sum(1)
                raw = ((AD / t1)[:, None] * q1).sum(0) + ((BD / t0)[:, None] * q0).sum(0)
            return raw, 0.0, 0.0, np.sum(AD * np.log(t1) + BD * np.log(1 - t1))
        GT = GT.astype(dtype)
        tm = np.tensordot(GT, theta, axes=(2, 0))
        q1 = tm * psi[None, :]
        q0 = (1 - tm) * psi[None, :]
        t1 = q1.sum(1)
        Z1 = q1 / t1[:, None]
        Z0 = q0 / q0.sum(1, keepdims=True)
        raw = np.dot(AD, Z1) + np.dot(BD, Z0)
        s1 = np.dot(AD, np.einsum("nkg,nk->ng", GT, Z1)) if want_theta else 0.0
        s2 = np.dot(BD, np.einsum("nkg,nk->ng", GT, Z0)) if want_theta else 0.0
        ll = np.sum(AD * np.log(t1) + BD * np.log(1 - t1))
    return raw, s1, s2, ll


def fit_chunked(AD, DP, GT_prob, psi, theta, max_iter=200, min_iter=5, epsilon_conv=1e-3, learn_theta=True,
                delay_fit_theta=0, dtype=np.longdouble, chunk=32768, threads=16):
    """The same loop on the one-pass schedule (pass p gives logLik[p - 1] and update p), in chunks."""
    AD = np.asarray(AD, dtype=np.float64)
    BD = np.asarray(DP, dtype=np.float64) - AD
    N = AD.size
    cuts = list(range(0, N, chunk))
    psi = np.asarray(psi).astype(dtype)
    theta = np.asarray(theta).astype(dtype)
    ll = np.zeros(max_iter, dtype=dtype)
    it = 0
    with ThreadPoolExecutor(threads) as pool:
        tms = {c: None for c in cuts}
        if not learn_theta:      # theta is fixed: GT . theta and its complement once
            def fixed(c):
                tm = np.tensordot(GT_prob[c:c + chunk].astype(dtype), theta, axes=(2, 0))
                return tm, 1 - tm
            tms = dict(zip(cuts, pool.map(fixed, cuts)))
        for p in range(max_iter + 1):
            parts = list(pool.map(lambda c: _chunk_sums(AD[c:c + chunk], BD[c:c + chunk], GT_prob[c:c + chunk],
                                                        psi, theta, dtype, learn_theta, tms[c]), cuts))
            raw, s1, s2, llp = parts[0]
            for x in parts[1:]:                      # (chunk order)
                raw, s1, s2, llp = raw + x[0], s1 + x[1], s2 + x[2], llp + x[3]
            if p >= 1:
                it = p - 1
                ll[it] = llp
                if stop_rule(ll, it, min_iter, max_iter, epsilon_conv)[0] or it == max_iter - 1:
                    break
            psi = raw / np.sum(raw)
            if learn_theta and p >= delay_fit_theta:
                theta = s1 / (s1 + s2)
    return dict(psi=psi, theta=theta, logLik=ll[it], logLik_all=ll[:it], it=it)


def lik_ratio(psi, psi_null, AD, DP, GT_prob, theta, log=False, dtype=np.float64):
    from scipy.stats import chi2
    AD = np.asarray(AD).astype(dtype)
    BD = np.asarray(DP).astype(dtype) - AD
    GT = np.asarray(GT_prob).astype(dtype)
    theta = np.asarray(theta).astype(dtype)
    LR = 2 * (loglik(AD, BD, GT, np.asarray(psi).astype(dtype), theta)
              - loglik(AD, BD, GT, np.asarray(psi_null).astype(dtype), theta))
    df = len(psi_null) - 1
    return LR, (chi2.logsf(float(LR), df) if log else chi2.sf(float(LR), df))


def synth_pool(n_var, n_donor, n_GT=3, seed=0, depth=30.0, sharp=0.97, private=True):
    """A planted pool: one-hot-ish genotype probabilities, Dirichlet abundances, Poisson depths, binomial
    alternative counts drawn from the model itself.  private: every variant is carried by ONE donor (genotype
    1 .. n_GT - 1, the others 0), which separates the donors' reads and lets the EM converge in tens of
    iterations; otherwise every genotype is uniform, the donors overlap and the EM takes thousands.
    -> AD, DP (int64), GT_prob (float64), psi, theta (planted)"""
    rng = np.random.default_rng(seed)
    theta = np.linspace(0.01, 0.99, n_GT)
    psi = rng.dirichlet(np.full(n_donor, 2.0))
    if private:
        gt = np.zeros((n_var, n_donor), dtype=np.int64)
        gt[np.arange(n_var), rng.integers(0, n_donor, size=n_var)] = rng.integers(1, n_GT, size=n_var)
    else:
        gt = rng.integers(0, n_GT, size=(n_var, n_donor))
    GT = gt_from_index(gt, n_GT, sharp)
    rate = np.tensordot(GT, theta, axes=(2, 0)) @ psi
    DP = rng.poisson(depth, size=n_var).astype(np.int64)
    AD = rng.binomial(DP, rate).astype(np.int64)
    return AD, DP, GT, psi, theta


def psi_standard_error(DP, GT_prob, psi, theta):
    """Cramer-Rao standard errors of psi from the planted rates and depths.  AD_n ~ Binomial(DP_n, t_n) with
    t_n = tm_n . psi has Fisher information I = sum_n DP_n tm_n tm_n' / (t_n (1 - t_n)); the EM keeps
    sum(psi) = 1, so the bound is that of the constrained estimate: C - C 1 1' C / (1' C 1) with C = I^-1
    (the unconstrained inverse projected onto the constraint's tangent space), the square roots of its
    diagonal."""
    tm = np.tensordot(GT_prob, theta, axes=(2, 0))
    t = tm @ psi
    info = (tm * (np.asarray(DP, float) / (t * (1 - t)))[:, None]).T @ tm
    C = np.linalg.inv(info)
    c1 = C.sum(1)
    return np.sqrt(np.diag(C - np.outer(c1, c1) / c1.sum()))


def gt_from_index(gt_index, n_GT, sharp):
    """GT_prob with `sharp` at gt_index[n, k] and the rest spread evenly (the synthetic-genotype fixtures)"""
    gt_index = np.asarray(gt_index).astype(np.int64)
    GT = np.full(gt_index.shape + (n_GT,), (1.0 - sharp) / (n_GT - 1))
    np.put_along_axis(GT, gt_index[:, :, None], sharp, axis=2)
    return GT


def c1_bulk():
    """pseudo-bulk of the c1 fixture: AD.sum(1), DP.sum(1) (int64) and the GT_prob of c1_wrap_seed2_init4"""
    from tests import gold
    AD, DP = gold.c1()
    GT = gold.load("c1_wrap_seed2_init4")["GT_prob"]
    return np.asarray(AD.sum(1)).ravel().astype(np.int64), np.asarray(DP.sum(1)).ravel().astype(np.int64), GT


def fixture_inputs(g):
    """(AD, DP, GT_prob, constructor kwargs, fit kwargs) of a c1_bulk_* fixture"""
    AD, DP, GT = c1_bulk()
    if "gt_index" in g:
        GT = gt_from_index(g["gt_index"], int(g["n_GT"]), float(g["gt_sharp"]))
    if "zero_row" in g:
        GT = GT.copy()
        GT[int(g["zero_row"])] = 0.0
    ctor, fit = {}, {}
    for k in g:
        if k.startswith("ctor_") and not k.endswith("_is_none") and k != "ctor_warning":
            ctor[k[5:]] = None if bool(g[k + "_is_none"]) else [float(x) for x in g[k]]
        elif k.startswith("fit_"):
            fit[k[4:]] = g[k].item()
    return AD, DP, GT, ctor, fit


FIT_CASES = ["c1_bulk_seed1", "c1_bulk_seed2", "c1_bulk_seed3", "c1_bulk_notheta", "c1_bulk_delay3",
             "c1_bulk_maxiter8", "c1_bulk_min0_eps1", "c1_bulk_thetadrawn", "c1_bulk_psiinit",
             "c1_bulk_badinit", "c1_bulk_gt2", "c1_bulk_k7", "c1_bulk_nan"]
