"""NumPy restatement of the ambient-RNA step (predit_ambient / _fit_EM_ambient of vireoSNP 0.5.9,
variant_ELBO_gain), written from its description, on each cell's non-zero selected entries only.

The CPU tests pin it to the reference's fixtures; the GPU tests use it where the reference cannot
run (synthetic problems of any size, iteration counts)."""
import numpy as np
from scipy.special import digamma, logsumexp


def elbo_gain(ID_prob, AD, DP, pseudocount=0.5):
    """variant_ELBO_gain: (n_var,) for scipy sparse AD, DP (n_var x n_cell)"""
    def elbo(ad, dp):
        s1, s2, ss = ad + pseudocount, (dp - ad) + pseudocount, dp + 2 * pseudocount
        return s1 * digamma(s1) + s2 * digamma(s2) - ss * digamma(ss)
    ad_id = np.asarray(AD @ ID_prob)
    dp_id = np.asarray(DP @ ID_prob)
    ad1 = np.asarray(AD.sum(1)).ravel()
    dp1 = np.asarray(DP.sum(1)).ravel()
    return logsumexp(elbo(ad_id, dp_id), axis=1) - elbo(ad1, dp1)


def theta_of(GT_prob, beta_mu):
    return np.tensordot(GT_prob, beta_mu[0, :], axes=(2, 0))


def fit_cell(a, b, th, psi0, min_iter=20, max_iter=200, eps=1e-3, dtype=float, trace=None):
    """one cell: a, b (n_e,) counts of its selected entries, th (n_e, K) their theta rows.
    -> psi, var, llr, it (the loop index at exit, as in the reference).  ``dtype=np.longdouble``
    runs the same statements in extended precision (is a cell's exit decided by rounding?).  ``trace``: a list
    that receives logLik[0 .. it], which the reference does not return."""
    a = np.asarray(a, dtype)
    b = np.asarray(b, dtype)
    th = np.asarray(th, dtype)
    K = th.shape[1]
    if a.sum() + b.sum() == 0:           # 0 / 0 in the reference: NaN, the loop never breaks
        nan = np.full(K, np.nan)
        return nan, nan.copy(), np.nan, max_iter - 1
    psi = np.array(psi0, dtype)
    ll = np.zeros(max_iter, dtype)
    for it in range(max_iter):
        t1 = th @ psi
        t0 = (1 - th) @ psi
        raw = psi * (th.T @ (a / t1) + (1 - th).T @ (b / t0))
        psi = raw / raw.sum()
        tv = th @ psi
        ll[it] = np.sum(a * np.log(tv) + b * np.log(1 - tv))
        if it > min_iter:
            if ll[it] < ll[it - 1]:
                pass
            elif it == max_iter - 1:
                pass
            elif ll[it] - ll[it - 1] < eps:
                break
    if trace is not None:
        trace.extend(ll[:it + 1])
    tv = th @ psi
    var = 1.0 / ((th / tv[:, None]) ** 2 * a[:, None] + (th / (1 - tv[:, None])) ** 2 * b[:, None]).sum(0)
    tm = th[:, int(np.argmax(psi))]
    llr = ll[it - 1] - np.sum(a * np.log(tm) + b * np.log(1 - tm))
    return psi, var, llr, it


def cell_entries(AD, DP, sel, c):
    """(rows, a, b) of cell c's non-zero entries on selected variants (AD, DP: scipy CSC)"""
    dp = DP[:, c].toarray().ravel()
    ad = AD[:, c].toarray().ravel()
    rows = np.flatnonzero(sel & (dp > 0))
    return rows, ad[rows], dp[rows] - ad[rows]


def predict(theta, sel, AD, DP, psi0, cells=None, **kw):
    """every cell (or the listed ones): -> psi, var, llr, it arrays"""
    AD, DP = AD.tocsc(), DP.tocsc()
    cells = range(AD.shape[1]) if cells is None else cells
    out = []
    for c in cells:
        rows, a, b = cell_entries(AD, DP, sel, c)
        out.append(fit_cell(a, b, theta[rows], psi0[c], **kw))
    return (np.array([o[0] for o in out]), np.array([o[1] for o in out]),
            np.array([o[2] for o in out]), np.array([o[3] for o in out]))
