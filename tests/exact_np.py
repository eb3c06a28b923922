"""One EM update or post-fit step in extended precision, with the error unit of every output.
TEST INFRASTRUCTURE ONLY.

A restatement of the single updates of the reference (vireoSNP 0.5.9; the lines are cited per
function, relative to the reference tree) in ``np.longdouble`` (eps 1.1e-19): SciPy's sparse
products run on long-double data, ``digamma`` / ``loggamma`` come from ``mpmath`` at 40 digits, as
in tests/golden/make_c3_arbiter.py.  Its own rounding is ~5e-4 of float64's, so it can judge a
float64 kernel to a fraction of one rounding.

The float64 state handed in (what ``DeviceModel.get_state`` / ``get_loglik`` read back) is taken
as exact input.  Every function returns ``{name: (value, unit)}`` with ``unit`` the size of ONE
float64 rounding of that output, an absolute number per element:

* a sum of signed terms (beta_sum, the two parts of beta_mu, logLik_ID, every ELBO part):
  ``EPS * sum|terms|``, from a second pass over the absolute values; the Beta KL counts each
  lgamma and each (q - 1) * psi on its own;
* a softmax output p: ``p * (2 * max_k unit(logit[row, k]) + EPS)``  (d p_k = p_k (dz_k - sum_j
  p_j dz_j), at most 2 max|dz| relative, plus the rounding of the result);
* a ratio (beta_mu): the relative units of numerator and denominator added.

The steps on a fitted model (``cell_loglik``, ``doublet``, ``donor_reads``) and one variant's own
mixture (``varmix_row``, a chain whose intermediate state cannot be read back: there the rounding
of one stage is carried into the next as a unit) follow the same conventions; their cases are in
tests/exact_postfit.py.  One update of the bulk donor-abundance EM and its log-likelihood
(``bulk_update``, ``bulk_loglik``) carry their stages' units the same way; their cases are in
tests/exact_bulk.py.  So do the per-cell ambient EM at a forced length and the ELBO gain of a variant
(``ambient_cell``, ``elbo_gain``); their cases are in tests/exact_ambient.py.

``distance`` expresses a float64 result in these units; ``held`` is the rule the tests assert.
"""
import mpmath
import numpy as np
from scipy.sparse import csc_matrix
from scipy.special import polygamma

LD = np.longdouble
EPS = 2.0 ** -53
TINY = 1e-290           # below this the suite compares probabilities absolutely (ATOL of the parity tests)
FACTOR = 4.0            # the margin of tests/test_gpu_postfit_sweep.py: two correct float64 sums


def ld(x):
    return np.asarray(x, dtype=LD)


# ------------------------------------------------------------------------------------
# special functions: mpmath at 40 digits on the distinct arguments
# ------------------------------------------------------------------------------------
def _mp(x):
    """long double -> mpf without loss (two float64 halves)"""
    hi = float(x)
    return mpmath.mpf(hi) + mpmath.mpf(float(x - LD(hi)))


_MEMO = {}              # fn -> {(hi, lo): value}: one update's functions share their arguments


def _special(fn, v):
    v = ld(v)
    u, inv = np.unique(v.ravel(), return_inverse=True)
    memo = _MEMO.setdefault(fn, {})
    if len(memo) > 1 << 20:
        memo.clear()
    hi = u.astype(np.float64)
    lo = (u - hi.astype(LD)).astype(np.float64)      # (the two halves of ``_mp``)
    out = np.empty(u.shape, dtype=LD)
    with mpmath.workdps(40):
        for i, key in enumerate(zip(hi.tolist(), lo.tolist())):
            val = memo.get(key)
            if val is None:
                val = memo[key] = LD(mpmath.nstr(fn(mpmath.mpf(key[0]) + mpmath.mpf(key[1])), 30))
            out[i] = val
    return out[inv.ravel()].reshape(v.shape)


def psi(v):
    return _special(mpmath.digamma, v)


def lgam(v):
    return _special(mpmath.loggamma, v)


# ------------------------------------------------------------------------------------
# the count matrices, long double, both orientations
# ------------------------------------------------------------------------------------
class Counts:
    """AD, BD = DP - AD and DP as long-double CSC (N x M) and their transposes (M x N)"""

    def __init__(self, AD, DP):
        AD, DP = csc_matrix(AD), csc_matrix(DP)
        BD = csc_matrix(DP - AD)

        def up(X):
            return csc_matrix((X.data.astype(LD), X.indices, X.indptr), shape=X.shape)

        self.AD, self.BD, self.DP = up(AD), up(BD), up(DP)
        self.ADt, self.BDt, self.DPt = (up(csc_matrix(X.T)) for X in (AD, BD, DP))
        self.shape = AD.shape
        per_cell = np.diff(DP.indptr)
        per_var = np.diff(csc_matrix(DP.T).indptr)
        # the longest contracted row or column: the length of the longest sequential sum
        self.longest = int(max(per_cell.max(initial=0), per_var.max(initial=0)))


def shapes(mu, sm):
    """theta_s1, theta_s2 (vireo_model.py:139-147, bmm_model.py:107-115)"""
    mu, sm = ld(mu), ld(sm)
    return mu * sm, (1 - mu) * sm


def softmax(L, unit_L, log_prior):
    """normalize(exp(loglik_amplify(L + log prior))) over the last axis (vireo_model.py:198-199,
    :218-219, bmm_model.py:153-154; vireo_base.py:44-74) -> (p, unit)"""
    z = L + log_prior
    uz = unit_L + EPS * np.abs(log_prior)
    z = z - z.max(axis=-1, keepdims=True)
    p = np.exp(z)
    p = p / p.sum(axis=-1, keepdims=True)
    return p, p * (2 * uz.max(axis=-1, keepdims=True) + EPS)


def _log_prior(prior, n_class):
    """log of a prior table (None: uniform over the last axis)"""
    if prior is None:
        return -np.log(LD(n_class))
    return np.log(ld(prior))


def _rel_entr(p, prior, n_class):
    """sum of scipy.stats.entropy(p, prior, axis=-1) (vireo_model.py:237-238, bmm_model.py:162):
    both normalised over the last axis, 0 log 0 = 0.  Terms: p log p and -p log q."""
    p = ld(p)
    p = p / p.sum(axis=-1, keepdims=True)
    if prior is None:
        logq = np.full(p.shape, -np.log(LD(n_class)), dtype=LD)
    else:
        q = ld(prior)
        logq = np.broadcast_to(np.log(q / q.sum(axis=-1, keepdims=True)), p.shape)
    m = p > 0
    a = p[m] * np.log(p[m])
    b = p[m] * logq[m]
    return np.sum(a - b), EPS * np.sum(np.abs(a) + np.abs(b))


def _beta_kl(s1, s2, q1, q2):
    """KL(Beta(s1, s2) || Beta(q1, q2)) summed over all entries: beta_entropy with a prior
    (vireo_base.py:77-127), cross(post, prior) - cross(post, post) -> (value, unit)"""
    q1, q2 = np.broadcast_to(ld(q1), s1.shape), np.broadcast_to(ld(q2), s1.shape)
    d1, d2, ds = psi(s1), psi(s2), psi(s1 + s2)

    def cross(a, b):
        terms = [lgam(a), lgam(b), -lgam(a + b), -(a - 1) * d1, -(b - 1) * d2, (a + b - 2) * ds]
        return sum(terms), sum(np.abs(t) for t in terms)

    cq, aq = cross(q1, q2)
    cp, ap = cross(s1, s2)
    return np.sum(cq - cp), EPS * np.sum(aq + ap)


# ------------------------------------------------------------------------------------
# Vireo (vireoSNP/utils/vireo_model.py)
# ------------------------------------------------------------------------------------
def vireo_theta(C, ID, GT, p1, p2, sm_old, ase=False, fix_beta_sum=False):
    """update_theta_size (vireo_model.py:165-185): s1 = prior + sum (AD @ ID) * GT over donors
    (ASE mode) or over variants and donors."""
    ID, GT = ld(ID), ld(GT)
    A, B = C.AD @ ID, C.BD @ ID
    ax = 1 if ase else (0, 1)
    t1 = np.sum(A[:, :, None] * GT, axis=ax).reshape(-1, GT.shape[2])
    t2 = np.sum(B[:, :, None] * GT, axis=ax).reshape(-1, GT.shape[2])
    a1 = np.abs(ld(p1)) + np.sum(np.abs(A)[:, :, None] * np.abs(GT), axis=ax).reshape(t1.shape)
    a2 = np.abs(ld(p2)) + np.sum(np.abs(B)[:, :, None] * np.abs(GT), axis=ax).reshape(t2.shape)
    s1, s2 = ld(p1) + t1, ld(p2) + t2
    mu = s1 / (s1 + s2)
    out = {"beta_mu": (mu, mu * EPS * (a1 / s1 + (a1 + a2) / (s1 + s2)))}
    if fix_beta_sum:        # vireo_model.py:184: beta_sum stays
        sm = np.broadcast_to(ld(sm_old), mu.shape)
        out["beta_sum"] = (sm, EPS * np.abs(sm))
    else:
        out["beta_sum"] = (s1 + s2, EPS * (a1 + a2))
    return out


def vireo_gt(C, ID, mu, sm, GT_prior, n_gt):
    """update_GT_prob (vireo_model.py:204-219)"""
    ID = ld(ID)
    A, S = C.AD @ ID, C.DP @ ID
    B = S - A
    s1, s2 = shapes(mu, sm)
    d1, d2, ds = (x[:, None, :] for x in (psi(s1), psi(s2), psi(s1 + s2)))
    A, B, S = A[:, :, None], B[:, :, None], S[:, :, None]
    L = A * d1 + B * d2 - S * ds
    unit = EPS * (A * np.abs(d1) + B * np.abs(d2) + S * np.abs(ds))
    GT, u = softmax(L, unit, _log_prior(GT_prior, n_gt))
    return {"GT_prob": (GT, u)}


def vireo_loglik(C, GT, mu, sm):
    """logLik_ID of update_ID_prob / get_ELBO (vireo_model.py:190-196, :227-234): the 3 T
    transposed products, regrouped as AD' Wa + BD' Wb - DP' Ws (make_c3_arbiter.py)"""
    GT = ld(GT)
    s1, s2 = shapes(mu, sm)
    d = [x[:, None, :] for x in (psi(s1), psi(s2), psi(s1 + s2))]
    W = [np.sum(GT * x, axis=2) for x in d]
    Wabs = [np.sum(np.abs(GT) * np.abs(x), axis=2) for x in d]
    L = C.ADt @ W[0] + C.BDt @ W[1] - C.DPt @ W[2]
    unit = EPS * (C.ADt @ Wabs[0] + C.BDt @ Wabs[1] + C.DPt @ Wabs[2])
    return {"logLik_ID": (L, unit)}


def id_from_loglik(L, unit_L, ID_prior, n_donor):
    """the tail of update_ID_prob (vireo_model.py:198-199, bmm_model.py:153-154)"""
    p, u = softmax(ld(L), unit_L, _log_prior(ID_prior, n_donor))
    return {"ID_prob": (p, u)}


def vireo_elbo_parts(L, ID, GT, mu, sm, ID_prior, GT_prior, p1, p2):
    """LB_p, KL_ID, KL_GT, KL_theta of get_ELBO (vireo_model.py:236-248)"""
    L, ID, GT = ld(L), ld(ID), ld(GT)
    s1, s2 = shapes(mu, sm)
    t = L * ID
    return {"LB_p": (np.sum(t), EPS * np.sum(np.abs(t))),
            "KL_ID": _rel_entr(ID, ID_prior, ID.shape[1]),
            "KL_GT": _rel_entr(GT, GT_prior, GT.shape[2]),
            "KL_theta": _beta_kl(s1, s2, p1, p2)}


# ------------------------------------------------------------------------------------
# BinomMixtureVB (vireoSNP/utils/bmm_model.py)
# ------------------------------------------------------------------------------------
def bmm_theta(C, ID, p1, p2, sm_old, fix_beta_sum=False):
    """update_theta_size (bmm_model.py:133-144)"""
    ID = ld(ID)
    s1 = C.AD @ ID + ld(p1)
    s2 = C.BD @ ID + ld(p2)
    a1 = C.AD @ np.abs(ID) + np.abs(ld(p1))
    a2 = C.BD @ np.abs(ID) + np.abs(ld(p2))
    mu = s1 / (s1 + s2)
    out = {"beta_mu": (mu, mu * EPS * (a1 / s1 + (a1 + a2) / (s1 + s2)))}
    if fix_beta_sum:        # bmm_model.py:143
        sm = np.broadcast_to(ld(sm_old), mu.shape)
        out["beta_sum"] = (sm, EPS * np.abs(sm))
    else:
        out["beta_sum"] = (s1 + s2, EPS * (a1 + a2))
    return out


def bmm_loglik(C, mu, sm):
    """get_E_logLik (bmm_model.py:118-130)"""
    s1, s2 = shapes(mu, sm)
    d1, d2, ds = psi(s1), psi(s2), psi(s1 + s2)
    L = C.ADt @ d1 + C.BDt @ d2 - C.DPt @ ds
    unit = EPS * (C.ADt @ np.abs(d1) + C.BDt @ np.abs(d2) + C.DPt @ np.abs(ds))
    return {"logLik_ID": (L, unit)}


def bmm_elbo_parts(L, ID, mu, sm, ID_prior, p1, p2):
    """LB_p, KL_ID, KL_theta of get_ELBO (bmm_model.py:157-175)"""
    L, ID = ld(L), ld(ID)
    s1, s2 = shapes(mu, sm)
    t = L * ID
    return {"LB_p": (np.sum(t), EPS * np.sum(np.abs(t))),
            "KL_ID": _rel_entr(ID, ID_prior, ID.shape[1]),
            "KL_theta": _beta_kl(s1, s2, p1, p2)}


# ------------------------------------------------------------------------------------
# the steps on a fitted model (vireoSNP/utils/vireo_doublet.py, vireoSNP/vireo.py:240-241)
# ------------------------------------------------------------------------------------
def cell_loglik(C, GT, psi1, psi2, psis, ID_prior):
    """vireo_doublet.py:53-68 against a given (n_var, n_col, n_class) genotype table: the 3 n_class
    transposed products, regrouped as in ``vireo_loglik``, and the posterior with ``ID_prior``
    (None: uniform; else 1 or n_cell rows).  psi*: the caller's float64 tables, (1 | n_var, n_class)."""
    GT = ld(GT)
    d = [ld(x)[:, None, :] for x in (psi1, psi2, psis)]
    W = [np.sum(GT * x, axis=2) for x in d]
    Wabs = [np.sum(np.abs(GT) * np.abs(x), axis=2) for x in d]
    L = C.ADt @ W[0] + C.BDt @ W[1] - C.DPt @ W[2]
    unit = EPS * (C.ADt @ Wabs[0] + C.BDt @ Wabs[1] + C.DPt @ Wabs[2])
    p, u = softmax(L, unit, _log_prior(ID_prior, GT.shape[1]))
    return {"logLik": (L, unit), "prob": (p, u)}


def doublet_table(GT):
    """add_doublet_GT (vireo_doublet.py:105-136) in long double: the singlet columns padded with
    zero mixed classes, then every donor pair (itertools.combinations order) over the T same and
    the T (T - 1) / 2 mixed classes, normalised over the classes"""
    GT = ld(GT)
    N, K, T = GT.shape
    a, b = np.triu_indices(K, 1)             # (row-major: the order of combinations)
    g1, g2 = np.triu_indices(T, 1)
    P, Q = GT[:, a, :], GT[:, b, :]
    both = np.concatenate([P * Q, P[:, :, g1] * Q[:, :, g2] + P[:, :, g2] * Q[:, :, g1]], axis=2)
    both = both / both.sum(axis=2, keepdims=True)
    single = np.concatenate([GT, np.zeros((N, K, g1.size), dtype=LD)], axis=2)
    return np.concatenate([single, both], axis=1)


def doublet(C, GT, psi1, psi2, psis, prior_both):
    """predict_doublet's logLik_ID and posterior (vireo_doublet.py:11-68) from the fitted GT_prob,
    the digamma tables of add_doublet_theta's classes and the prior of all K + K (K - 1) / 2 columns
    (None: uniform)"""
    return cell_loglik(C, doublet_table(GT), psi1, psi2, psis, prior_both)


def donor_reads(C, ID):
    """AD @ ID_prob and DP @ ID_prob (vireo.py:240-241)"""
    ID = ld(ID)
    absID = np.abs(ID)
    return {"AD_reads": (C.AD @ ID, EPS * (C.AD @ absID)), "DP_reads": (C.DP @ ID, EPS * (C.DP @ absID))}


# ------------------------------------------------------------------------------------
# one variant's own mixture (BinomMixtureVB._fit_BV on a 1 x n_cell row, bmm_model.py:178-201)
# ------------------------------------------------------------------------------------
def varmix_row(ad, dp, K, n_iter):
    """The protocol of tests/varmix_np.fit_row on the covered cells of one row: the deterministic
    start, then ``n_iter`` iterations of theta -> logits -> softmax -> ELBO.  -> (list of
    {ELBO, beta_mu, beta_sum, size} per iteration, elbo_one), every entry (value, unit).

    No intermediate state of a fit can be read back, so what one stage rounds is carried into the
    next as a unit: u(ID_ik) = ID_ik (2 max_k unit(L_ik) + EPS) (the softmax's rule; 3 EPS ID for the
    start values, three roundings), into size_k as sum_i u(ID_ik), into the sums of the next theta
    as sum_i a_i u(ID_ik), and from those sums into the logits as a_i psi'(s1_k) u(s1_k) + ... (on a
    row with a few cells of 1e6 reads the float64 restatement is 870 units out in ``size`` without
    this last term: the deep cells' rounding moves a component's shapes, and those every cell's
    logits)."""
    ad, dp = np.asarray(ad), np.asarray(dp)
    cov = dp > 0
    a, d = ld(ad[cov]), ld(dp[cov])
    b = d - a
    f = a / d
    c = ld(np.arange(K)) / LD(K - 1)
    ID = np.maximum(LD(0), 1 - np.abs(f[:, None] - c[None, :]) * LD(K - 1)) + LD(1) / 64
    ID = ID / ID.sum(axis=1, keepdims=True)
    ID = ID / ID.sum(axis=1, keepdims=True)          # set_initial normalises once more (bmm_model.py:80-81)
    uID = 3 * EPS * ID
    out = []
    for _ in range(n_iter):
        s1, s2 = 1 + a @ ID, 1 + b @ ID              # update_theta_size (:133-144)
        u1 = EPS * s1 + a @ uID
        u2 = EPS * s2 + b @ uID
        mu = s1 / (s1 + s2)
        d1, d2, ds = psi(s1), psi(s2), psi(s1 + s2)
        L = a[:, None] * d1 + b[:, None] * d2 - d[:, None] * ds      # get_E_logLik (:118-130)
        uL = EPS * (a[:, None] * np.abs(d1) + b[:, None] * np.abs(d2) + d[:, None] * np.abs(ds))
        # (what the sums carry moves the digammas: psi'(s) u(s), a float64 trigamma is plenty for a unit)
        t1, t2, ts = (ld(polygamma(1, np.asarray(x, dtype=np.float64))) for x in (s1, s2, s1 + s2))
        uL = uL + a[:, None] * (t1 * u1) + b[:, None] * (t2 * u2) + d[:, None] * (ts * (u1 + u2))
        ID, uID = softmax(L, uL, -np.log(LD(K)))     # update_ID_prob (:147-154)
        lb = L * ID
        m = ID > 0
        ent = np.zeros(ID.shape, dtype=LD)
        ent[m] = ID[m] * np.log(ID[m] * K)
        kl, ukl = _beta_kl(s1, s2, 1.0, 1.0)
        out.append({"ELBO": (np.sum(lb) - np.sum(ent) - kl,
                             EPS * (np.sum(np.abs(lb)) + np.sum(np.abs(ent))) + ukl),
                    "beta_mu": (mu, mu * (u1 / s1 + (u1 + u2) / (s1 + s2))),
                    "beta_sum": (s1 + s2, u1 + u2),
                    "size": (ID.sum(axis=0), EPS * ID.sum(axis=0) + uID.sum(axis=0))})
    ta, tb = a.sum(), b.sum()                        # exact integers
    s1, s2 = np.array([1 + ta]), np.array([1 + tb])
    terms = [ta * psi(s1)[0], tb * psi(s2)[0], -(ta + tb) * psi(s1 + s2)[0]]
    kl, ukl = _beta_kl(s1, s2, 1.0, 1.0)
    one = (sum(terms) - kl, EPS * sum(abs(t) for t in terms) + ukl)
    return out, one


# ------------------------------------------------------------------------------------
# bulk donor abundance (vireoSNP/utils/vireo_bulk.py:75-96; the factored form of csrc/vrx_bulk.h)
# ------------------------------------------------------------------------------------
def _bulk_rates(GT, theta):
    """tm[n, k] = sum_g P[n, k, g] theta_g and 1 - tm, each with its unit (a sum; one more rounding
    for the complement, whose cancellation where tm -> 1 belongs to the formula)"""
    P, th = np.asarray(GT, dtype=np.float64), ld(theta)      # (a genotype class at a time: no long-double copy)
    tm = sum(P[:, :, g] * th[g] for g in range(P.shape[2]))
    utm = EPS * sum(np.abs(P[:, :, g]) * np.abs(th[g]) for g in range(P.shape[2]))
    om = 1 - tm
    return P, tm, utm, om, utm + EPS * np.abs(om)


def _bulk_fold(x, P):
    """sum_nk x[n, k] P[n, k, g] per class g"""
    return np.array([(x * P[:, :, g]).sum() for g in range(P.shape[2])], dtype=LD)


def bulk_update(AD, BD, GT, psi, theta):
    """One EM update of VireoBulk.fit (vireo_bulk.py:77-91) from float64 (psi, theta), taken as exact:
    -> {"psi": (psi', unit), "theta": (theta', unit)}.

    No intermediate can be read back, so every stage carries the unit of the stage it reads:
    u(tm) into t1 = sum_k tm_k psi_k and t0; u(t1) / t1 and u(tm_k) into every term
    x1_nk = (AD_n / t1_n) tm_nk psi_k (three roundings of its own: the division and two products),
    likewise x0; the terms' units into psi_raw_k = sum_n x1 + x0, s1_g = sum_nk x1 P and s2_g, each
    also a sum of its own (EPS sum|terms|); psi' = raw / sum raw and theta' = s1 / (s1 + s2) are ratios.
    Written without a division by tm, raw or s1: a donor of psi_k = 0 keeps psi'_k = 0 with unit 0."""
    a, b, psi = ld(AD), ld(BD), ld(psi)
    P, tm, utm, om, uom = _bulk_rates(GT, theta)
    q1, q0 = tm * psi, om * psi
    t1, t0 = q1.sum(axis=1), q0.sum(axis=1)
    ut1 = EPS * np.abs(q1).sum(axis=1) + (utm * psi).sum(axis=1)
    ut0 = EPS * np.abs(q0).sum(axis=1) + (uom * psi).sum(axis=1)
    w1, w0 = a / t1, b / t0
    x1, x0 = w1[:, None] * q1, w0[:, None] * q0
    ux1 = x1 * (ut1 / t1 + 3 * EPS)[:, None] + w1[:, None] * psi * utm
    ux0 = x0 * (ut0 / t0 + 3 * EPS)[:, None] + w0[:, None] * psi * uom
    raw = (x1 + x0).sum(axis=0)
    uraw = EPS * raw + (ux1 + ux0).sum(axis=0)
    s1, s2 = _bulk_fold(x1, P), _bulk_fold(x0, P)
    u1, u2 = EPS * s1 + _bulk_fold(ux1, P), EPS * s2 + _bulk_fold(ux0, P)
    tot = raw.sum()
    utot = EPS * tot + uraw.sum()
    new_psi = raw / tot
    new_theta = s1 / (s1 + s2)
    return {"psi": (new_psi, uraw / tot + new_psi * utot / tot),
            "theta": (new_theta, u1 / (s1 + s2) + new_theta * (u1 + u2) / (s1 + s2))}


def bulk_loglik(AD, BD, GT, psi, theta):
    """sum_n AD_n log t1_n + BD_n log(1 - t1_n), t1 = GT . theta . psi (vireo_bulk.py:94-96, :152-158),
    for one psi (K,) or several (Q, K) -> (value, unit), scalars or (Q,).

    A sum of its 2 N terms, which also carries what t1 carries: d log t1 = u(t1) / t1 and
    d log(1 - t1) = (u(t1) + EPS (1 - t1)) / (1 - t1), the rounding of the complement included.  Both
    sides form log(1 - t1), so its cancellation where t1 -> 1 (and the absolute rounding of 1 - t1
    where t1 -> 0) is the formula's and stands in the unit.  The exact side takes log1p(-t1)."""
    a, b = ld(AD)[:, None], ld(BD)[:, None]
    psi = ld(psi)
    one = psi.ndim == 1
    Q = np.atleast_2d(psi).T                        # (K, Q)
    _, tm, utm, _, _ = _bulk_rates(GT, theta)
    t1 = tm @ Q
    ut1 = EPS * (np.abs(tm) @ np.abs(Q)) + utm @ np.abs(Q)
    la, lb = a * np.log(t1), b * np.log1p(-t1)
    value = (la + lb).sum(axis=0)
    carried = a * ut1 / t1 + b * (ut1 + EPS * (1 - t1)) / (1 - t1)
    unit = EPS * (np.abs(la) + np.abs(lb)).sum(axis=0) + carried.sum(axis=0)
    return (value[0], unit[0]) if one else (value, unit)


# ------------------------------------------------------------------------------------
# ambient RNA (vireoSNP/utils/vireo_doublet.py:139-210, variant_select.py:66-106; the factored form of
# csrc/vrx_ambient.h)
# ------------------------------------------------------------------------------------
def _amb_loglik(a, b, t1, ut1):
    """sum_e a log t1 + b log(1 - t1) with what t1 carries, as ``bulk_loglik``: the cancellation of
    1 - t1 is the formula's and stands in the unit; the exact side takes log1p(-t1)"""
    la, lb = a * np.log(t1), b * np.log1p(-t1)
    carried = a * ut1 / t1 + b * (ut1 + EPS * (1 - t1)) / (1 - t1)
    return (la + lb).sum(), EPS * (np.abs(la) + np.abs(lb)).sum() + carried.sum()


def ambient_cell(a, b, th, psi0, n_updates):
    """One cell of the ambient EM by the header formulas of csrc/vrx_ambient.h, exactly ``n_updates``
    updates psi_k <- psi_k r_k / sum_j psi_j r_j from psi0 and no stop rule: what the device returns when
    min_iter = max_iter = n_updates and epsilon = 0.  a, b (n_e,): the counts of the cell's selected
    entries, th (n_e, K) their theta rows, all float64 or integer and taken as exact.
    -> {"psi": psi after n_updates updates, "var": 1 / Fisher information at that psi,
        "llr": L(psi after n_updates - 1 updates) - L0}, each (value, unit); L0 is the one-donor
    log-likelihood at the first maximum of the final psi.  NaN throughout without selected counts.

    No intermediate can be read back, so every stage carries the unit of the stage it reads:
    u(t1) = EPS t1 + th . u(psi), u(t0) likewise with one more rounding for 1 - th; the weights a / t1 and
    b / t0 carry u(t) / t + EPS relative; r_k is a sum of its own (EPS sum|terms|) plus the weights' carry;
    psi r, its sum and the ratio add their relative units, into the next update's u(psi).  Written without
    a division by psi or r: a component of exactly 0 stays 0 with unit 0.  The Fisher sums carry twice the
    relative unit of t1 and of 1 - t1 (three roundings a term: the square, the division, the product), var
    that of a ratio, llr u(L) + u(L0) and its own rounding."""
    a, b, th, psi = ld(a), ld(b), ld(th), ld(psi0)
    K = th.shape[1]
    if a.sum() + b.sum() == 0:
        nan = np.full(K, np.nan, dtype=LD)
        return {"psi": (nan, nan.copy()), "var": (nan.copy(), nan.copy()), "llr": (LD(np.nan), LD(np.nan))}
    om = 1 - th
    upsi = np.zeros(K, dtype=LD)
    L = uL = None
    for _ in range(n_updates):
        t1, t0 = th @ psi, om @ psi
        ut1 = EPS * t1 + th @ upsi
        ut0 = 2 * EPS * t0 + om @ upsi
        L, uL = _amb_loglik(a, b, t1, ut1)              # of the psi this update starts from
        x1, x0 = th * (a / t1)[:, None], om * (b / t0)[:, None]
        r = (x1 + x0).sum(axis=0)
        ur = EPS * (x1 + x0).sum(axis=0) + (x1 * (ut1 / t1 + EPS)[:, None] + x0 * (ut0 / t0 + EPS)[:, None]).sum(axis=0)
        q = psi * r
        uq = upsi * r + psi * ur + EPS * q
        tot = q.sum()
        utot = EPS * tot + uq.sum()
        psi = q / tot
        upsi = uq / tot + psi * (utot / tot + EPS)
    t1 = th @ psi
    ut1 = EPS * t1 + th @ upsi
    c1 = 1 - t1
    uc1 = ut1 + EPS * c1
    f1, f0 = a / (t1 * t1), b / (c1 * c1)
    uf = f1 * (2 * ut1 / t1 + 3 * EPS) + f0 * (2 * uc1 / c1 + 3 * EPS)
    th2 = th * th
    fisher = th2.T @ (f1 + f0)
    ufisher = EPS * fisher + th2.T @ uf
    var = 1 / fisher
    tm = th[:, int(np.argmax(psi))]                     # exact inputs: a sum, and the rounding of 1 - tm
    la, lb = a * np.log(tm), b * np.log1p(-tm)
    L0, uL0 = (la + lb).sum(), EPS * (np.abs(la) + np.abs(lb) + b).sum()
    llr = L - L0
    return {"psi": (psi, upsi), "var": (var, var * (ufisher / fisher + EPS)),
            "llr": (llr, uL + uL0 + EPS * np.abs(llr))}


def elbo_gain(C, ID, pseudocount):
    """variant_ELBO_gain (variant_select.py:66-106) from ``donor_reads(C, ID)`` with its units:
    logsumexp_k t(AD@ID, DP@ID)[:, k] - t(row sums), t = s1 psi(s1) + s2 psi(s2) - ss psi(ss) with
    s1 = ad + pc, s2 = (dp - ad) + pc, ss = dp + 2 pc -> {"gain": (value, unit)} per variant.

    A term's unit: the rounding of its three products and the carry (|psi(s)| + s psi'(s)) u(s) of each
    shape (a float64 trigamma is plenty for a unit), u(s) the unit of the reads it is formed of and the
    rounding of forming it.  The logsumexp moves by at most its largest term's unit (d lse = sum_k p_k d t_k)
    and rounds its own sum, logarithm and result; the one-donor term has exact integer row sums."""
    reads = donor_reads(C, ID)
    (A, uA), (D, uD) = reads["AD_reads"], reads["DP_reads"]
    pc = LD(pseudocount)

    def term(ad, uad, dp, udp):
        bd = dp - ad
        s = (ad + pc, bd + pc, dp + 2 * pc)
        us = (uad + EPS * s[0], uad + udp + EPS * (np.abs(bd) + s[1]), udp + EPS * s[2])
        d = [psi(x) for x in s]
        tri = [ld(polygamma(1, np.asarray(x, dtype=np.float64))) for x in s]
        prod = [x * y for x, y in zip(s, d)]
        unit = EPS * sum(np.abs(x) for x in prod)
        unit = unit + sum((np.abs(y) + x * z) * u for x, y, z, u in zip(s, d, tri, us))
        return prod[0] + prod[1] - prod[2], unit

    T, uT = term(A, uA, D, uD)
    mx = T.max(axis=1)
    lse = mx + np.log(np.exp(T - mx[:, None]).sum(axis=1))
    ulse = uT.max(axis=1) + EPS * (np.abs(lse) + 1)
    zero = np.zeros(C.shape[0], dtype=LD)
    one, uone = term(np.asarray(C.AD.sum(axis=1)).ravel(), zero, np.asarray(C.DP.sum(axis=1)).ravel(), zero)
    gain = lse - one
    return {"gain": (gain, ulse + uone + EPS * np.abs(gain))}


# ------------------------------------------------------------------------------------
# the judge
# ------------------------------------------------------------------------------------
def distance(got, exact, unit):
    """max |got - exact| / unit over the elements; differences below TINY count as none
    (probabilities that underflow), a difference where the unit is 0 as infinite"""
    got, exact, unit = ld(got), ld(exact), ld(unit)
    if got.shape != exact.shape:
        raise ValueError("shape %s against %s" % (got.shape, exact.shape))
    if not np.all(np.isfinite(got)):
        return float("inf")
    d = np.abs(got - exact)
    live = d > TINY
    if not live.any():
        return 0.0
    with np.errstate(divide="ignore"):
        return float(np.max(d[live] / np.broadcast_to(unit, d.shape)[live]))


def bound(u_orc):
    """what a float64 implementation may be away from exact, given the float64 oracle's own
    distance on the same input: FACTOR x that, and never less than FACTOR roundings"""
    return FACTOR * max(u_orc, 1.0)


def held(u_dev, u_orc):
    return u_dev <= bound(u_orc)
