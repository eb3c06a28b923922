"""The contract of vireo_amd.variant_mixture_gain in plain NumPy float64: BinomMixtureVB._fit_BV
(vireoSNP/utils/bmm_model.py:178-201) on ONE variant's 1 x n_cell row, over all cells (uncovered ones
included), from the deterministic start, with the full trace -- and the closed form of the one-component
bound.  tests/test_varmix_cpu.py proves it equal to oracle.vireo_oracle; the GPU tests compare the device
with it.  Also the row generator those tests share."""
import numpy as np
from scipy.special import betaln, digamma
from scipy.stats import entropy


def id_init(ad, dp, K):
    """w_k = max(0, 1 - |a/d - k/(K-1)| (K-1)) + 1/64, normalised; cells without reads get 1/K"""
    ad = np.asarray(ad, dtype=np.float64)
    dp = np.asarray(dp, dtype=np.float64)
    out = np.full((ad.size, K), 1.0 / K)
    cov = dp > 0
    f = ad[cov] / dp[cov]
    c = np.arange(K) / (K - 1)
    w = np.maximum(0.0, 1.0 - np.abs(f[:, None] - c[None, :]) * (K - 1)) + 1.0 / 64
    out[cov] = w / np.sum(w, axis=1, keepdims=True)
    return out


def _beta_kl_uniform(s1, s2):
    """sum_k KL(Beta(s1_k, s2_k) || Beta(1, 1)) in the term order of vireo_base.py:96-125"""
    d1, d2, ds = digamma(s1), digamma(s2), digamma(s1 + s2)
    q1 = np.ones_like(s1)
    cq = betaln(q1, q1) - (q1 - 1) * d1 - (q1 - 1) * d2 + ((q1 + q1) - 2) * ds
    cp = betaln(s1, s2) - (s1 - 1) * d1 - (s2 - 1) * d2 + ((s1 + s2) - 2) * ds
    return np.sum(cq - cp)


def fit_row(ad, dp, K, max_iter=200, min_iter=20, epsilon_conv=1e-2, start=None):
    """One variant.  -> dict(trace = ELBO[0 .. it], n_iter = it, warn, elbo = ELBO[it - 1], beta_mu, beta_sum,
    size (covered cells only), ID_prob, margins = the tested differences ELBO[j] - ELBO[j - 1])"""
    ad = np.asarray(ad, dtype=np.float64)
    dp = np.asarray(dp, dtype=np.float64)
    bd = dp - ad
    n_cell = ad.size
    ID = id_init(ad, dp, K) if start is None else np.array(start, dtype=np.float64)
    ID = ID / np.sum(ID, axis=1, keepdims=True)               # set_initial normalises what it is given (:80-81)
    prior = np.full((n_cell, K), 1.0) / np.sum(np.full((n_cell, K), 1.0), axis=1, keepdims=True)
    trace = np.zeros(max_iter)
    warn = 0
    margins = []
    it = 0
    for it in range(max_iter):
        t1 = ad[None, :] @ ID + 1.0                            # update_theta_size (:133-144)
        t2 = bd[None, :] @ ID + 1.0
        mu = t1 / (t1 + t2)
        sm = t1 + t2
        s1, s2 = mu * sm, (1 - mu) * sm                        # the theta_s1 / theta_s2 properties (:107-115)
        L = ad[:, None] @ digamma(s1) + bd[:, None] @ digamma(s2) - dp[:, None] @ digamma(s1 + s2)
        X = L + np.log(prior)                                  # update_ID_prob (:147-154)
        X = X - np.max(X, axis=1, keepdims=True)
        ID = np.exp(X)
        ID = ID / np.sum(ID, axis=1, keepdims=True)
        trace[it] = np.sum(L * ID) - np.sum(entropy(ID, prior, axis=-1)) - _beta_kl_uniform(s1, s2)
        if it > min_iter:
            diff = trace[it] - trace[it - 1]
            margins.append(diff)
            if diff < -1e-6:
                warn |= 1
            elif it == max_iter - 1:
                warn |= 2
            elif diff < epsilon_conv:
                break
    cov = dp > 0
    return dict(trace=trace[:it + 1].copy(), n_iter=it, warn=warn, elbo=trace[it - 1], beta_mu=mu[0], beta_sum=sm[0],
                size=np.sum(ID[cov], axis=0), ID_prob=ID, margins=np.array(margins))


def elbo_one(ad, dp):
    """the bound _fit_BV records (at every iteration) with n_donor = 1, where ID = 1"""
    ad = np.asarray(ad, dtype=np.float64)
    dp = np.asarray(dp, dtype=np.float64)
    bd = dp - ad
    t1, t2 = np.sum(ad) + 1.0, np.sum(bd) + 1.0
    mu, sm = t1 / (t1 + t2), t1 + t2
    s1, s2 = np.array([mu * sm]), np.array([(1 - mu) * sm])
    L = ad * digamma(s1) + bd * digamma(s2) - dp * digamma(s1 + s2)
    return np.sum(L) - _beta_kl_uniform(s1, s2)


def knife_edge(margins, epsilon_conv, cap=1e-9):
    """some tested difference lies within `cap` of a threshold of the stop rule"""
    m = np.asarray(margins)
    return bool(m.size and (np.min(np.abs(m - epsilon_conv)) < cap or np.min(np.abs(m + 1e-6)) < cap))


N_CELL = 300
DEPTHS = (3, 20, 60)
FLAT_RATES = (0.0, 0.05, 0.5, 1.0)


def gen_rows(lengths, seed, n_cell=None):
    """Dense (AD, DP) int64 matrices, one row per entry of `lengths` (its number of covered cells).  Depth
    is Poisson(3 | 20 | 60) + 1 per row; the allele rate is a planted two-level mix or one level of
    {0, 0.05, 0.5, 1}, in turn."""
    rng = np.random.default_rng(seed)
    n_cell = max(N_CELL, max(lengths) if len(lengths) else 0) if n_cell is None else n_cell
    AD = np.zeros((len(lengths), n_cell), dtype=np.int64)
    DP = np.zeros((len(lengths), n_cell), dtype=np.int64)
    for v, n in enumerate(lengths):
        cells = np.sort(rng.choice(n_cell, n, replace=False))
        d = rng.poisson(DEPTHS[v % 3], n) + 1
        kind = (v // 3) % 5
        if kind == 0:                                     # a clone: two levels
            lo, hi = rng.uniform(0.0, 0.1), rng.uniform(0.25, 0.9)
            p = np.where(rng.random(n) < rng.uniform(0.2, 0.5), hi, lo)
        else:
            p = np.full(n, FLAT_RATES[kind - 1])
        DP[v, cells] = d
        AD[v, cells] = rng.binomial(d, p)
    return AD, DP
