"""The steps outside the fit loop, shared by tests/test_exact_postfit_cpu.py (float64 NumPy in the
device's place) and tests/test_gpu_postfit_exact.py (the device): cases, the float64 side, the judge.

Four one-shot functions of explicit float64 or integer inputs: the doublet step
(``vrx_problem_doublet``), the cell log-likelihood against a caller's table
(``vrx_problem_cell_loglik``), the donor reads (``vrx_problem_donor_reads``) and the per-variant
mixtures (``vrx_varmix_fit`` at its shortest fit).  Data, states and priors are those of
tests/exact_cases.py; the exact side is tests/exact_np.py.  Every shape is the smallest at which the
path it names exists.
"""
import functools
from types import SimpleNamespace

import numpy as np
from scipy.special import digamma

from oracle import vireo_oracle as O
from tests import exact_cases as EC
from tests import exact_np as X
from tests import varmix_np as VN

LDS0, LDS1 = EC.LDS0, EC.LDS1
# one side shorter than a slab: no LDS-resident pass is built (as the size_* cases of exact_cases.py)
GATHER_ONLY = ("size_255x1", "size_1x63")


def _ns(table, name, **kw):
    assert name not in table
    table[name] = SimpleNamespace(name=name, **kw)


def lds_settings(data, n_col):
    """the VIREO_LDS settings a case runs under, with what ``DeviceModel.info()`` must then report:
    the LDS-resident passes take two columns or more and a tiled stream"""
    out = [("gather", LDS0, False)]
    if n_col >= 2 and data not in GATHER_ONLY:
        out.append(("lds", LDS1, True))
    return out


def distances(out, ex):
    return {k: X.distance(np.reshape(v, np.shape(ex[k][0])), *ex[k]) for k, v in out.items()}


def a_priori(C):
    return C.longest + 16


# ------------------------------------------------------------------------------------
# doublets
# ------------------------------------------------------------------------------------
def st_one_hot_gt(s, p, rng):    # a pair's normaliser is a single product
    g = rng.integers(0, p.T, (p.N, p.K))
    s.GT[:] = 0.0
    np.put_along_axis(s.GT, g[:, :, None], 1.0, axis=2)


DOUBLET = {}


def _d(name, data="small", K=4, T=3, ase=False, state=(), prior="uniform", rate=None):
    _ns(DOUBLET, name, data=data, K=K, T=T, ase=ase, state=tuple(state), prior=prior, rate=rate)


# K padding, the K > KP loop of the softmax, the widths of the command line (C = 136, 210)
for _K in (2, 3, 4, 5, 8, 11, 12, 16, 20, 23):
    _d("K%d" % _K, K=_K)
for _T in (1, 2, 3, 4, 5, 8):                       # G = 1 ... 36; T = 1 has no mixed class
    _d("T%d" % _T, T=_T)
_d("ase_T2", T=2, ase=True, state=[EC.st_random_theta])
_d("ase_T3", T=3, ase=True, state=[EC.st_random_theta])
_d("prior_none", prior=None)
for _rate, _tag in ((None, ""), (0.5, "_rate_half")):
    _d("prior_vector" + _tag, prior="vector", rate=_rate)
    _d("prior_cells" + _tag, prior="cells", rate=_rate)
for _data in ("ragged", "split", "size_255x1", "size_1x63", "size_257x65", "depth255", "depth_beyond",
              "one_beyond"):
    _d(_data, data=_data)
_d("many", data="many", K=6)                        # several contracted ranges
_d("tiny_gt", state=[EC.st_tiny_gt])                # the pair products underflow
_d("one_hot_gt", state=[st_one_hot_gt])
_d("sharp_gt_deep", data="deep", state=[EC.st_sharp_gt])     # logits that spread beyond exp's range
_d("edge_shapes", T=8, state=[EC.st_edge_b])        # the edge values as beta sums
_d("edge_shapes_a", T=8, state=[EC.st_edge_a])      # ... as the two shapes
_d("twin_classes", state=[EC.st_twins])             # classes 0 and 1 alike, class 2 1e-6 away
_d("cross_K3_T3", K=3, T=3)                         # (also through the explicit table: CROSS)
_d("cross_K4_T2", K=4, T=2)
CROSS = ("cross_K3_T3", "cross_K4_T2")


def doublet_theta(mu, sm):
    """add_doublet_theta and the three digamma tables exactly as predict_doublet forms them
    (vireo_amd/vireo_doublet.py): float64 inputs of device, oracle and exact side alike"""
    from vireo_amd.vireo_doublet import add_doublet_theta
    # (one class has no mixed class; the reference's helper, like ours, indexes an empty pair list there)
    mu2, sm2 = add_doublet_theta(mu, sm) if mu.shape[1] > 1 else (mu, sm)
    return (np.ascontiguousarray(digamma(sm2 * mu2)), np.ascontiguousarray(digamma(sm2 * (1 - mu2))),
            np.ascontiguousarray(digamma(sm2)))


def doublet_prior(ID_prior, n_pair, rate):
    """ID_prior_both of predict_doublet (vireo_doublet.py:45-50)"""
    return np.append(ID_prior * (1 - rate), np.ones((ID_prior.shape[0], n_pair)) / n_pair * rate, axis=1)


@functools.lru_cache(maxsize=2)
def doublet_problem(name):
    sp = DOUBLET[name]
    AD, DP = EC.data(sp.data)
    p = SimpleNamespace(spec=sp, AD=AD, DP=DP, N=AD.shape[0], M=AD.shape[1], K=sp.K, T=sp.T, kind="vireo")
    p.C = X.Counts(AD, DP)
    p.n_pair = p.K * (p.K - 1) // 2
    p.n_col = p.K + p.n_pair
    rng = np.random.default_rng(2000)
    rows = p.N if sp.ase else 1
    s = SimpleNamespace(GT=O.unit_sum(rng.random((p.N, p.K, p.T))),
                        mu=np.ones((rows, p.T)) * np.linspace(0.01, 0.99, p.T), sm=np.full((rows, p.T), 50.0))
    for f in sp.state:
        f(s, p, rng)
    p.GT = np.ascontiguousarray(s.GT)
    p.psi = doublet_theta(s.mu, s.sm)
    p.rate = min(0.5, p.M / 100000) if sp.rate is None else sp.rate
    if sp.prior is None:                            # no prior rows: uniform over all columns
        p.ID_prior = p.prior_both = None
    else:
        p.ID_prior = {"uniform": lambda: np.full((1, p.K), 1.0 / p.K),
                      "vector": lambda: EC.pr_id_vector(p, rng)["ID_prior"],
                      "cells": lambda: EC.pr_id_cells(p, rng)["ID_prior"]}[sp.prior]()
        p.prior_both = np.ascontiguousarray(doublet_prior(p.ID_prior, p.n_pair, p.rate))
    return p


def doublet_exact(p):
    if getattr(p, "_exact", None) is None:
        p._exact = X.doublet(p.C, p.GT, *p.psi, p.prior_both)
    return p._exact


def _posterior(L, prior):
    if prior is None:
        prior = np.full((1, L.shape[1]), 1.0 / L.shape[1])
    return O.softmax_log(L + np.log(prior))


def doublet_np(p):
    """the float64 side: the pieces of oracle.vireo_doublet on the case's tables"""
    if p.T > 1:
        GT2 = O.doublet_GT(p.GT)
    else:                                           # (no genotype pair to list: the same-class products alone)
        a, b = np.triu_indices(p.K, 1)
        GT2 = np.append(p.GT, O.unit_sum(p.GT[:, a, :] * p.GT[:, b, :]), axis=1)
    L = O._cell_loglik(GT2, *(x[:, None, :] for x in p.psi), p.AD, p.DP)
    return dict(logLik=L, prob=_posterior(L, p.prior_both))


# ------------------------------------------------------------------------------------
# cell_loglik: a caller's table
# ------------------------------------------------------------------------------------
CELL = {}
PRIOR_MODES = ("null", "none", "row", "cells")      # prob_out NULL; prob_out with 0, 1, n_cell prior rows
for _i, (_c, _g) in enumerate((c, g) for c in (1, 2, 5, 17, 70) for g in (1, 2, 3, 8)):
    # every n_col and every n_class meets both theta layouts and every prior form
    _ns(CELL, "c%d_g%d" % (_c, _g), n_col=_c, n_class=_g, psi_full=bool((_i + _i // 4) % 2),
        mode=PRIOR_MODES[(_i + _i // 4) % 4])


@functools.lru_cache(maxsize=2)
def cell_problem(name):
    sp = CELL[name]
    AD, DP = EC.data("small")
    p = SimpleNamespace(spec=sp, AD=AD, DP=DP, N=AD.shape[0], M=AD.shape[1], n_col=sp.n_col, n_class=sp.n_class)
    p.C = X.Counts(AD, DP)
    rng = np.random.default_rng(3000)
    rows = p.N if sp.psi_full else 1
    p.GT = O.unit_sum(rng.random((p.N, p.n_col, p.n_class)))
    s1, s2 = rng.uniform(0.3, 60.0, (rows, p.n_class)), rng.uniform(0.3, 60.0, (rows, p.n_class))
    p.psi = (digamma(s1), digamma(s2), digamma(s1 + s2))
    p.prior = {"null": None, "none": None, "row": (rng.random((1, p.n_col)) + 0.1) * 1.7,
               "cells": O.unit_sum(rng.random((p.M, p.n_col)) + 0.05)}[sp.mode]
    return p


def cell_exact(p):
    if getattr(p, "_exact", None) is None:
        p._exact = X.cell_loglik(p.C, p.GT, *p.psi, p.prior)
        if p.spec.mode == "null":
            del p._exact["prob"]
    return p._exact


def cell_np(p):
    L = O._cell_loglik(p.GT, *(x[:, None, :] for x in p.psi), p.AD, p.DP)
    out = dict(logLik=L)
    if p.spec.mode != "null":
        out["prob"] = _posterior(L, p.prior)
    return out


# ------------------------------------------------------------------------------------
# donor reads
# ------------------------------------------------------------------------------------
READS = {}
for _i, (_c, _data) in enumerate((c, d) for c in (1, 2, 5, 17, 70, 136)
                                 for d in ("small", "ragged", "split", "one_beyond")):
    # every n_col and every data set meets both states
    _ns(READS, "%s_c%d" % (_data, _c), data=_data, n_col=_c, one_hot=bool((_i + _i // 4) % 2))


@functools.lru_cache(maxsize=2)
def reads_problem(name):
    sp = READS[name]
    AD, DP = EC.data(sp.data)
    p = SimpleNamespace(spec=sp, AD=AD, DP=DP, N=AD.shape[0], M=AD.shape[1], n_col=sp.n_col)
    p.C = X.Counts(AD, DP)
    rng = np.random.default_rng(4000)
    if sp.one_hot:                                  # exact zeros and ones
        p.ID = np.zeros((p.M, p.n_col))
        p.ID[np.arange(p.M), rng.integers(0, p.n_col, p.M)] = 1.0
    else:
        p.ID = O.unit_sum(rng.random((p.M, p.n_col)))
    return p


def reads_exact(p):
    if getattr(p, "_exact", None) is None:
        p._exact = X.donor_reads(p.C, p.ID)
    return p._exact


def reads_np(p):
    return dict(AD_reads=p.AD @ p.ID, DP_reads=p.DP @ p.ID)


# ------------------------------------------------------------------------------------
# per-variant mixtures: max_iter = 2, min_iter = 5, the shortest fit the library accepts -- the stop
# rule never fires, every row runs iterations 0 and 1 and reports n_iter = 1, warn = 0
# ------------------------------------------------------------------------------------
VM_KS = (2, 3, 4, 5, 6, 7, 8)
VM_FIT = dict(max_iter=2, min_iter=5, epsilon_conv=1e-2)
VM_W = 512                       # vrx_varmix_wave_rows(): the GPU test asserts the library says the same
VM_LENGTHS = (0, 1, 2, 3, 63, 64, 65, 127, 128, 129, VM_W - 1, VM_W, VM_W + 1, 2 * VM_W - 1, 2 * VM_W,
              2 * VM_W + 1, 4 * VM_W + 3)
VM_OUTPUTS = ("trace[0]", "trace[1]", "beta_mu", "beta_sum", "size", "elbo_one")


@functools.lru_cache(maxsize=None)
def varmix_rows():
    """dense (AD, DP) and the group of every row: each length at depths 3, 20 and 60 (the odd last
    pair, the 128-entry wave chunk, wave against workgroup, the 512-entry workgroup pass), then the
    special rows"""
    n_cell = 4 * VM_W + 3
    AD, DP = VN.gen_rows([n for n in VM_LENGTHS for _ in VN.DEPTHS], seed=41, n_cell=n_cell)
    group = ["depth%d" % VN.DEPTHS[v % 3] for v in range(AD.shape[0])]
    rng = np.random.default_rng(42)
    n = 120
    d = rng.poisson(20, n) + 1
    deep = rng.poisson(1500, n) + 1
    big = d.copy()
    big[[5, 50, 99]] = (1000003, 999983, 1000211)   # elbo_one: terms of 1e7 that cancel
    special = [(np.zeros(n, dtype=np.int64), d),                     # all reference
               (d.copy(), d),                                         # all alternate
               (np.where(np.arange(n) % 3 == 0, deep, 0), deep),     # the middle component of K = 3 empties
               (np.where(np.arange(n) % 2 == 0, deep, 0), deep),
               (rng.binomial(big, np.where(np.arange(n) % 4 == 0, 0.4, 0.02)), big)]
    A2, D2 = np.zeros((len(special), n_cell), dtype=np.int64), np.zeros((len(special), n_cell), dtype=np.int64)
    for v, (a, dd) in enumerate(special):
        A2[v, :n], D2[v, :n] = a, dd
    return np.vstack([AD, A2]), np.vstack([DP, D2]), group + ["special"] * len(special)


def _covered(v):
    AD, DP, _ = varmix_rows()
    cov = DP[v] > 0
    return AD[v, cov], DP[v, cov]


@functools.lru_cache(maxsize=2)
def varmix_exact(K):
    """per row: name -> (value, unit)"""
    out = []
    for v in range(varmix_rows()[0].shape[0]):
        its, one = X.varmix_row(*_covered(v), K, 2)
        out.append({"trace[0]": its[0]["ELBO"], "trace[1]": its[1]["ELBO"], "beta_mu": its[1]["beta_mu"],
                    "beta_sum": its[1]["beta_sum"], "size": its[1]["size"], "elbo_one": one})
    return out


def varmix_np(K, fit_row=VN.fit_row):
    """the float64 side, per row: name -> value"""
    out = []
    for v in range(varmix_rows()[0].shape[0]):
        ad, dp = _covered(v)
        r = fit_row(ad, dp, K, **VM_FIT)
        assert r["n_iter"] == 1 and r["warn"] == 0 and r["elbo"] == r["trace"][0]
        out.append({"trace[0]": r["trace"][0], "trace[1]": r["trace"][1], "beta_mu": r["beta_mu"],
                    "beta_sum": r["beta_sum"], "size": r["size"], "elbo_one": VN.elbo_one(ad, dp)})
    return out


def varmix_row_distances(K, rows):
    """per row: output -> distance"""
    ex = varmix_exact(K)
    return [{k: X.distance(r[k], *ex[v][k]) for k in VM_OUTPUTS} for v, r in enumerate(rows)]


def varmix_distances(K, rows):
    """(group, output) -> the largest distance over the rows of the group, so that one lucky float64
    row does not set the bound"""
    group = varmix_rows()[2]
    out = {}
    for v, us in enumerate(varmix_row_distances(K, rows)):
        for k, u in us.items():
            out[(group[v], k)] = max(out.get((group[v], k), 0.0), u)
    return out


def varmix_a_priori(v):
    """the covered cells of row v in the longest contracted row's place"""
    return int((varmix_rows()[1][v] > 0).sum()) + 16


# ------------------------------------------------------------------------------------
# the judge
# ------------------------------------------------------------------------------------
def judge(rows, pinned, step, case, u_dev, u_orc):
    """assert the project's rule on every output of a case and keep the figures for the table"""
    bad = []
    for k in u_dev:
        limit = pinned.get((step, case, k), X.bound(u_orc[k]))
        rows.append((step, case, k, u_dev[k], u_orc[k], limit))
        print("%-8s %-28s %-10s device %9.3f  float64 %9.3f  bound %9.3f" % rows[-1])
        if not u_dev[k] <= limit:
            bad.append((k, u_dev[k], u_orc[k], limit))
    assert not bad, "%s %s: (output, device, float64, bound) %s" % (step, case, bad)
