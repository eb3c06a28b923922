"""The ambient-RNA step one update at a time, shared by tests/test_exact_ambient_cpu.py (float64 NumPy in the
device's place) and tests/test_gpu_ambient_exact.py (the device): the helpers that call
``vrx_problem_ambient`` (also used by tests/test_gpu_postfit_sweep.py), the cases, the float64 side, a
float64 copy of the device's schedule, the judge.  TEST INFRASTRUCTURE ONLY; imports without a GPU.

``vrx_problem_ambient`` with ``min_iter = max_iter = n`` and ``epsilon = 0`` never meets ``it > min_iter``:
every counted cell runs exactly n updates and leaves at ``it = n - 1`` with psi after n updates, the variance
at that psi and ``llr = L(psi after n - 1 updates) - L0``.  n = 2 is the shortest run the entry point takes.
The exact side is tests/exact_np.py (``ambient_cell``, ``elbo_gain``), the float64 side tests/ambient_np.py
(``fit_cell`` at the same forced length, ``elbo_gain``).  A case's distance is the largest over its counted
cells (its variants), the device's and float64's alike, so that one lucky float64 cell does not set the bound.
"""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
from scipy.sparse import csc_matrix

from tests import ambient_np as A
from tests import exact_np as X
from tests.exact_postfit import judge

DEFAULT_BUDGET = 16384          # VIREO_AMBIENT_LDS when it is not set
LDS_MAX = 64 * 1024


# ------------------------------------------------------------------------------------
# calling the library (moved here from tests/test_gpu_postfit_sweep.py, unchanged)
# ------------------------------------------------------------------------------------
def amb_lds_bytes(K, cap):
    """vrx_amb_lds_bytes (vrx_ambient.h): psi[K] | r[K] | w1[64] | w0[64] | cap theta rows of stride K | 1
    doubles, then 64 row numbers"""
    return (2 * K + 128 + cap * (K | 1)) * 8 + 64 * 4


def amb_cap(K, budget):
    """the most entries whose theta rows a cell keeps in LDS under VIREO_AMBIENT_LDS = budget"""
    fixed = amb_lds_bytes(K, 0)
    return (budget - fixed) // ((K | 1) * 8) if budget > fixed else 0


def run_ambient(counts, K, theta, sel, psi0, min_iter, max_iter, eps):
    from vireo_amd import _lib
    from vireo_amd._lib import dptr, f64
    M = counts.n_cell
    theta, psi0 = f64(theta), f64(psi0)
    assert theta.shape == (counts.n_var, K) and psi0.shape == (M, K)
    psi, var = np.full((M, K), -7.0), np.full((M, K), -7.0)
    llr, n_iter = np.full(M, -7.0), np.full(M, -7, np.int32)
    mask = np.ascontiguousarray(sel, dtype=np.uint8)
    _lib.check(_lib.lib().vrx_problem_ambient(
        counts.handle, K, dptr(theta), mask.ctypes.data_as(C.POINTER(C.c_uint8)), dptr(psi0), min_iter, max_iter,
        eps, dptr(psi), dptr(var), dptr(llr), n_iter.ctypes.data_as(C.POINTER(C.c_int32)), None))
    return psi, var, llr, n_iter


def built_ambient_problem(seed, K, targets, n_background, bg_max, top, empty_selection=False):
    """(N x M) counts in merged CSC form: cell i < len(targets) has exactly targets[i] entries on selected
    variants (and a few on others), then `n_background` cells with 0 .. bg_max entries anywhere.
    -> shape, colptr, rowidx, ad, dp, sel, theta, psi0"""
    rng = np.random.default_rng(7000 + seed)
    N = 640
    sel = rng.random(N) < 0.55
    sel[:max(max(targets, default=0), bg_max) + 8] = True         # (enough selected variants for every target)
    rng.shuffle(sel)
    on, off = np.flatnonzero(sel), np.flatnonzero(~sel)
    GT = rng.dirichlet(np.ones(3) * 0.3, (N, K))
    theta = np.tensordot(GT, np.array([0.01, 0.5, 0.99]), axes=(2, 0))
    cols = []
    for n in targets:
        rows = np.concatenate([rng.choice(on, n, replace=False),
                               rng.choice(off, int(rng.integers(0, min(30, off.size))), replace=False)])
        cols.append(np.sort(rows))
    for _ in range(n_background):
        cols.append(np.sort(rng.choice(N, int(rng.integers(0, bg_max + 1)), replace=False)))
    M = len(cols)
    colptr = np.concatenate([[0], np.cumsum([c.size for c in cols])]).astype(np.int64)
    rowidx = np.concatenate(cols).astype(np.int32) if colptr[-1] else np.zeros(0, np.int32)
    dp = rng.integers(1, top + 1, rowidx.size).astype(np.int32)
    donor = np.repeat(rng.integers(0, K, M), np.diff(colptr))
    ad = rng.binomial(dp, theta[rowidx, donor]).astype(np.int32)
    if empty_selection:
        sel = np.zeros(N, bool)
    psi0 = rng.dirichlet(np.ones(K), M)
    return (N, M), colptr, rowidx, ad, dp, sel, theta, psi0


def id_prob(rng, M, K, kind):
    soft = rng.dirichlet(np.ones(K) * 0.5, M) if K > 1 else rng.random((M, 1))
    if kind == "random":
        return soft
    if kind == "zeros":              # exact zeros: a donor nobody is assigned to, cells without a donor
        soft[:, rng.integers(K)] = 0.0
        soft[rng.random(M) < 0.1] = 0.0
        return soft
    ID = np.zeros((M, K))            # exact zeros and ones, rows within 1e-9 of one-hot, a few soft ones
    ID[np.arange(M), rng.integers(0, K, M)] = 1.0
    near = rng.random(M) < 0.2
    if K > 1:
        ID[near] = ID[near] * (1 - 1e-9) + (1 - ID[near]) * 1e-9 / (K - 1)
    some = rng.random(M) < 0.1
    ID[some] = soft[some]
    return ID


def library_plan(K):
    """(cap, LDS bytes per cell) of ``vrx_problem_ambient`` at K donors under the environment as it is:
    ``vrx_ambient_info``, the library's own arithmetic (no device needed)"""
    from vireo_amd import _lib
    cap, lds = C.c_int32(-1), C.c_int64(-1)
    _lib.check(_lib.lib().vrx_ambient_info(K, C.byref(cap), C.byref(lds)))
    return int(cap.value), int(lds.value)


def same_bits(x, y):
    """bitwise, any NaN equal to any NaN (the sweep's comparison between routes)"""
    x, y = np.asarray(x), np.asarray(y)
    return x.shape == y.shape and np.array_equal(x, y, equal_nan=True) and \
        np.array_equal(np.signbit(x), np.signbit(y))


# ------------------------------------------------------------------------------------
# edits of a built problem (p: its arrays, writable)
# ------------------------------------------------------------------------------------
def ed_deep(p, rng):               # 1e6 reads beside 1
    i = np.arange(p.dp.size)
    deep, one = i % 7 == 0, i % 7 == 1
    p.dp[deep] = 1000003 - i[deep] % 5
    p.ad[deep] = rng.binomial(p.dp[deep], 0.3)
    p.dp[one] = 1
    p.ad[one] = i[one] % 2


def ed_zero_psi(p, rng):           # must stay exactly 0
    p.psi0[:, 1] = 0.0
    p.psi0 /= p.psi0.sum(axis=1, keepdims=True)


def ed_tiny_psi(p, rng):           # must stay finite and non-zero
    p.psi0[:, 1] = 1e-300


def ed_near_one_psi(p, rng):
    p.psi0[:] = 1e-12 / (p.K - 1)
    p.psi0[:, 0] = 1 - 1e-12


def ed_edge_theta(p, rng):         # t1 reaches 1e-9 and 1 - 1e-9 where a row has every donor there
    p.theta[:] = rng.choice([1e-9, 0.5, 1 - 1e-9], p.theta.shape)


def ed_same_theta(p, rng):         # r_k alike for all k: psi moves by roundings only, llr is a pure cancellation
    p.theta[:] = p.theta[:, :1]


def ed_alt_ref(p, rng):            # constructed cells of all-alternative and of all-reference reads; a = 0, b > 0 elsewhere
    cell = np.repeat(np.arange(p.M), np.diff(p.colptr))
    p.ad[cell % 3 == 0] = p.dp[cell % 3 == 0]
    p.ad[cell % 3 == 1] = 0
    rest = (cell % 3 == 2) & (np.arange(p.dp.size) % 4 == 0)
    p.ad[rest] = 0


def ed_last_read(p, rng):          # every entry of 5 000 reads, the last selected entry of each cell of one
    p.dp[:] = 5000
    p.ad[:] = rng.binomial(5000, 0.4, p.dp.size)
    for c in range(p.M):
        on = np.flatnonzero(p.sel[p.rowidx[p.colptr[c]:p.colptr[c + 1]]])
        if on.size:
            e = p.colptr[c] + on[-1]
            p.dp[e], p.ad[e] = 1, 0


def ed_close_theta(p, rng):        # theta rows 1e-7 apart
    p.theta[:] = 0.2 + 0.6 * rng.random(p.K)[None, :] + 1e-7 * np.arange(p.theta.shape[0])[:, None]


def ed_small_last_psi(p, rng):     # the last donor at 1e-9
    p.psi0[:, -1] = 0.0
    p.psi0 *= (1 - 1e-9) / p.psi0.sum(axis=1, keepdims=True)
    p.psi0[:, -1] = 1e-9


EDITS = {f.__name__[3:]: f for f in (ed_deep, ed_zero_psi, ed_tiny_psi, ed_near_one_psi, ed_edge_theta, ed_same_theta,
                                     ed_alt_ref, ed_last_read, ed_close_theta, ed_small_last_psi)}


# ------------------------------------------------------------------------------------
# the EM cases: name -> K, selected entries per constructed cell, small cap (cells of cap - 1, cap, cap + 1
# entries are added; None: no such budget), VIREO_ENTRY_FMT, largest count, an edit, the forced lengths
# ------------------------------------------------------------------------------------
EM = {}
CHUNKS = (1, 2, 63, 64, 65, 127, 128, 129)       # around the 64-entry chunks of vrx_amb_pass, two chunks and more
HUGE_EPS = (5, 30, 1e9)                          # the sweep's rule: every counted cell leaves at it = 6


def _e(name, kind, K, targets, cap, fmt, top, edit=None, lengths=(2,), seed=None):
    assert name not in EM
    EM[name] = SimpleNamespace(name=name, kind=kind, K=K, targets=tuple(targets), cap=cap, fmt=fmt, top=top,
                               edit=edit, lengths=tuple(lengths), seed=100 + len(EM) if seed is None else seed)


# ---- max_iter = 2: K over the second trip of the lane-strided loops (k = lane, lane + 64, ...), every chunk edge
_e("K1", "em", 1, CHUNKS, None, 0, 40)
_e("K2", "em", 2, CHUNKS, 64, 1, 300)            # cap edges = chunk edges
_e("K3", "em", 3, CHUNKS, 10, 2, 5000)
_e("K8", "em", 8, CHUNKS, 1, 0, 40)              # cap 1: cells of 0 (NaN), 1, 2 entries
_e("K16", "em", 16, CHUNKS, 20, 1, 5000)
_e("K33", "em", 33, CHUNKS, 128, 2, 300)
_e("K63", "em", 63, CHUNKS, 5, 0, 40)
_e("K64", "em", 64, CHUNKS, None, 1, 300)
_e("K65", "em", 65, CHUNKS, 10, 2, 5000)
_e("K130", "em", 130, CHUNKS, 3, 0, 40)          # more entries than any budget caches
_e("deep_K5", "em", 5, (1, 2, 65, 129), 10, 2, 40, "deep")
# ---- edge states
_e("zero_psi", "em", 5, (1, 64, 65), 10, 0, 40, "zero_psi")
_e("tiny_psi", "em", 5, (1, 64, 65), 10, 1, 300, "tiny_psi")
_e("near_one_psi", "em", 5, (1, 64, 65), 10, 0, 40, "near_one_psi")
_e("edge_theta_K2", "em", 2, (1, 2, 64, 65, 129), 10, 0, 40, "edge_theta")
_e("edge_theta_K5", "em", 5, (1, 64, 65), 10, 1, 300, "edge_theta")
_e("same_theta", "em", 8, (1, 64, 65, 129), 10, 0, 40, "same_theta")
_e("alt_ref", "em", 5, (1, 2, 3, 64, 65, 66, 129, 128, 127), 10, 1, 300, "alt_ref")
_e("one_entry_K130", "em", 130, (1, 1, 1), 3, 0, 40)
_e("argmax_change", "em", 4, (3, 4, 5, 6, 8, 10, 12, 16) * 6, 5, 0, 40)        # (problem() lists the cells: p.flip)
# ---- what the defects of tests/test_exact_ambient_cpu.py are written for
_e("teeth_last_read", "em", 3, (65, 65, 65), 10, 1, 5000, "last_read")
_e("teeth_close_theta", "em", 5, (65, 100, 129), 10, 0, 40, "close_theta")
_e("teeth_r64", "em", 65, (3, 40, 65), 10, 0, 40, "small_last_psi")
# ---- longer forced runs, chains from a state read back, the stop rule against the forced length
_e("long_small", "long", 3, (1, 2, 63, 64, 65, 129), 10, 0, 40, lengths=(3, 4, 7))
_e("long_K65", "long", 65, (1, 63, 64, 65, 129), 10, 1, 300, lengths=(3, 4, 7))
_e("long_K130", "long", 130, (1, 64, 65, 129), 10, 2, 5000, lengths=(3, 4, 7))

N_BACKGROUND, BG_MAX = 4, 40


@functools.lru_cache(maxsize=4)
def problem(name):
    sp = EM[name]
    targets = list(sp.targets) + ([sp.cap - 1, sp.cap, sp.cap + 1] if sp.cap is not None else [])
    shape, colptr, rowidx, ad, dp, sel, theta, psi0 = built_ambient_problem(
        sp.seed, sp.K, targets, n_background=N_BACKGROUND, bg_max=BG_MAX, top=sp.top)
    p = SimpleNamespace(spec=sp, name=name, K=sp.K, shape=shape, N=shape[0], M=shape[1], colptr=colptr, rowidx=rowidx,
                        ad=ad.copy(), dp=dp.copy(), sel=sel, theta=theta.copy(), psi0=psi0.copy(), targets=targets)
    if sp.edit:
        EDITS[sp.edit](p, np.random.default_rng(sp.seed + 1))
    assert np.all(p.ad >= 0) and np.all(p.ad <= p.dp)
    p.AD = csc_matrix((p.ad, rowidx, colptr), shape=shape)
    p.DP = csc_matrix((p.dp, rowidx, colptr), shape=shape)
    # per cell: the counts of its selected entries and their theta rows, in variant order (the device's order)
    p.cells = []
    for c in range(p.M):
        rows, a, b = A.cell_entries(p.AD, p.DP, sel, c)
        p.cells.append((a.astype(np.float64), b.astype(np.float64), np.ascontiguousarray(p.theta[rows])))
    p.n_sel = np.array([a.size for a, _, _ in p.cells])
    p.counted = np.array([a.sum() + b.sum() > 0 for a, b, _ in p.cells])
    # the budgets: default, global, all cached where that fits 64 KiB, the small cap
    p.routes = [("default", None), ("global", 0)]
    every = amb_lds_bytes(sp.K, int(p.n_sel.max()))
    if every <= LDS_MAX:
        p.routes.append(("all_cached", every))
    if sp.cap is not None:
        p.routes.append(("cap_%d" % sp.cap, amb_lds_bytes(sp.K, sp.cap)))
    if name == "argmax_change":
        p.flip = argmax_changes(p)
    for arr in (p.ad, p.dp, p.theta, p.psi0):
        arr.setflags(write=False)
    return p


def route_cap(K, budget):
    """the Python copy of the library's cap under a budget (None: the variable is not set)"""
    return amb_cap(K, DEFAULT_BUDGET if budget is None else budget)


def argmax_changes(p):
    """the cells whose largest component after one update is another than after two (float64 restatement)"""
    out = []
    for c, (a, b, th) in enumerate(p.cells):
        if a.size == 0:
            continue
        p1 = A.fit_cell(a, b, th, p.psi0[c], min_iter=1, max_iter=1, eps=0.0)[0]
        p2 = A.fit_cell(a, b, th, p.psi0[c], min_iter=2, max_iter=2, eps=0.0)[0]
        if np.argmax(p1) != np.argmax(p2) and min(top_gap(p1), top_gap(p2)) >= 1e-6:
            out.append(c)
    return out


def top_gap(psi):
    """relative gap between the two largest components (inf for one component)"""
    if len(psi) < 2:
        return np.inf
    s = np.sort(np.asarray(psi, dtype=np.float64))
    return (s[-1] - s[-2]) / s[-1]


# ------------------------------------------------------------------------------------
# the sides: what a case asks of the implementation under test
# ------------------------------------------------------------------------------------
class Float64Side:
    """tests/ambient_np.py in the device's place (the route changes nothing)"""

    def run(self, p, psi0, n, budget):
        """-> psi (M, K), var (M, K), llr (M,), n_iter (M,) of n forced updates"""
        return self.fit(p, psi0, (n, n, 0.0), budget)

    def fit(self, p, psi0, rule, budget):
        out = [A.fit_cell(a, b, th, psi0[c], min_iter=rule[0], max_iter=rule[1], eps=rule[2])
               for c, (a, b, th) in enumerate(p.cells)]
        return (np.array([o[0] for o in out]), np.array([o[1] for o in out]), np.array([o[2] for o in out]),
                np.array([o[3] for o in out]))

    def caps(self, p):
        """route -> the cap it runs under"""
        return {name: route_cap(p.K, budget) for name, budget in p.routes}

    def gain(self, g, lds):
        return A.elbo_gain(g.ID, g.AD, g.DP, pseudocount=g.pc)


ORACLE = Float64Side()


# ---- a float64 copy of the device's schedule (csrc/vrx_ambient.h), for the CPU harness
def _fma(x, y, z):
    """fma in float64 through long double (the product of two doubles needs 106 bits, 64 are kept: one
    rounding more than the instruction in rare cases, which the copy does not depend on)"""
    return np.asarray(X.ld(x) * X.ld(y) + X.ld(z), dtype=np.float64)


def _butterfly(v):
    """v += shfl_xor(v, o), o = 32 .. 1, on 64 lanes"""
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[lane ^ o]
    return v[0]


def _copy_pass(a, b, th, psi, r, mode, kmax, cached, wrong):
    """vrx_amb_pass: 64 entries at a time (the fma chains of t1 and t0 over the donors, the log-likelihood terms
    per lane, the two weights), then r_k over the chunk's entries in order.  r comes in as the pass before left it
    and is zeroed here.  -> log-likelihood (butterfly over the lanes), r"""
    n, K = th.shape
    r = r.copy()
    keep = 64 if (wrong == "r64_stale" and K > 64) else K
    r[:keep] = 0.0
    ll = np.zeros(64)
    with np.errstate(all="ignore"):
        for base in range(0, n, 64):
            m = min(64, n - base)
            e = slice(base, base + m)
            t1, t0 = np.zeros(m), np.zeros(m)
            for k in range(K):
                t1 = _fma(th[e, k], psi[k], t1)
                t0 = _fma(1.0 - th[e, k], psi[k], t0)
            if mode == 0:
                ll[:m] += a[e] * np.log(t1) + b[e] * np.log(1.0 - t1)
                w1, w0 = a[e] / t1, b[e] / t0
            else:
                tm = th[e, kmax]
                ll[:m] += a[e] * np.log(tm) + b[e] * np.log(1.0 - tm)
                f0 = b[e] / ((1.0 - t1) * (1.0 - t1))
                if wrong == "fisher_b" and base + m == n:
                    f0[-1] = 0.0                         # the b / (1 - t1)^2 term of the last entry
                w1, w0 = a[e] / (t1 * t1) + f0, None
            rows = th[e]
            if wrong == "stale_rows" and not cached and base > 0 and base + m == n:
                rows = th[base - 64:base - 64 + m]      # the row numbers of the chunk before
            walk = list(range(m))
            if wrong == "skip_last" and base + m == n and mode == 0:
                walk = walk[:-1]
            if wrong == "twice_64" and base == 0 and n > 64 and mode == 0:
                t64 = _t(th[64], psi)                    # (entry 64 walked once more, behind entry 63)
                rows, w1, w0 = np.vstack([rows, th[64:65]]), np.append(w1, a[64] / t64[0]), np.append(w0, b[64] / t64[1])
                walk.append(m)
            acc = r
            for j in walk:
                if mode == 0:
                    acc = _fma(rows[j], w1[j], acc)
                    acc = _fma(1.0 - rows[j], w0[j], acc)
                else:
                    acc = _fma(rows[j] * rows[j], w1[j], acc)
            r = acc
    return _butterfly(ll), r


def _t(row, psi):
    t1 = t0 = np.float64(0.0)
    for k in range(len(psi)):
        t1 = _fma(row[k], psi[k], t1)
        t0 = _fma(1.0 - row[k], psi[k], t0)
    return float(t1), float(t0)


def copy_cell(a, b, th, psi0, n_updates, cached=True, wrong=None):
    """vrx_amb_em for one cell at a forced length, in float64 on the device's schedule -> psi, var, llr.
    ``wrong`` names one defect:
      skip_last    the last entry of the cell left out of r
      twice_64     entry 64 added twice, at the end of the first chunk and at the start of the second
      stale_rows   the last chunk of an uncached cell reads the theta rows of the chunk before
      r64_stale    r_k, k >= 64, not zeroed before a pass (it keeps the sum of the pass before)
      fisher_b     the b / (1 - t1)^2 term of the last entry dropped from the Fisher sum
      old_argmax   L0 taken at the first maximum of the psi before the last update"""
    K = th.shape[1]
    if a.sum() + b.sum() == 0:
        return np.full(K, np.nan), np.full(K, np.nan), np.nan
    psi, r = np.array(psi0, dtype=np.float64), np.zeros(K)
    ll_prev, before = 0.0, psi
    for p in range(n_updates + 1):
        ll, r = _copy_pass(a, b, th, psi, r, 0, 0, cached, wrong)
        if p == n_updates:
            break
        ll_prev = ll
        tot = 0.0
        for k in range(K):                             # the M step's sum, in index order
            tot += psi[k] * r[k]
        before, psi = psi, psi * r / tot
    kmax = int(np.argmax(before if wrong == "old_argmax" else psi))
    ll0, r = _copy_pass(a, b, th, psi, r, 1, kmax, cached, wrong)
    with np.errstate(all="ignore"):
        return psi, 1.0 / r, ll_prev - ll0


class CopySide(Float64Side):
    def __init__(self, wrong=None):
        self.wrong = wrong

    def run(self, p, psi0, n, budget):
        cap = route_cap(p.K, budget)
        out = [copy_cell(a, b, th, psi0[c], n, cached=a.size <= cap, wrong=self.wrong)
               for c, (a, b, th) in enumerate(p.cells)]
        return (np.array([o[0] for o in out]), np.array([o[1] for o in out]), np.array([o[2] for o in out]),
                np.full(p.M, n - 1))

    def fit(self, p, psi0, rule, budget):
        raise NotImplementedError("the copy runs forced lengths only")

    def gain(self, g, lds, switch=10.0, drop_smallest=False):
        """vrx_amb_gain on float64 sums: the series digamma with its recurrence up to ``switch``, the
        logsumexp in two passes (largest term, then the sum in donor order)"""
        from tests.test_exact_cpu import series_digamma
        pc = g.pc

        def term(ad, dp):
            s1, s2, ss = ad + pc, (dp - ad) + pc, dp + 2.0 * pc
            return s1 * series_digamma(s1, switch) + s2 * series_digamma(s2, switch) - ss * series_digamma(ss, switch)

        T = term(np.asarray(g.AD @ g.ID), np.asarray(g.DP @ g.ID))
        mx = T.max(axis=1)
        E = np.exp(T - mx[:, None])
        if drop_smallest:
            E[np.arange(T.shape[0]), T.argmin(axis=1)] = 0.0
        tot = np.zeros(T.shape[0])
        for k in range(T.shape[1]):
            tot += E[:, k]
        return (np.log(tot) + mx) - term(np.asarray(g.AD.sum(1)).ravel().astype(np.float64),
                                         np.asarray(g.DP.sum(1)).ravel().astype(np.float64))


# ------------------------------------------------------------------------------------
# exact values, distances
# ------------------------------------------------------------------------------------
OUTPUTS = ("psi", "var", "llr")


def exact_cells(p, psi0, n):
    """per cell: name -> (value, unit) of n forced updates from psi0"""
    return [X.ambient_cell(a, b, th, psi0[c], n) for c, (a, b, th) in enumerate(p.cells)]


@functools.lru_cache(maxsize=8)
def exact_from_start(name, n):
    p = problem(name)
    return exact_cells(p, p.psi0, n)


def cell_distances(p, got, ex):
    """per counted cell: output -> distance; the NaN pattern compared exactly on every cell"""
    psi, var, llr = got[:3]
    out = {}
    for c in range(p.M):
        e = ex[c]
        if not p.counted[c]:
            assert np.all(np.isnan(psi[c])) and np.all(np.isnan(var[c])) and np.isnan(llr[c]), (p.name, c)
            assert np.all(np.isnan(np.asarray(e["psi"][0], dtype=np.float64))) and np.isnan(float(e["llr"][0]))
            continue
        assert not (np.isnan(psi[c]).any() or np.isnan(var[c]).any() or np.isnan(llr[c])), (p.name, c)
        out[c] = {"psi": X.distance(psi[c], *e["psi"]), "var": X.distance(var[c], *e["var"]),
                  "llr": X.distance(llr[c], *e["llr"])}
    return out


def worst(per_cell):
    return {k: max((u[k] for u in per_cell.values()), default=0.0) for k in OUTPUTS}


def a_priori(p, c):
    """the cell's entries + K + 16"""
    return int(p.n_sel[c]) + p.K + 16


def _check_values(p, psi0, psi):
    ok = p.counted
    assert np.all(np.isfinite(psi[ok])), p.name
    if p.spec.edit == "zero_psi":
        assert np.all(psi0[:, 1] == 0.0) and np.all(psi[ok, 1] == 0.0) and not np.signbit(psi[ok, 1]).any()
    if p.spec.edit == "tiny_psi":
        assert np.all(psi[ok, 1] > 0.0) and np.all(psi[ok, 1] < 1e-250)


def run_routes(p, side, psi0, n):
    """n forced updates on every route: n_iter = n - 1 on every cell (the NaN cells too), all routes the same bits
    -> the default route's results"""
    res = {name: side.run(p, psi0, n, budget) for name, budget in p.routes}
    first = res["default"]
    for name, got in res.items():
        assert np.array_equal(got[3], np.full(p.M, n - 1)), (p.name, name, got[3])
        for x, y, what in zip(got[:3], first[:3], OUTPUTS):
            assert same_bits(x, y), (p.name, name, what)
    return first


def check_routes(p, side):
    """which route each constructed cell takes under each budget, with the cap the side reports (the device's:
    ``vrx_ambient_info`` under that environment) -- and the Python copy of that arithmetic agrees"""
    caps = side.caps(p)
    n = p.n_sel[:len(p.targets)]
    assert list(n) == list(p.targets), (p.name, list(n))
    for name, budget in p.routes:
        cap = caps[name]
        assert cap == route_cap(p.K, budget), (p.name, name, cap)
        assert amb_lds_bytes(p.K, cap) <= LDS_MAX
        cached = n <= cap
        if name == "global":
            assert cap == 0 and not cached[n > 0].any()
        elif name == "all_cached":
            assert cap == p.n_sel.max() and cached.all()
        elif name.startswith("cap_"):
            assert cap == p.spec.cap and list(n[-3:]) == [cap - 1, cap, cap + 1] and list(cached[-3:]) == [True, True, False]
            assert cached.any() and not cached.all()
        else:
            assert cap == amb_cap(p.K, DEFAULT_BUDGET)
            assert cached.all() == (n.max() <= cap)   # (K = 130 caches 12 entries, K = 1 all of these)


def judge_run(p, side, rows, pinned, step, label, psi0, n, got, ex=None):
    ex = exact_cells(p, psi0, n) if ex is None else ex
    _check_values(p, psi0, got[0])
    u_dev = worst(cell_distances(p, got, ex))
    u_orc = worst(cell_distances(p, ORACLE.run(p, psi0, n, None), ex))
    judge(rows, pinned, step, label, u_dev, u_orc)


def run_em(p, side, rows, pinned):
    """the forced lengths of the case, each from the case's start, on every route"""
    check_routes(p, side)
    for n in p.spec.lengths:
        got = run_routes(p, side, p.psi0, n)
        label = p.name if len(p.spec.lengths) == 1 else "%s n=%d" % (p.name, n)
        judge_run(p, side, rows, pinned, p.spec.kind, label, p.psi0, n, got, exact_from_start(p.name, n))


def run_long(p, side, rows, pinned):
    """3, 4 and 7 forced updates from the start; two legs of 2 against one run of 4; the sweep's stop rule
    (5, 30, 1e9) against 7 forced updates"""
    run_em(p, side, rows, pinned)
    leg1 = run_routes(p, side, p.psi0, 2)
    leg2 = run_routes(p, side, leg1[0], 2)               # from the float64 state read back
    whole = run_routes(p, side, p.psi0, 4)
    for x, y, what in zip(leg2[:3], whole[:3], OUTPUTS):
        assert same_bits(x, y), (p.name, "chain", what)
    judge_run(p, side, rows, pinned, "chain", "%s leg 1" % p.name, p.psi0, 2, leg1, exact_from_start(p.name, 2))
    start = np.where(p.counted[:, None], leg1[0], p.psi0)    # (a cell without counts returns NaN whatever it starts from)
    judge_run(p, side, rows, pinned, "chain", "%s leg 2" % p.name, start, 2, leg2)
    forced = run_routes(p, side, p.psi0, 7)
    for name, budget in p.routes:
        ruled = side.fit(p, p.psi0, HUGE_EPS, budget)
        assert np.array_equal(ruled[3][p.counted], np.full(int(p.counted.sum()), 6)), (p.name, name, ruled[3])
        assert np.array_equal(ruled[3][~p.counted], np.full(int((~p.counted).sum()), HUGE_EPS[1] - 1))
        for x, y, what in zip(ruled[:3], forced[:3], OUTPUTS):
            assert same_bits(x, y), (p.name, name, "stop rule", what)


RUN = {"em": run_em, "long": run_long}


def run(name, side, rows, pinned):
    p = problem(name)
    RUN[p.spec.kind](p, side, rows, pinned)
    return p


# ------------------------------------------------------------------------------------
# the ELBO gain: name -> variants, columns, pseudocount, ID_prob kind
# ------------------------------------------------------------------------------------
GAIN = {}
GAIN_CELLS = 96                  # threshold sqrt(96) / 3 = 3.27: variants of a few reads fall on both sides


def _g(N, K, pc, kind):
    name = "N%d_K%d_pc%g_%s" % (N, K, pc, kind)
    assert name not in GAIN
    GAIN[name] = SimpleNamespace(name=name, N=N, K=K, pc=pc, kind=kind, seed=500 + len(GAIN))


# K 1 .. 70; pseudocounts 1e-3 (ten steps of digamma's recurrence at an unassigned donor), 0.5, 10 (none anywhere);
# N around the kernel's block of 256 threads, one per variant; the three kinds of ID_prob
_g(257, 1, 0.5, "random")
_g(256, 2, 1e-3, "random")
_g(255, 3, 10.0, "zeros")
_g(255, 7, 0.5, "zeros")
_g(256, 7, 0.5, "onehot")        # integer sums: shapes of exactly 9.5, 10 and 10.5, around digamma's switch
_g(257, 16, 1e-3, "onehot")
_g(256, 40, 0.5, "onehot")
_g(255, 70, 10.0, "onehot")
_g(1, 16, 10.0, "zeros")
_g(1, 40, 1e-3, "random")
_g(1, 70, 0.5, "random")
_g(1, 3, 0.5, "onehot")


@functools.lru_cache(maxsize=2)
def gain_problem(name):
    sp = GAIN[name]
    rng = np.random.default_rng(sp.seed)
    M, N, K = GAIN_CELLS, sp.N, sp.K
    ID = id_prob(rng, M, K, sp.kind)
    crisp = np.flatnonzero(np.all((ID == 0.0) | (ID == 1.0), axis=1) & (ID.sum(axis=1) == 1.0))
    rows = []                                   # per variant: (cells, ad, dp)

    def some(n, top, pool=None):
        cells = np.sort(rng.choice(M if pool is None else pool, n, replace=False))
        dp = rng.integers(1, top + 1, n)
        return cells, rng.binomial(dp, rng.choice([0.02, 0.5, 0.98], n)), dp

    def special(v):
        if v == 0:
            return np.zeros(0, int), np.zeros(0, int), np.zeros(0, int)         # no reads
        if v == 1:
            return np.array([5]), np.array([1]), np.array([1])                  # one read
        if v == 2:
            c, _, dp = some(5, 40)
            return c, dp.copy(), dp                                             # all alternative
        if v == 3:
            c, _, dp = some(5, 40)
            return c, np.zeros(5, int), dp                                      # all reference
        if v == 4:                                                              # 5e6 reads beside one read
            return np.array([3, 60]), np.array([1503211, 1]), np.array([5000017, 1])
        if v == 5:
            return some(M, 40)                                                  # every cell
        if sp.kind == "onehot" and crisp.size and v in (6, 7, 8):               # one donor's sums: 9, 10, 19 reads
            ad = {6: 9, 7: 10, 8: 9}[v]
            return crisp[:1], np.array([ad]), np.array([ad if v < 8 else 19])
        return None

    for v in range(N):
        if N == 1:
            c, ad, dp = some(10, 40)
            dp[0], ad[0] = 5000017, 1503211
            rows.append((c, ad, dp))
            continue
        sv = special(v)
        if sv is not None:
            rows.append(sv)
        else:       # a few cells each; at many columns mostly cells with a 0 / 1 row, so that the sums stay integers
            pool = crisp if (K >= 16 and sp.kind == "onehot" and v % 16 and crisp.size >= 6) else None
            rows.append(some(int(rng.integers(1, 7)), 40, pool))
    r = np.concatenate([np.full(len(c), v) for v, (c, _, _) in enumerate(rows)])
    c = np.concatenate([x[0] for x in rows]).astype(int)
    AD = csc_matrix((np.concatenate([x[1] for x in rows]).astype(np.int64), (r, c)), shape=(N, M))
    DP = csc_matrix((np.concatenate([x[2] for x in rows]).astype(np.int64), (r, c)), shape=(N, M))
    AD.eliminate_zeros()
    g = SimpleNamespace(spec=sp, name=name, N=N, M=M, K=K, pc=sp.pc, ID=ID, AD=AD, DP=DP, C=X.Counts(AD, DP),
                        entries=np.array([len(x[0]) for x in rows]), threshold=np.sqrt(M) / 3.0)
    # both VIREO_LDS settings wherever the variant pass takes the shape (tests/exact_cases.py: both sides >= 63)
    g.lds = ("0", "1") if min(N, M) >= 63 else ("0",)
    return g


def gain_exact(g):
    if getattr(g, "_exact", None) is None:
        g._exact = X.elbo_gain(g.C, g.ID, g.pc)["gain"]
    return g._exact


def gain_shapes(g):
    """every digamma argument of the case (float64): the sums of the donors and of the one-donor model"""
    A1, D1 = np.asarray(g.AD @ g.ID), np.asarray(g.DP @ g.ID)
    a1, d1 = np.asarray(g.AD.sum(1)).ravel(), np.asarray(g.DP.sum(1)).ravel()
    return np.concatenate([x.ravel() for x in (A1 + g.pc, (D1 - A1) + g.pc, D1 + 2 * g.pc, a1 + g.pc,
                                               (d1 - a1) + g.pc, d1 + 2 * g.pc)])


def gain_units(g, gain):
    """per variant: |gain - exact| in units"""
    value, unit = gain_exact(g)
    assert gain.shape == (g.N,) and np.all(np.isfinite(gain)), g.name
    return np.asarray(np.abs(X.ld(gain) - value) / unit, dtype=np.float64)


def run_gain(name, side, rows, pinned):
    """every variant of the case against exact, under each VIREO_LDS setting it takes; the selection
    gain >= threshold as the exact one wherever the exact gain is further from the threshold than the bound"""
    g = gain_problem(name)
    value, unit = gain_exact(g)
    u_orc = float(gain_units(g, ORACLE.gain(g, None)).max())
    for lds in g.lds:
        gain = side.gain(g, lds)
        u = gain_units(g, gain)
        clear = np.abs(value - g.threshold) > X.bound(u_orc) * unit
        assert np.array_equal((gain >= g.threshold)[clear], np.asarray(value >= g.threshold)[clear]), g.name
        judge(rows, pinned, "gain", "%s lds%s" % (name, lds), {"gain": float(u.max())}, {"gain": u_orc})
    return g
