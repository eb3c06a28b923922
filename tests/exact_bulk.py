"""The bulk donor-abundance EM one update at a time, shared by tests/test_exact_bulk_cpu.py (float64 NumPy
in the device's place) and tests/test_gpu_bulk_exact.py (the device): the tile arithmetic of
csrc/vrx_bulk.hip restated, the cases, the float64 side, the judge.

``BulkData.fit(psi, theta, max_iter=1)`` runs two passes: pass 0 sums and applies update 0, pass 1 yields
``logLik[0]`` of the updated parameters and stops.  So psi', theta' and the log-likelihood after exactly one
update come back as float64; a second ``fit(max_iter=1)`` continues from that state.  The exact side is
tests/exact_np.py (``bulk_update``, ``bulk_loglik``); the log-likelihood is judged at the float64 state each
side returned, which its own second pass read.

A case names (K, G), the number of variants as an expression in T (the tile of the pass it is written
against, for a long input) and W (the workgroups that stay resident: CUs x workgroups per CU), the tiles
that gives, and an edit of the values.  Every shape is the smallest at which the path it names exists.
"""
import functools
import zlib
from types import SimpleNamespace

import numpy as np

from tests import bulk_np as B
from tests import exact_np as X
from tests.exact_postfit import judge          # noqa: F401  (the rule, with the table's row format)

# ------------------------------------------------------------------------------------
# the tile arithmetic (bulk_tile and the grid of vrx_bulk_create; the constants of csrc/vrx_bulk.h)
# ------------------------------------------------------------------------------------
BLOCK, Q, COHORT = 256, 8, 4
LDS_TILE, LDS_COHORT, LDS_CU, LDS_MAX = 40 * 1024, 64 * 1024, 160 * 1024, 64 * 1024
PASSES = {"fit": ("T", "n_wg"), "ll": ("T_ll", "n_wg_ll"), "co": ("T_co", "n_wg_co"),
          "co_ll": ("T_co_ll", "n_wg_co_ll")}


def n_slice(K, G):
    return 1 if K * G >= BLOCK else BLOCK // (K * G)


def lds_bytes(K, G, T, which):
    """-> (bytes of a workgroup of T variants, bytes per variant)"""
    L = K * G
    S, SK, n_acc = L | 1, K | 1, n_slice(K, G) * L
    fixed, per = {"fit": (K + G + 1 + 3 * n_acc + 4, S + SK + 2), "ll": (Q * K + G + 4 * Q, S),
                  "co": (COHORT * (4 + K + G + 3 * n_acc) + 1, S + SK + 2),
                  "co_ll": (COHORT * (Q * K + G + 4 * Q), S)}[which]
    return 8 * (fixed + T * per), 8 * per


def tile(N, K, G, which):
    fixed, per = lds_bytes(K, G, 0, which)
    budget = LDS_COHORT if which.startswith("co") else LDS_TILE
    T = (budget - fixed) // per if budget > fixed else 0
    return max(min(T, BLOCK, N + (N & 1)) & ~1, 2)


def per_cu(K, G, T, which):
    return min(4, max(1, LDS_CU // lds_bytes(K, G, T, which)[0]))


def plan(N, K, G, n_cu):
    """what ``BulkData.info()`` reports"""
    out = {}
    for which, (kt, kw) in PASSES.items():
        T = tile(N, K, G, which)
        out[kt], out[kw] = T, min(-(-N // T), n_cu * per_cu(K, G, T, which))
    return out


def long_input(K, G, which, n_cu):
    """-> (T, W) of an input longer than a tile: W workgroups stay resident"""
    T = tile(1 << 30, K, G, which)
    return T, n_cu * per_cu(K, G, T, which)


# ------------------------------------------------------------------------------------
# edits of the values (d: the case's arrays; K >= 2 where a donor is singled out)
# ------------------------------------------------------------------------------------
def ed_zero_psi(d, rng):           # must stay exactly 0
    d.psi0[1] = 0.0
    d.psi0 /= d.psi0.sum()


def ed_tiny_psi(d, rng):           # must stay finite and non-zero
    d.psi0[1] = 1e-300


def ed_near_one_psi(d, rng):
    d.psi0[:] = 1e-12 / (d.K - 1)
    d.psi0[0] = 1 - 1e-12


def ed_small_psi(d, rng):          # one donor at 1e-9: a fold that skips it is 1e-9 out
    d.psi0[d.K - 1] = 0.0
    d.psi0 *= (1 - 1e-9) / d.psi0.sum()
    d.psi0[d.K - 1] = 1e-9


def ed_edge_theta(d, rng):         # t1 reaches 1e-9 and 1 - 1e-9 where every donor is one-hot on class 0 / G - 1
    d.theta0 = np.linspace(0.0, 1.0, d.G)
    d.theta0[0], d.theta0[-1] = 1e-9, 1 - 1e-9
    for g, rows in ((0, slice(0, None, 4)), (d.G - 1, slice(1, None, 4))):
        d.GT[rows] = 0.0
        d.GT[rows, :, g] = 1.0


def ed_onehot_gt(d, rng):          # exact zeros
    g = rng.integers(0, d.G, (d.N, d.K))
    d.GT[:] = 0.0
    np.put_along_axis(d.GT, g[:, :, None], 1.0, axis=2)


def ed_tiny_gt(d, rng):
    d.GT[rng.random(d.GT.shape) < 0.2] = 1e-300


def ed_counts(d, rng):             # no reads, all alternative, all reference
    n = np.arange(d.N)
    d.DP[..., n % 5 == 0] = 0
    d.AD[..., n % 5 == 0] = 0
    d.AD[..., n % 5 == 1] = d.DP[..., n % 5 == 1]
    d.AD[..., n % 5 == 2] = 0


def ed_deep(d, rng):               # 1e6 reads beside 1
    n = np.arange(d.N)
    deep, one = n % 7 == 0, n % 7 == 1
    d.DP[..., deep] = 1000003 - n[deep] % 5
    d.AD[..., deep] = rng.binomial(d.DP[..., deep].astype(np.int64), 0.3)
    d.DP[..., one] = 1
    d.AD[..., one] = n[one] % 2


def ed_tail_1e13(d, rng):          # the last donor's row of the last variant: entries of 1e-13, each another
    d.GT[-1, -1, :] = 1e-13 * np.arange(d.G, 0, -1)
    d.GT[-1, -1, 0] = 1.0


def ed_straddle_1e12(d, rng):      # the first entry of every odd row: the second half of a pair that straddles
    d.theta0[0] = 0.2
    d.GT[1::2, 0, 0] = 1e-12


def ed_last_depth1(d, rng):
    d.DP[-1], d.AD[-1] = 1, 1


EDITS = {f.__name__[3:]: f for f in (ed_zero_psi, ed_tiny_psi, ed_near_one_psi, ed_small_psi, ed_edge_theta,
                                     ed_onehot_gt, ed_tiny_gt, ed_counts, ed_deep, ed_tail_1e13,
                                     ed_straddle_1e12, ed_last_depth1)}
ROTATE = (None, "counts", "deep", "onehot_gt", "tiny_gt")      # the edits any shape takes (inputs of one to three variants: none)


def _rot(i):
    return ROTATE[i % len(ROTATE)]


# ------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------
CASES = {}


def _c(name, kind, K, G, n, tiles, edit=None, **kw):
    """n, tiles: expressions in T and W"""
    assert name not in CASES
    CASES[name] = SimpleNamespace(name=name, kind=kind, K=K, G=G, n=str(n), tiles=str(tiles), edit=edit, **kw)


LOAD_KG = ((1, 2), (1, 3), (2, 2), (3, 3), (5, 3), (4, 5), (7, 4), (3, 8))
LOAD_N = (("1", 1), ("2", 1), ("3", 1), ("T-1", 1), ("T", 1), ("T+1", 2), ("2*T-1", 2), ("2*T+1", 3))
REDUCE = (1, 2, 63, 64, 65, 128, 129)
N_PSI = (1, 7, 8, 9, 17)
SLICE_KG = ((28, 3), (29, 3), (42, 3), (43, 3), (85, 3), (86, 3), (64, 4), (128, 2), (129, 2), (150, 3))

# ---- single sample, one update
for _i, (_K, _G) in enumerate(LOAD_KG):        # L odd and even, nv L odd, a last tile of 1 and of T - 1, both instances
    for _j, (_n, _t) in enumerate(LOAD_N):
        _c("load_K%d_G%d_N=%s" % (_K, _G, _n), "fit", _K, _G, _n, _t, _rot(_i + _j) if _j > 2 else None)
for _i, (_K, _G) in enumerate(SLICE_KG):       # n_slice 3, 2, 2, 1, 1, 1; L = 256, 256, 258; several rounds
    _ns = n_slice(_K, _G)
    for _r in sorted({_ns, _ns + 1, 2 * _ns - 1} - {0}):       # nv % n_slice = 0, 1, n_slice - 1 in the last tile
        _c("slice_K%d_G%d_N=T+%d" % (_K, _G, _r), "fit", _K, _G, "T+%d" % _r, 2, _rot(_i + _r))
_c("grid_tiles=W", "fit", 150, 3, "T*W", "W")
_c("grid_stride", "fit", 150, 3, "2*T*W+3", "2*W+1", "deep")  # a second and a third tile per workgroup
for _i, _n in enumerate(REDUCE):               # partials per lane of vrx_bulk_reduce
    _c("reduce_%d" % _n, "fit", 4, 3, "%d*T-%d" % (_n, _i % 3), _n, _rot(_i))
for _n, _t in ((1, 1), (2, 1), (3, 2), (51, 26)):              # the donor limit: T = 2
    _c("donors454_N=%d" % _n, "fit", 454, 3, _n, _t)
for _K, _n, _t in ((5, "2*T+1", 3), (100, "333", "-(-333//T)")):
    for _e in ("zero_psi", "tiny_psi", "near_one_psi", "small_psi", "edge_theta", "onehot_gt", "tiny_gt", "counts",
               "deep"):
        _c("value_%s_K%d" % (_e, _K), "fit", _K, 3, _n, _t, _e)
# ---- what the corruptions of tests/test_exact_bulk_cpu.py are written for
_c("teeth_odd_tail", "fit", 3, 3, 3, 1, "tail_1e13")                   # nv L = 27
_c("teeth_straddle", "fit", 3, 3, 4, 1, "straddle_1e12")               # L = 9: rows 1, 3 start in a pair's second half
_c("teeth_last_slice", "fit", 28, 3, "T+4", 2, "last_depth1")          # n_slice = 3, nv = 4
# ---- chains: three updates one by one against three at once
for _lt in (True, False):
    _tag = "" if _lt else "_theta_fixed"
    _c("chain_small" + _tag, "chain", 3, 3, "T+1", 2, learn_theta=_lt)
    _c("chain_one_slice" + _tag, "chain", 86, 3, "2*T+1", 3, learn_theta=_lt)
    _c("chain_grid_stride" + _tag, "chain", 150, 3, "2*T*W+3", "2*W+1", learn_theta=_lt)
# ---- the log-likelihood pass (T, W: those of vrx_bulk_ll)
for _i, (_K, _G) in enumerate(((1, 2), (3, 3), (4, 5), (150, 3))):
    for _j, (_n, _t) in enumerate(LOAD_N):
        _c("ll_K%d_G%d_N=%s" % (_K, _G, _n), "ll", _K, _G, _n, _t, _rot(_i + _j) if _j > 2 else None)
for _i, _n in enumerate(REDUCE):
    _c("ll_reduce_%d" % _n, "ll", 4, 3, "%d*T-%d" % (_n, _i % 3), _n, _rot(_i))
_c("ll_grid_stride", "ll", 150, 3, "2*T*W+3", "2*W+1")
# ---- the cohort (T, W: those of vrx_bulk_cohort_pass; of vrx_bulk_cohort_ll where the kind says so)
COHORT_S = (1, COHORT - 1, COHORT, COHORT + 1, 2 * COHORT + 1)
for _i, (_K, _G, _n, _t) in enumerate(((1, 2, "T+1", 2), (3, 3, "2*T+1", 3), (4, 5, "2*T-1", 2), (43, 3, "T+1", 2),
                                       (128, 2, "T+2", 2), (129, 2, "T+1", 2), (150, 3, "T-1", 1),
                                       (3, 3, "3", 1), (4, 5, "T", 1), (1, 2, "2*T+1", 3))):
    _c("cohort_K%d_G%d_N=%s_S%d" % (_K, _G, _n, COHORT_S[_i % 5]), "cohort", _K, _G, _n, _t, S=COHORT_S[_i % 5])
_c("cohort_grid_stride", "cohort", 150, 3, "2*T*W+3", "2*W+2", S=COHORT + 1)         # (T = 2: two tiles more)
_c("cohort_ll_grid_stride", "cohort_ll", 150, 3, "2*T*W+3", "2*W+1", S=2)
for _i, (_K, _G) in enumerate(((43, 3), (128, 2), (129, 2), (150, 3))):      # where T_co_ll is not T_co
    _c("cohort_ll_K%d_G%d_N=T+1_S%d" % (_K, _G, COHORT_S[_i + 1]), "cohort_ll", _K, _G, "T+1", 2, S=COHORT_S[_i + 1])
_c("cohort_chain", "cohort_chain", 5, 3, "T+1", 2, S=COHORT + 1)

WHICH = {"fit": "fit", "chain": "fit", "ll": "ll", "cohort": "co", "cohort_ll": "co_ll", "cohort_chain": "co"}


@functools.lru_cache(maxsize=2)
def build(name, n_cu):
    """the arrays of a case on a device of n_cu CUs, with the tile and workgroup counts it is written for"""
    sp = CASES[name]
    which = WHICH[sp.kind]
    T, W = long_input(sp.K, sp.G, which, n_cu)
    N = int(eval(sp.n, {"T": T, "W": W}))
    seed = zlib.crc32(name.encode()) % (1 << 31)
    AD, DP, GT, _, _ = B.synth_pool(N, sp.K, sp.G, seed=seed, private=False)
    rng = np.random.default_rng(seed + 1)
    d = SimpleNamespace(spec=sp, name=name, N=N, K=sp.K, G=sp.G, which=which, GT=GT, n_cu=n_cu)
    S = getattr(sp, "S", 0)
    if S:                                   # different counts, depths and starts per sample
        rate = np.tensordot(GT, np.linspace(0.01, 0.99, sp.G), axes=(2, 0))
        depth = [(30.0, 1e6, 1.0, 8.0)[s % COHORT] for s in range(S)]     # 1e6 beside 1 in every chunk
        d.DP = np.stack([rng.poisson(depth[s], N) if depth[s] > 1 else np.ones(N, dtype=np.int64)
                         for s in range(S)]).astype(np.float64)
        d.AD = np.stack([rng.binomial(d.DP[s].astype(np.int64), rate @ rng.dirichlet(np.full(sp.K, 2.0)))
                         for s in range(S)]).astype(np.float64)
        d.psi0 = rng.dirichlet(np.full(sp.K, 2.0), size=S)
        d.theta0 = np.linspace(0.05, 0.9, sp.G) + rng.uniform(-0.02, 0.02, (S, sp.G))
    else:
        d.AD, d.DP = AD.astype(np.float64), DP.astype(np.float64)
        d.psi0 = rng.dirichlet(np.full(sp.K, 2.0))
        d.theta0 = np.linspace(0.05, 0.9, sp.G) + rng.uniform(-0.02, 0.02, sp.G)
    if N < 16:                              # a handful of variants: reads of both alleles at each, or an update
        d.DP = np.maximum(d.DP, 2.0)        # ends at theta = 0 or 1 and the log-likelihood at 0 x inf
        d.AD = np.clip(d.AD, 1.0, d.DP - 1)
    if sp.edit:
        EDITS[sp.edit](d, rng)
    d.BD = d.DP - d.AD
    d.psis = rng.dirichlet(np.full(sp.K, 2.0), size=(S, max(N_PSI)) if S else max(N_PSI))
    # the tile and workgroup counts the case is written for
    d.plan = plan(N, sp.K, sp.G, n_cu)
    d.T, d.n_wg = (d.plan[k] for k in PASSES[which])
    d.tiles = -(-N // d.T)
    assert d.tiles == int(eval(sp.tiles, {"T": T, "W": W})), (name, N, d.T, d.tiles)
    assert d.n_wg == min(d.tiles, W), (name, d.n_wg, W)
    assert d.T == (T if N >= T else N + (N & 1)), (name, N, d.T, T)    # (a short input: a short tile)
    for arr in (d.AD, d.DP, d.BD, d.GT, d.psi0, d.theta0, d.psis):
        arr.setflags(write=False)
    return d


def a_priori(d):
    """the longest contraction (the variants, then donors and classes) + 16"""
    return d.N + d.K + d.G + 16


# ------------------------------------------------------------------------------------
# the float64 side: tests/bulk_np.py in the device's place
# ------------------------------------------------------------------------------------
class Float64Side:
    """the calls a case makes, answered by the NumPy restatement; tests/test_gpu_bulk_exact.py answers
    them with a ``BulkData``"""

    def fit(self, d, psi, theta, max_iter=1, learn_theta=True):
        """-> psi, theta, logLik[0 .. max_iter - 1]"""
        return self._fit(d.AD, d.DP, d.GT, psi, theta, max_iter, learn_theta)

    @staticmethod
    def _fit(AD, DP, GT, psi, theta, max_iter, learn_theta):
        r = B.fit(AD, DP, GT, psi, theta, max_iter=max_iter, learn_theta=learn_theta, delay_fit_theta=0)
        return r["psi"], r["theta"], np.append(r["logLik_all"], r["logLik"])

    def loglik(self, d, psis, theta):
        return np.array([B.loglik(d.AD, d.BD, d.GT, p, theta) for p in psis])

    def fit_cohort(self, d, idx, psi, theta, max_iter=1, learn_theta=True):
        """the samples idx of the case as a cohort, from the rows of psi, theta -> psi, theta, traces"""
        out = [self._fit(d.AD[s], d.DP[s], d.GT, psi[i], theta[i], max_iter, learn_theta) for i, s in enumerate(idx)]
        return tuple(np.stack([o[j] for o in out]) for j in range(3))

    def loglik_cohort(self, d, idx, psis, theta):
        return np.array([[B.loglik(d.AD[s], d.BD[s], d.GT, p, theta[i]) for p in psis[i]] for i, s in enumerate(idx)])


ORACLE = Float64Side()


# ------------------------------------------------------------------------------------
# running a case on a side
# ------------------------------------------------------------------------------------
def update_distances(AD, BD, GT, start, got, learn_theta=True):
    """psi', theta' of one update from ``start`` against exact; logLik against the exact value at the
    float64 (psi', theta') it was taken of"""
    psi, theta, trace = got
    assert trace.shape == (1,)
    ex = X.bulk_update(AD, BD, GT, *start)
    u = {"psi": X.distance(psi, *ex["psi"])}
    if learn_theta:
        u["theta"] = X.distance(theta, *ex["theta"])
    u["logLik"] = X.distance(trace[0], *X.bulk_loglik(AD, BD, GT, psi, theta))
    return u


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _check_values(d, psi, theta, trace):
    assert np.all(np.isfinite(psi)) and np.all(np.isfinite(theta)) and np.all(np.isfinite(trace)), d.name
    assert np.all(theta > 0) and np.all(theta < 1)
    if d.spec.edit == "zero_psi":
        assert d.psi0[1] == 0.0 and psi[1] == 0.0 and not np.signbit(psi[1])
    if d.spec.edit == "tiny_psi":
        assert 0.0 < psi[1] < 1e-290


def run_fit(d, side, rows, pinned, step="fit"):
    got = side.fit(d, d.psi0, d.theta0)
    _check_values(d, *got)
    u_dev = update_distances(d.AD, d.BD, d.GT, (d.psi0, d.theta0), got)
    u_orc = update_distances(d.AD, d.BD, d.GT, (d.psi0, d.theta0), ORACLE.fit(d, d.psi0, d.theta0))
    judge(rows, pinned, step, d.name, u_dev, u_orc)
    return u_orc


def run_chain(d, side, rows, pinned):
    """three fits of one iteration, each judged alone from the float64 state the side returned in front
    of it; one fit of three iterations returns the same bits"""
    lt = d.spec.learn_theta
    state, traces = (d.psi0, d.theta0), []
    for i in range(3):
        got = side.fit(d, *state, learn_theta=lt)
        if not lt:
            assert same_bits(got[1], state[1])          # theta comes back as given
        u_dev = update_distances(d.AD, d.BD, d.GT, state, got, lt)
        u_orc = update_distances(d.AD, d.BD, d.GT, state, ORACLE.fit(d, *state, learn_theta=lt), lt)
        judge(rows, pinned, "chain", "%s update %d" % (d.name, i), u_dev, u_orc)
        state = got[:2]
        traces.append(got[2][0])
    psi, theta, trace = side.fit(d, d.psi0, d.theta0, max_iter=3, learn_theta=lt)
    assert same_bits(psi, state[0]) and same_bits(theta, state[1]) and same_bits(trace, traces), d.name


def run_loglik(d, side, rows, pinned):
    """n_psi = 1, 7, 8, 9, 17 vectors in one call and one by one: the same bits; every value against exact"""
    every = side.loglik(d, d.psis, d.theta0)
    assert every.shape == (max(N_PSI),) and np.all(np.isfinite(every))
    for n in N_PSI:
        assert same_bits(side.loglik(d, d.psis[:n], d.theta0), every[:n]), (d.name, n)
    for q in range(max(N_PSI)):
        assert same_bits(side.loglik(d, d.psis[q:q + 1], d.theta0), every[q:q + 1]), (d.name, q)
    ex = X.bulk_loglik(d.AD, d.BD, d.GT, d.psis, d.theta0)
    judge(rows, pinned, "loglik", d.name, {"logLik": X.distance(every, *ex)},
          {"logLik": X.distance(ORACLE.loglik(d, d.psis, d.theta0), *ex)})


def _shifted(S):
    """the cohort with a copy of its last sample in front: every sample one slot further"""
    return [S - 1] + list(range(S))


def run_cohort(d, side, rows, pinned):
    """every sample against exact, and bitwise what it is in a cohort of one and in another slot"""
    S = d.spec.S
    idx = list(range(S))
    got = side.fit_cohort(d, idx, d.psi0, d.theta0)
    orc = ORACLE.fit_cohort(d, idx, d.psi0, d.theta0)
    for s in idx:
        u_dev = update_distances(d.AD[s], d.BD[s], d.GT, (d.psi0[s], d.theta0[s]), [x[s] for x in got])
        u_orc = update_distances(d.AD[s], d.BD[s], d.GT, (d.psi0[s], d.theta0[s]), [x[s] for x in orc])
        judge(rows, pinned, "cohort", "%s sample %d" % (d.name, s), u_dev, u_orc)
    sh = _shifted(S)
    moved = side.fit_cohort(d, sh, d.psi0[sh], d.theta0[sh])
    for x, y in zip(got, moved):
        assert same_bits(x, y[1:]), d.name
    for s in idx:
        alone = side.fit_cohort(d, [s], d.psi0[s:s + 1], d.theta0[s:s + 1])
        for x, y in zip(got, alone):
            assert same_bits(x[s:s + 1], y), (d.name, s)
    run_cohort_loglik(d, side, rows, pinned, n_psi=(1, 9))


def run_cohort_loglik(d, side, rows, pinned, n_psi=N_PSI):
    S = d.spec.S
    idx = list(range(S))
    every = side.loglik_cohort(d, idx, d.psis, d.theta0)
    assert every.shape == (S, max(N_PSI)) and np.all(np.isfinite(every))
    for n in n_psi:
        assert same_bits(side.loglik_cohort(d, idx, d.psis[:, :n], d.theta0), every[:, :n]), (d.name, n)
    sh = _shifted(S)
    assert same_bits(side.loglik_cohort(d, sh, d.psis[sh], d.theta0[sh])[1:], every), d.name
    orc = ORACLE.loglik_cohort(d, idx, d.psis, d.theta0)
    for s in idx:
        assert same_bits(side.loglik_cohort(d, [s], d.psis[s:s + 1], d.theta0[s:s + 1]), every[s:s + 1]), (d.name, s)
        ex = X.bulk_loglik(d.AD[s], d.BD[s], d.GT, d.psis[s], d.theta0[s])
        judge(rows, pinned, "co_ll", "%s sample %d" % (d.name, s), {"logLik": X.distance(every[s], *ex)},
              {"logLik": X.distance(orc[s], *ex)})


def run_cohort_chain(d, side, rows, pinned):
    S = d.spec.S
    idx = list(range(S))
    state, traces = (d.psi0, d.theta0), []
    for i in range(3):
        got = side.fit_cohort(d, idx, *state)
        orc = ORACLE.fit_cohort(d, idx, *state)
        for s in idx:
            start = (state[0][s], state[1][s])
            u_dev = update_distances(d.AD[s], d.BD[s], d.GT, start, [x[s] for x in got])
            u_orc = update_distances(d.AD[s], d.BD[s], d.GT, start, [x[s] for x in orc])
            judge(rows, pinned, "cohort", "%s sample %d update %d" % (d.name, s, i), u_dev, u_orc)
        state = got[:2]
        traces.append(got[2][:, 0])
    psi, theta, trace = side.fit_cohort(d, idx, d.psi0, d.theta0, max_iter=3)
    assert same_bits(psi, state[0]) and same_bits(theta, state[1]) and same_bits(trace, np.stack(traces, axis=1))


RUN = {"fit": run_fit, "chain": run_chain, "ll": run_loglik, "cohort": run_cohort, "cohort_ll": run_cohort_loglik,
       "cohort_chain": run_cohort_chain}


def run(name, n_cu, side, rows, pinned):
    d = build(name, n_cu)
    RUN[d.spec.kind](d, side, rows, pinned)
    return d
