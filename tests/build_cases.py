"""The builder sweep shared by tests/test_build_cases_cpu.py (NumPy in the device's place) and
tests/test_gpu_build_exact.py (both problem builders on the device): cases, integer operands, the
int64 products, the restated build rules and the planted defects.

A *case* is a small merged (AD, DP) pattern -- one CSC pattern with an (ad, dp) pair per entry, as
``DeviceCounts.from_merged`` takes it, so that explicit zeros stay in -- an environment, a ``balance``
flag, and what the build must then report: whether ``VIREO_BUILD=device`` builds on the device
(``device_built``; the cases where ``device_build`` declines carry the reason), the stream forms,
the entry formats, the rows cut into pieces.  The rules that decide those (``pick_forms`` /
``settle_forms``, ``pick_fmt``, the pieces of ``tile_layout``, the virtual rows) are restated here;
the CPU twin holds every declaration to the restated rule.

The check needs no decoder: with integer operands a pass over the packed entries or over a tiled
stream is exact integer arithmetic in float64 whatever its summation order, as long as the sum of
|weight| x |count| over an output cell stays below 2^53 (``magnitudes``).  Every entry of
``donor_reads(ID)`` and of ``vrx_problem_cell_loglik`` at one class must then EQUAL the SciPy int64
product (``products``), and one entry lost, repeated or misplaced changes an integer (``DEFECTS``).
"""
import functools
import zlib
from types import SimpleNamespace

import numpy as np
from scipy.sparse import csc_matrix

from tests import exact_cases as EC

LDS1 = EC.LDS1
PAIRS = dict(VIREO_CELL_FORM="0", VIREO_VAR_FORM="0")
ADBD = dict(VIREO_CELL_FORM="1", VIREO_VAR_FORM="3")
# every switch a case or the GPU test sets: cleared in front of each build
ENV_KEYS = ("VIREO_BUILD", "VIREO_LDS", "VIREO_ENTRY_FMT", "VIREO_CELL_FORM", "VIREO_VAR_FORM",
            "VIREO_LDS_SLAB_CELL", "VIREO_BUILD_CONCURRENT", "VIREO_BALANCE_CHECK", "VIREO_BALANCE_GREEDY",
            "VIREO_LDS_SPLIT_X10", "VIREO_LDS_FILL_CUS", "VIREO_LDS_BLOCKS", "VIREO_LDS_SORT", "VIREO_BALANCE",
            "VIREO_BALANCE_SPLIT", "VIREO_BALANCE_BLOCK", "VIREO_PAIR_WORDS_X100", "VIREO_LDS_MIN_NNZ",
            "VIREO_LDS_MIN_NNZ_VAR", "VIREO_LDS_MAX_PAD", "VIREO_TILES_CELL", "VIREO_TILES_VAR")

# the feature tags of the sweep: each is carried by at least one case (the CPU twin), and appears in the
# GPU run's table on a device-built case -- except the two declared fall-backs
TAGS = ("single_entry", "one_variant", "one_cell", "odd_n_cell", "row_4095", "row_4096", "row_4097",
        "long_variant_row", "long_cell_row", "explicit_zero", "dp_zero", "ad_zero", "negative_bd",
        "count_2047", "count_2048", "count_32767", "count_32768", "fmt_boundary_63", "fmt_boundary_64",
        "fmt_boundary_65535", "fmt_boundary_65536", "entry_fmt_0", "entry_fmt_1", "entry_fmt_2",
        "empty_edges", "heavy_tail_pieces", "slab_cell_32", "build_serial", "balanced", "balanced_pieces",
        "balance_check", "balance_greedy_host", "pair_tile_64", "adbd_tile_96", "slab_edge", "size_edge",
        "pair_words", "adbd_words", "mixed_forms", "several_slabs", "ragged", "declines_nnz_0",
        "declines_pairs_2048")
FALL_BACKS = ("declines_nnz_0", "declines_pairs_2048")

N_COLS = (1, 5, 16, 17)          # one column, a ragged block, a flat block, a strided pair of blocks
GPU_SEED = 0                     # the operand seed of the GPU test
SEEDS = (0, 1, 2)                # the seeds the planted defects are held to (GPU_SEED among them)
ID_TOP, GT_TOP, PSI_TOP = 1 << 20, 1 << 10, 1 << 9
# cell orientation: (name, n_col, (psi1, psi2, psis) or None = signed per-variant rows).  The unit
# settings isolate AD, BD and DP; n_col 1 stays on the gather kernels of a host-built problem
CELL_OPS = (("rows", 5, None), ("AD", 16, (1, 0, 0)), ("BD", 17, (0, 1, 0)), ("DP", 1, (0, 0, -1)))


# ------------------------------------------------------------------------------------
# data
# ------------------------------------------------------------------------------------
def _rand(N, M, density, top, seed, lo=1):
    rng = np.random.default_rng(seed)
    dp = (rng.random((N, M)) < density) * rng.integers(lo, top + 1, (N, M))
    return rng.binomial(dp, rng.choice([0.03, 0.5, 0.96], (N, 1))), dp


def _single():
    ad, dp = np.zeros((70, 40), np.int64), np.zeros((70, 40), np.int64)
    dp[33, 17], ad[33, 17] = 5, 2
    return ad, dp


def _odd_cells():
    """an odd number of cells: the last double row of the virtual rows holds one cell, with entries"""
    ad, dp = _rand(130, 1027, 0.04, 9, 31)
    dp[::3, -1] = 4
    ad[::3, -1] = 1
    return ad, dp


def _long_row(L, cell):
    """one variant that covers L cells (cell: one cell that covers L variants) over a sparse rest"""
    def make():
        ad, dp = _rand(24, L + 2, 0.01, 5, L)
        rng = np.random.default_rng(L + 1)
        dp[5, 1:L + 1] = rng.integers(1, 6, L)
        dp[5, 0] = dp[5, L + 1] = 0
        ad[5, :] = rng.binomial(dp[5, :], 0.4)
        return (ad.T.copy(), dp.T.copy()) if cell else (ad, dp)
    return make


def _zeros():
    """explicit zeros: entries that stay in the pattern with (0, 0); dp = 0 beside ad > 0; ad = 0"""
    ad, dp = _rand(200, 150, 0.1, 9, 41)
    rng = np.random.default_rng(42)
    keep = rng.random(dp.shape) < 0.03                  # (0, 0) where nothing was drawn, kept
    gone = (dp > 0) & (rng.random(dp.shape) < 0.15)     # dp = 0, ad as drawn (some of them > 0)
    ad[gone] += 1
    dp[gone] = 0
    ad[(dp > 0) & (rng.random(dp.shape) < 0.3)] = 0
    dp[-1, -1], ad[-1, -1] = 3, 1                       # (the last entry of the last row counts)
    return ad, dp, keep


def _neg_bd():
    ad, dp = _rand(200, 150, 0.1, 40, 43)
    swap = (dp > 0) & (np.random.default_rng(44).random(dp.shape) < 0.2)
    ad[swap] = dp[swap] + 1 + ad[swap]                  # AD beyond DP: BD = DP - AD < 0
    return ad, dp


def _top(top, seed):
    """counts below ``top`` and two entries at it (one with ad = dp, one with ad = dp // 3)"""
    def make():
        ad, dp = _rand(160, 120, 0.15, top - 1, seed)
        dp[3, 7], ad[3, 7] = top, top
        dp[150, 100], ad[150, 100] = top, top // 3
        return ad, dp
    return make


def _empty_edges():
    ad, dp = _rand(300, 260, 0.08, 9, 51)
    dp[:40], dp[-35:], dp[:, :30], dp[:, -33:] = 0, 0, 0, 0
    return np.minimum(ad, dp), dp


def heavy_tail(N, M, seed=11, K=6):
    """the input of test_balanced_slabs_with_rows_cut_into_pieces (tests/test_gpu_parity.py) at N x M"""
    rng = np.random.default_rng(seed)
    cov_v = np.exp(rng.normal(0.0, 1.2, N))[:, None]
    cov_c = np.exp(rng.normal(0.0, 1.0, M))[None, :]
    p = np.minimum(0.9, 0.025 * cov_v * cov_c / (cov_v.mean() * cov_c.mean()))
    dp = (rng.random((N, M)) < p) * (1 + rng.poisson(1.5, (N, M)))
    z = rng.integers(0, K, M)
    gt = rng.integers(0, 3, (N, K))
    return rng.binomial(dp, np.array([0.01, 0.5, 0.99])[gt][:, z]), dp


# that input is 2600 x 2300: at 8, 10 and 12 % of it, the smallest that cuts pieces in both orientations
HEAVY_LADDER = ((208, 184), (260, 230), (312, 276))
HEAVY_SMALL = HEAVY_LADDER[-1]
BAL_SHAPE = (600, 1100)      # more than one nominal slab in both orientations (512 variants, 512 cell pairs)

DATA = {
    "single": _single,
    "one_variant": lambda: _rand(1, 700, 0.5, 9, 21),
    "one_cell": lambda: _rand(700, 1, 0.5, 9, 22),
    "odd_cells": _odd_cells,
    "zeros": _zeros,
    "neg_bd": _neg_bd,
    "top2047": _top(2047, 61),
    "top2048": _top(2048, 62),
    "top32767": _top(32767, 63),
    "top32768": _top(32768, 64),
    "top63": _top(63, 65),
    "top64": _top(64, 66),
    "top65535": _top(65535, 67),
    "top65536": _top(65536, 68),
    "empty_edges": _empty_edges,
    "heavy": lambda: heavy_tail(*HEAVY_SMALL),
    "plain": lambda: _rand(300, 260, 0.08, 9, 71),
    "bal": lambda: _rand(*BAL_SHAPE, 0.03, 6, 72),
    "bal_heavy": lambda: heavy_tail(*BAL_SHAPE),
    "empty": lambda: (np.zeros((70, 40), np.int64), np.zeros((70, 40), np.int64)),
}
for _L in (4095, 4096, 4097):
    DATA["row%d_var" % _L] = _long_row(_L, False)
    DATA["row%d_cell" % _L] = _long_row(_L, True)


def merge(AD, DP, keep=None):
    """(shape, colptr int64, rowidx int32, ad int32, dp int32) on the union pattern of two sparse or
    dense matrices, plus the positions of ``keep`` (explicit zeros): what ``merge_counts`` hands the
    library, formed independently of it"""
    AD, DP = csc_matrix(AD), csc_matrix(DP)
    N, M = AD.shape
    parts = []
    for X in (AD, DP) + (() if keep is None else (csc_matrix(keep),)):
        X = X.copy()
        X.sum_duplicates()
        X.eliminate_zeros()
        cols = np.repeat(np.arange(M, dtype=np.int64), np.diff(X.indptr))
        parts.append((cols * N + X.indices, X.data))
    keys = np.unique(np.concatenate([k for k, _ in parts]))
    ad, dp = np.zeros(keys.size, np.int32), np.zeros(keys.size, np.int32)
    ad[np.searchsorted(keys, parts[0][0])] = parts[0][1]
    dp[np.searchsorted(keys, parts[1][0])] = parts[1][1]
    colptr = np.zeros(M + 1, np.int64)
    np.cumsum(np.bincount(keys // N, minlength=M), out=colptr[1:])
    return (N, M), colptr, (keys % N).astype(np.int32), ad, dp


def matrices(merged):
    """int64 CSC (AD, DP) of a merged pattern; explicit zeros stay stored and change no product"""
    shape, colptr, rowidx, ad, dp = merged
    return (csc_matrix((ad.astype(np.int64), rowidx, colptr), shape=shape),
            csc_matrix((dp.astype(np.int64), rowidx, colptr), shape=shape))


@functools.lru_cache(maxsize=None)
def merged(data):
    if data in DATA:
        out = DATA[data]()
        return merge(*out)
    return merge(*EC.data(data))


# ------------------------------------------------------------------------------------
# the build rules, restated (vrx_engine.hip)
# ------------------------------------------------------------------------------------
def form1_words(v):
    """vrx_form1_words: a count is cut into chunks of at most three significant bits, largest first"""
    v, n = abs(int(v)), 0
    while v:
        sh = max(0, v.bit_length() - 3)
        v -= (v >> sh) << sh
        n += 1
    return n


def expected_forms(m, env):
    """pick_forms + settle_forms -> (cell_form, var_form): pair words when every 61st entry averages more
    than 1.56 AD/BD words, AD/BD words after all when a count does not fit the pairs' 11 bits; a forced
    form stays"""
    _, _, _, ad, dp = m
    words = [form1_words(a) + form1_words(d - a) for a, d in zip(ad[::61].tolist(), dp[::61].tolist()) if d >= a]
    pairs = (sum(words) / len(words) if words else 1.0) > 1.56
    forced = "VIREO_CELL_FORM" in env or "VIREO_VAR_FORM" in env
    cell = int(env.get("VIREO_CELL_FORM", 0 if pairs else 1))
    var = int(env.get("VIREO_VAR_FORM", 0 if pairs else 3))
    if pairs and not forced and max_count(m) >= 2048:
        cell, var = 1, 3
    return cell, var


def max_count(m):
    return int(max(m[3].max(initial=0), m[4].max(initial=0)))


def expected_format(m, env):
    """pick_fmt -> (variant, cell) orientation: the narrowest entry format that holds the counts (the
    contracted index fits 20 bits at these sizes); VIREO_ENTRY_FMT may only widen it"""
    top = max_count(m)
    f = 0 if top < 64 else 1 if top < 65536 else 2
    forced = int(env.get("VIREO_ENTRY_FMT", -1))
    f = forced if f <= forced <= 2 else f
    return f, f


def _rows_by_variant(m):
    (N, M), colptr, rowidx, ad, dp = m
    cols = np.repeat(np.arange(M, dtype=np.int64), np.diff(colptr))
    order = np.argsort(rowidx, kind="stable")
    return rowidx[order].astype(np.int64), cols[order], ad[order].astype(np.int64), dp[order].astype(np.int64)


def _extra(lens, split_x10):
    """tile_layout: a row longer than max(64, mean x VIREO_LDS_SPLIT_X10 / 10) is cut into pieces"""
    lens = np.asarray(lens, np.int64)
    mean = lens.sum() / max(lens.size, 1)
    cap = max(64, int(mean * split_x10 / 10.0 + 0.5))
    return int(np.maximum(1, -(-lens // cap)).sum() - lens.size)


def expected_pieces(m, env, var_form):
    """(variant, cell): the row pieces beyond one per row, ``info()``'s extra_pieces_*.  Virtual rows
    (var_form 3): row 2n holds the pairs of cells where variant n has AD counts, row 2n + 1 those
    where it has BD counts"""
    (N, M), colptr, _, _, _ = m
    x10 = int(env.get("VIREO_LDS_SPLIT_X10", 20))
    cell = _extra(np.diff(colptr), x10)
    r, c, a, d = _rows_by_variant(m)
    if var_form == 3:
        lens = np.zeros(2 * N, np.int64)
        for half, on in ((0, a != 0), (1, d - a != 0)):
            key = np.unique(r[on] * ((M + 1) // 2 + 1) + c[on] // 2)
            lens[half::2] = np.bincount(key // ((M + 1) // 2 + 1), minlength=N)
        return _extra(lens, x10), cell
    return _extra(np.bincount(r, minlength=N), x10), cell


# ------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------
CASES = {}


def _case(name, data, tags, env=None, balance=False, device_built=True, declines=None, forms=(1, 3),
          fmt=0, pieces=(None, None), host_lds=True):
    """forms: (cell_form, var_form) of the streams; fmt: the entry format of both orientations;
    pieces: (variant, cell) -- True: some rows are cut, False: none, None: not named; host_lds: the host
    builder builds the streams under VIREO_LDS=1; declines: why ``device_build`` leaves the problem to
    the host builder (device_built is then False)"""
    assert name not in CASES and set(tags) <= set(TAGS), (name, set(tags) - set(TAGS))
    assert device_built == (declines is None)
    CASES[name] = SimpleNamespace(name=name, data=data, tags=tuple(tags), env=dict(LDS1, **(env or {})),
                                  balance=balance, device_built=device_built, declines=declines,
                                  cell_form=forms[0], var_form=forms[1], entry_format=(fmt, fmt),
                                  pieces=pieces, host_lds=host_lds)


def _both(name, data, tags, fmt=0, **kw):
    """a case on AD/BD words and its twin on pair words, both forced"""
    _case(name, data, tuple(tags) + ("adbd_words",), env=ADBD, forms=(1, 3), fmt=fmt, **kw)
    _case(name + "_pairs", data, tuple(tags) + ("pair_words",), env=PAIRS, forms=(0, 0), fmt=fmt, **kw)


# ---- shapes exact_cases.py already has, on the forms their counts choose by themselves
_case("mid", "mid", ["adbd_words"])
_case("many", "many", ["several_slabs", "adbd_words"])
_case("ragged", "ragged", ["ragged", "adbd_words"], pieces=(True, True))
_case("split", "split", ["heavy_tail_pieces", "adbd_words"], fmt=1, pieces=(True, True))
_case("pair_tall", "pair_tall", ["pair_tile_64", "pair_words"], env=PAIRS, forms=(0, 0))
_case("shallow_tall", "shallow_tall", ["adbd_tile_96", "adbd_words"])
_case("one_beyond", "one_beyond", ["count_2048", "adbd_words"], fmt=1)
_case("depth3", "depth3", ["adbd_words"])
_case("depth255", "depth255", ["pair_words"], forms=(0, 0), fmt=1)
_case("depth2047", "depth2047", ["count_2047", "pair_words"], forms=(0, 0), fmt=1)
_case("depth_beyond", "depth_beyond", ["adbd_words"], fmt=1)
_case("form_c1_v0", "depth255", ["mixed_forms"], env=dict(VIREO_CELL_FORM="1", VIREO_VAR_FORM="0"), forms=(1, 0), fmt=1)
_case("form_c0_v3", "depth255", ["mixed_forms"], env=dict(VIREO_CELL_FORM="0", VIREO_VAR_FORM="3"), forms=(0, 3), fmt=1)
for _tag in EC.SLAB_EDGES:
    _both("slab_edge_" + _tag, "slab_edge_" + _tag, ["slab_edge"])
for _n, _m in ((255, 1), (1, 63), (256, 64), (257, 65), (1025, 257)):
    _both("size_%dx%d" % (_n, _m), "size_%dx%d" % (_n, _m), ["size_edge"])

# ---- what targets the builder alone
_both("single", "single", ["single_entry"])
_both("one_variant", "one_variant", ["one_variant"], pieces=(False, False))
_both("one_cell", "one_cell", ["one_cell"], pieces=(False, False))
_both("odd_cells", "odd_cells", ["odd_n_cell"])
for _L in (4095, 4096, 4097):
    _both("row%d_var" % _L, "row%d_var" % _L, ["row_%d" % _L, "long_variant_row"], pieces=(True, False))
    _both("row%d_cell" % _L, "row%d_cell" % _L, ["row_%d" % _L, "long_cell_row"], pieces=(False, True))
_both("zeros", "zeros", ["explicit_zero", "dp_zero", "ad_zero", "negative_bd"])
_both("neg_bd", "neg_bd", ["negative_bd"], fmt=1)
_case("top2047", "top2047", ["count_2047", "pair_words"], forms=(0, 0), fmt=1)       # deep counts: pairs by themselves
_case("top2048", "top2048", ["count_2048", "adbd_words"], forms=(1, 3), fmt=1)       # ... AD/BD words after all
_case("top2048_pairs", "top2048", ["count_2048", "declines_pairs_2048"], env=PAIRS, forms=(0, 0), fmt=1,
      device_built=False, declines="pair words forced and a count of 2048: their 11 bits cannot hold it",
      host_lds=False)
_case("top32767", "top32767", ["count_32767", "adbd_words"], env=ADBD, fmt=1)
_case("top32768", "top32768", ["count_32768", "adbd_words"], env=ADBD, fmt=1)
for _top, _nat in ((63, 0), (64, 1), (65535, 1), (65536, 2)):
    for _f in (0, 1, 2):
        _case("top%d_fmt%d" % (_top, _f), "top%d" % _top,
              ["fmt_boundary_%d" % _top, "entry_fmt_%d" % max(_f, _nat), "adbd_words"],
              env=dict(ADBD, VIREO_ENTRY_FMT=str(_f)), fmt=max(_f, _nat))
_both("empty_edges", "empty_edges", ["empty_edges"])
_case("heavy", "heavy", ["heavy_tail_pieces", "adbd_words"], env=ADBD, pieces=(True, True))
_case("heavy_pairs", "heavy", ["heavy_tail_pieces", "pair_words"], env=PAIRS, forms=(0, 0), pieces=(True, True))
_both("slab_cell32", "plain", ["slab_cell_32"])
for _n in ("slab_cell32", "slab_cell32_pairs"):
    CASES[_n].env["VIREO_LDS_SLAB_CELL"] = "32"
_both("serial", "plain", ["build_serial"])
for _n in ("serial", "serial_pairs"):
    CASES[_n].env["VIREO_BUILD_CONCURRENT"] = "0"
# balanced slabs (AD/BD words of several slabs): the greedy on the device, compared with the host's inside
# the build (VIREO_BALANCE_CHECK=1), and the host's alone; rows whole and cut into pieces
BAL = dict(ADBD, VIREO_BALANCE_CHECK="1")
_case("bal_plain", "bal", ["several_slabs", "adbd_words"], env=ADBD)
_case("bal", "bal", ["balanced", "balance_check"], env=dict(BAL, VIREO_LDS_SPLIT_X10="60"), balance=True,
      pieces=(False, False))
_case("bal_greedy_host", "bal", ["balanced", "balance_greedy_host"],
      env=dict(ADBD, VIREO_LDS_SPLIT_X10="60", VIREO_BALANCE_GREEDY="host"), balance=True, pieces=(False, False))
_case("bal_pieces", "bal_heavy", ["balanced", "balanced_pieces", "balance_check"], env=BAL, balance=True,
      pieces=(True, True))
_case("bal_pieces_greedy_host", "bal_heavy", ["balanced", "balanced_pieces", "balance_greedy_host"],
      env=dict(ADBD, VIREO_BALANCE_GREEDY="host"), balance=True, pieces=(True, True))
_case("bal_heavy_small", "heavy", ["balanced", "balanced_pieces", "balance_check"], env=BAL, balance=True,
      pieces=(True, True))
# ---- where device_build declines: the host builder takes over, and says so
_case("empty", "empty", ["declines_nnz_0"], env=ADBD, device_built=False,
      declines="nnz = 0: nothing to build on the device")


def case_env(spec, build, **more):
    """the environment of one build of a case"""
    return dict(spec.env, VIREO_BUILD=build, **more)


# ------------------------------------------------------------------------------------
# integer operands and the int64 products
# ------------------------------------------------------------------------------------
def _rng(name, seed, what):
    return np.random.default_rng([zlib.crc32(name.encode()), seed, what])


def _nonzero(rng, top, shape):
    x = rng.integers(-top, top + 1, shape)
    x[x == 0] = 1
    return x


@functools.lru_cache(maxsize=4)
def operands(name, seed=GPU_SEED):
    """ID[n_col] (n_cell x n_col, signed, no zero: every entry has weight in the variant pass) and, per
    cell operand, GT (n_var x n_col x 1, positive) and the three psi tables (1 or n_var rows).  The
    per-variant tables are pairwise different everywhere (residues 0, 1, 2 of 3), so the factors of
    AD, BD and DP the device forms from them (psi1 - psis, psi2 - psis, psi1 - psi2) never vanish."""
    (N, M) = merged(CASES[name].data)[0]
    op = SimpleNamespace(ID={}, cell={})
    for K in N_COLS:
        op.ID[K] = _nonzero(_rng(name, seed, K), ID_TOP, (M, K)).astype(np.float64)
    for what, (tag, K, unit) in enumerate(CELL_OPS):
        rng = _rng(name, seed, 100 + what)
        GT = rng.integers(1, GT_TOP + 1, (N, K, 1)).astype(np.float64)
        if unit is None:
            base = rng.integers(-PSI_TOP // 3, PSI_TOP // 3, (3, N, 1))
            psi = [(3 * base[i] + i).astype(np.float64) for i in range(3)]
        else:
            psi = [np.full((1, 1), float(u)) for u in unit]
        op.cell[tag] = (GT, psi)
    return op


def _weights(GT, psi):
    g = GT[:, :, 0].astype(np.int64)
    return [g * p.astype(np.int64) for p in psi]


def products(m, op):
    """name -> int64 matrix: ("reads", n_col) -> (AD @ ID, DP @ ID); ("cell", tag) -> AD.T @ W1 +
    (DP - AD).T @ W2 - DP.T @ Ws with W = GT x psi (the unit settings leave AD.T @ GT, (DP - AD).T @ GT
    and DP.T @ GT)"""
    AD, DP = matrices(m)
    BD = DP - AD
    out = {}
    for K, ID in op.ID.items():
        I = ID.astype(np.int64)
        out["reads", K] = (AD @ I, DP @ I)
    for tag, (GT, psi) in op.cell.items():
        w1, w2, ws = _weights(GT, psi)
        out["cell", tag] = AD.T @ w1 + BD.T @ w2 - DP.T @ ws
    return out


def magnitudes(m, op):
    """the largest sum of |weight| x |count| over an output cell, per orientation, over every grouping a
    pass may use: the variant pass adds AD, BD or DP counts against ID; the cell pass adds AD against
    psi1 - psi2 or psi1 - psis and DP or BD against psi2 - psis.  Below 2^53 every partial sum of every
    order is an integer float64 holds exactly."""
    AD, DP = matrices(m)
    A, B, D = abs(AD), abs(DP - AD), abs(DP)
    top_v = top_c = 0
    for ID in op.ID.values():
        I = np.abs(ID).astype(np.int64)
        top_v = max(top_v, int(((A + B + D) @ I).max(initial=0)))
    for GT, psi in op.cell.values():
        w1, w2, ws = _weights(GT, psi)
        fa = np.abs(w1 - w2) + np.abs(w1 - ws)
        fb = np.abs(w2 - ws)
        top_c = max(top_c, int((A.T @ fa + (B + D).T @ fb).max(initial=0)))
    return top_v, top_c


def count_cells(prods):
    return sum(sum(x.size for x in v) if isinstance(v, tuple) else v.size for v in prods.values())


def mismatches(got, want):
    """the number of cells of a float64 result that differ from the int64 product (no tolerance)"""
    want = np.asarray(want)
    got = np.asarray(got).reshape(want.shape)
    return int(np.count_nonzero(got != want.astype(np.float64)))


# ------------------------------------------------------------------------------------
# planted defects: what a builder could do to the input, done to a copy of it
# ------------------------------------------------------------------------------------
def _copy(m):
    shape, colptr, rowidx, ad, dp = m
    return [shape, colptr.copy(), rowidx.copy(), ad.copy(), dp.copy()]


def _pick(rng, ok):
    at = np.flatnonzero(ok)
    return None if at.size == 0 else int(at[rng.integers(at.size)])


def _remove(m, e):
    shape, colptr, rowidx, ad, dp = _copy(m)
    colptr[np.searchsorted(colptr, e, side="right"):] -= 1
    return shape, colptr, np.delete(rowidx, e), np.delete(ad, e), np.delete(dp, e)


def d_dropped(m, rng):
    e = _pick(rng, (m[3] != 0) | (m[4] != 0))
    return None if e is None else _remove(m, e)


def d_doubled(m, rng):
    e = _pick(rng, (m[3] != 0) | (m[4] != 0))
    if e is None:
        return None
    out = _copy(m)
    out[3][e] *= 2
    out[4][e] *= 2
    return tuple(out)


def d_rows_swapped(m, rng):
    """two neighbouring entries of a column exchange their row indices (their values change rows)"""
    _, colptr, rowidx, ad, dp = m
    same_col = np.ones(max(rowidx.size - 1, 0), bool)
    same_col[colptr[1:-1][(colptr[1:-1] > 0) & (colptr[1:-1] < rowidx.size)] - 1] = False
    e = _pick(rng, same_col & ((ad[:-1] != ad[1:]) | (dp[:-1] != dp[1:])))
    if e is None:
        return None
    out = _copy(m)
    out[3][[e, e + 1]] = out[3][[e + 1, e]]
    out[4][[e, e + 1]] = out[4][[e + 1, e]]
    return tuple(out)


def d_ad_dp_exchanged(m, rng):
    e = _pick(rng, m[3] != m[4])
    if e is None:
        return None
    out = _copy(m)
    out[3][e], out[4][e] = m[4][e], m[3][e]
    return tuple(out)


def d_last_lost(m, rng):
    """the last entry of the last (non-empty) variant row"""
    _, _, rowidx, ad, dp = m
    if rowidx.size == 0:
        return None
    e = int(np.flatnonzero(rowidx == rowidx.max())[-1])
    assert ad[e] != 0 or dp[e] != 0, "the last entry of the last row is an explicit zero: it has no weight"
    return _remove(m, e)


def d_wrapped_2048(m, rng):
    """a count of 2048 kept in 11 bits"""
    if not ((m[3] == 2048).any() or (m[4] == 2048).any()):
        return None
    out = _copy(m)
    out[3][out[3] == 2048] = 0
    out[4][out[4] == 2048] = 0
    return tuple(out)


DEFECTS = {"dropped": d_dropped, "doubled": d_doubled, "rows_swapped": d_rows_swapped,
           "ad_dp_exchanged": d_ad_dp_exchanged, "last_lost": d_last_lost, "wrapped_2048": d_wrapped_2048}


def differs(a, b):
    """does any product of two inputs differ"""
    for k, v in a.items():
        pa, pb = (v, b[k]) if isinstance(v, tuple) else ((v,), (b[k],))
        if any(not np.array_equal(x, y) for x, y in zip(pa, pb)):
            return True
    return False
