"""NumPy restatement of the greedy barcode selection (variant_select / barcode_entropy of the reference,
vireoSNP/utils/variant_select.py:5-62), the seeded cases of tests/golden/c1_barcode.npz and the GTbarcode
runs of tests/golden/barcode/.  What the device pass is held to, bit for bit.

The reference decides by float equality on entropy(Z_cnt / sum(Z_cnt), base=2) with Z_cnt in np.unique's
order of the barcode strings, so the order of the terms is part of the behaviour:
  classes   single-character categories: every barcode of a round has the same length, so string order is
            the order of (class rank, value); after a choice the new rank is the dense rank of that pair
  terms     the non-empty bins c(class, value) of a variant, class-major and value-minor
  sums      np.sum of a contiguous float64 array of n <= 128 terms (np_sum_rule)
  entropy   p = c / K; s = sum(p); q = p / s; sum(entr(q)) / log(2)
"""
import os

import numpy as np
from scipy.special import entr

HERE = os.path.dirname(os.path.abspath(__file__))
BITS_ONE = np.float64(1.0).view(np.int64)
LOG2 = np.log(2)
MAX_DONORS = 128


def np_sum_rule(A, n):
    """np.sum of the first n entries of every row of A (float64, n <= 128): below 8 terms one after the
    other from 0.0; else eight accumulators over the blocks of 8, combined pairwise, then the last n % 8."""
    A = np.asarray(A, dtype=np.float64)
    assert 0 <= n <= 128
    if n < 8:
        res = np.zeros(A.shape[0])
        for i in range(n):
            res = res + A[:, i]
        return res
    r = [A[:, j].copy() for j in range(8)]
    n8 = n - n % 8
    for i in range(8, n8, 8):
        for j in range(8):
            r[j] = r[j] + A[:, i + j]
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for i in range(n8, n):
        res = res + A[:, i]
    return res


def rows_sum(A, n_terms):
    """np_sum_rule per row with its own number of leading terms"""
    out = np.empty(A.shape[0])
    for n in np.unique(n_terms):
        sel = np.flatnonzero(n_terms == n)
        out[sel] = np_sum_rule(A[sel], int(n))
    return out


def dense_rank(rank, values):
    """the class ranks after a chosen variant: the dense rank of (rank, value)"""
    key = np.asarray(rank, dtype=np.int64) * 16 + np.asarray(values, dtype=np.int64)
    return np.unique(key, return_inverse=True)[1].astype(np.int64)


def class_state(rank):
    """(donors in class order, class boundaries): what a round sends to the device"""
    rank = np.asarray(rank)
    order = np.argsort(rank, kind="stable").astype(np.int32)
    n_class = int(rank.max()) + 1
    bnd = np.searchsorted(rank[order], np.arange(n_class + 1)).astype(np.int32)
    return order, bnd


def ordered_counts(GT, rank, order_blind=False):
    """per variant its terms, left-aligned: (counts [n_var][<= K], number of terms)"""
    GT = np.asarray(GT, dtype=np.int64)
    n_var, K = GT.shape
    n_cat = int(GT.max()) + 1 if GT.size else 1
    n_class = int(np.max(rank)) + 1
    bins = np.zeros((n_var, n_class * n_cat), dtype=np.int64)
    rows = np.arange(n_var)
    for k in range(K):
        np.add.at(bins, (rows, rank[k] * n_cat + GT[:, k]), 1)
    if order_blind:
        bins = np.sort(bins, axis=1)
    n_terms = (bins > 0).sum(1)
    first = np.argsort(bins == 0, axis=1, kind="stable")[:, :K]      # the non-empty bins, in order
    return np.take_along_axis(bins, first, 1), n_terms


def entropies(GT, rank, order_blind=False):
    """(entropy, j) per variant: j = bits(s) - bits(1.0) of the normalising sum"""
    K = np.asarray(GT).shape[1]
    cnt, n_terms = ordered_counts(GT, rank, order_blind)
    p = cnt.astype(np.float64) / np.float64(K)
    s = rows_sum(p, n_terms)
    q = p / s[:, None]
    S = rows_sum(entr(q), n_terms)
    return S / LOG2, s.view(np.int64) - BITS_ONE


def entr_table(K, half_width):
    """T[j + H][c] = entr((c / K) / s_j), s_j the double whose bit pattern is bits(1.0) + j"""
    j = np.arange(-half_width, half_width + 1, dtype=np.int64)
    s = (BITS_ONE + j).view(np.float64)
    p = np.arange(K + 1, dtype=np.float64) / np.float64(K)
    return np.ascontiguousarray(entr(p[None, :] / s[:, None]))


def median_np(values):
    """np.median of a 1-D array in words: the middle one, or (a + b) / 2 of the two middle ones"""
    v = np.sort(np.asarray(values, dtype=np.float64))
    n = len(v)
    return v[n // 2] if n % 2 else (v[n // 2 - 1] + v[n // 2]) / 2


def select(GT, var_count=None, rand_seed=0, order_blind=False, rng=None):
    """The whole selection with every round recorded.  Draws from np.random (seeded here) unless rng is
    given.  Returns dict(ent [rounds][n_var], tied, kept, chosen, final, barcodes, lines, j_range)."""
    GT = np.asarray(GT)
    n_var, K = GT.shape
    if rng is None:
        np.random.seed(rand_seed)
        rng = np.random
    rank = np.zeros(K, dtype=np.int64)
    barcodes = ["#"] * K
    now = 0
    rec = dict(ent=[], tied=[], kept=[], chosen=[], lines=[], j_lo=0, j_hi=0)
    while True:
        ent, j = entropies(GT, rank, order_blind)
        rec["ent"].append(ent)
        rec["j_lo"], rec["j_hi"] = min(rec["j_lo"], int(j.min())), max(rec["j_hi"], int(j.max()))
        top = np.max(ent)
        if top == now:
            break
        idx = np.flatnonzero(top == ent)
        rec["tied"].append(len(idx))
        if var_count is not None:
            idx = idx[var_count[idx] >= median_np(var_count[idx])]
        rec["kept"].append(len(idx))
        rec["lines"].append("Randomly select 1 more variants out %d" % len(idx))
        use = idx[rng.randint(len(idx))]
        rec["chosen"].append(int(use))
        barcodes = [b + str(int(g)) for b, g in zip(barcodes, GT[use])]
        rank = dense_rank(rank, GT[use])
        now = ent[use]
    if now < np.log2(K):
        rec["lines"].append("Warning: variant_select can't distinguish all samples.")
    rec.update(ent=np.array(rec["ent"]), final=now, barcodes=barcodes)
    return rec


# ---- the seeded cases of tests/golden/c1_barcode.npz -------------------------------------------
# name -> (kind, K, n_var, categories, seed, with var_count)
CASES = {}
for _seed in (1, 2, 4, 6, 8, 9):           # the inputs on which an order-blind entropy changes the result
    CASES["k10_s%d_vc" % _seed] = ("uniform", 10, 300, 3, _seed, True)
    CASES["k10_s%d" % _seed] = ("uniform", 10, 300, 3, _seed, False)
for _K in (1, 2, 7, 8, 9, 16, 17, 127, 128):
    CASES["k%d" % _K] = ("uniform", _K, 300, 3, 3, True)
CASES["cat2"] = ("uniform", 12, 300, 2, 5, True)
CASES["cat10"] = ("uniform", 12, 300, 10, 5, True)
CASES["cat10_novc"] = ("uniform", 24, 200, 10, 6, False)
CASES["sparse"] = ("sparse", 24, 400, 3, 7, True)
CASES["monomorphic"] = ("mono", 5, 50, 3, 0, True)
CASES["twins"] = ("twins", 6, 120, 3, 11, True)
ORDER_SENSITIVE = ["k10_s%d%s" % (s, v) for s in (1, 2, 4, 6, 8, 9) for v in ("_vc", "")]
FIXTURE_KEYS = ("ent", "tied", "kept", "chosen", "final", "barcodes", "lines", "rng_key", "rng_pos")


def case_input(name):
    """(GT int64 [n_var][K], var_count float64 or None)"""
    kind, K, n_var, n_cat, seed, with_vc = CASES[name]
    rs = np.random.RandomState(1000 * K + seed)
    if kind == "sparse":
        GT = rs.randint(1, n_cat, (n_var, K)) * (rs.rand(n_var, K) < 0.1)
    else:
        GT = rs.randint(0, n_cat, (n_var, K))
    vc = rs.randint(21, 200, n_var).astype(float)
    if kind == "mono":
        GT[:] = 1
    if kind == "twins":
        GT[:, 4] = GT[:, 1]                 # two donors that no variant tells apart
    return GT, (vc if with_vc else None)


def fixture_case(fixture, name):
    return {key: fixture["%s_%s" % (name, key)] for key in FIXTURE_KEYS}


# ---- past the grid cap of the maximum --------------------------------------------------------------
# vrx_barcode_max launches at most VRX_BC_MAX_BLOCKS blocks of VRX_BC_BLOCK threads (csrc/vrx_barcode.h: 1024
# x 256) and strides beyond; vrx_barcode_max2 then takes 1 024 partials, four per thread.
BC_GRID = 1024 * 256
CAPPED_SIZES = (BC_GRID + 1, 2 * BC_GRID + 3)          # the second and the third sweep
CAPPED_DONORS = (2, 9)


def capped_case(n_var, K):
    """(GT, var_count) of three categories whose first two rounds decide past the cap.
    Round 1: the one maximum is the LAST variant, which only a strided sweep reaches (every other variant
    holds fewer categories, or the same ones less evenly).  Round 2, once that variant is chosen: the tie
    set has members on both sides of index BC_GRID and the median of var_count decides between them.
    K = 9: six planted variants whose pattern splits every class of the chosen one; K = 2: the chosen
    variant tells both donors apart, so every variant ties."""
    rs = np.random.RandomState(7 * K + n_var % 1000)
    vc = rs.randint(21, 200, n_var).astype(float)
    if K == 2:
        GT = np.repeat(rs.randint(0, 3, (n_var, 1)), 2, axis=1)      # (a, a): entropy 0
        GT[-1] = [0, 1]
        vc[-1] = 250.0                                               # (kept by any median of these counts)
        return GT, vc
    assert K == 9
    GT = rs.randint(0, 2, (n_var, K))                                 # two categories: at most 1 bit
    GT[-1] = [0, 0, 0, 1, 1, 1, 2, 2, 2]                              # log2(3) bits, alone
    # (at BC_GRID + 1 variants the only index past the cap is the chosen variant's own: the six stay below)
    past = [BC_GRID, BC_GRID + 6, n_var - 2] if n_var > BC_GRID + 8 else [BC_GRID - 4, BC_GRID - 3, BC_GRID - 2]
    planted = [5, 100000, BC_GRID - 1] + past
    GT[planted] = [0, 1, 2, 0, 1, 2, 0, 1, 1]                         # uneven now, eight bins of nine next round
    vc[planted] = [1.0, 9.0, 2.0, 8.0, 3.0, 7.0]                      # median 5: survivors 100000 and past[0], past[2]
    return GT, vc


# ---- the GTbarcode runs of tests/golden/barcode/<run>/ -------------------------------------------
BARCODE_VCF = os.path.join(HERE, "golden", "data", "donors.cellSNP.vcf.gz")
BARCODE_RUNS = {
    "seed0": ["--randSeed", "0"],
    "seed1": ["--randSeed", "1"],
    "seed7": ["--randSeed", "7"],
    "seed1_noHomoAlt_PL": ["--randSeed", "1", "--noHomoAlt", "-t", "PL"],
    "seed3_GT": ["--randSeed", "3", "-t", "GT"],
}


def barcode_run_dir(run):
    return os.path.join(HERE, "golden", "barcode", run)
