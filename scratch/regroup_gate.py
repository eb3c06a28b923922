"""Gate for regrouping the rows of a tile into rounds AFTER the balanced-slab greedy (CPU only, no GPU).

A round of the LDS passes costs, in every slab, its longest row rounded up to whole trips of 4 words.  Which 16
rows share a round is decided by `tile_layout` before the greedy runs ("dealt by length") and is blind to the
+-2 words of noise the greedy leaves; the format does not care (rowmap carries the placement), so a regrouping
changes the trips a wave stores and executes and no bit of any result.  This script prices it on c3-shaped
tiles built by the real host builder: `tile_layout`'s rule for the rows of a tile, `vrx_balance_tile` (the
specification of the greedy, called in the built library) for the slabs, FORM 1 word counts per entry.

    python scratch/regroup_gate.py [tiles, default "0,16"] [random exchange steps, default 200000] [cell | variant]

Prints, per tile: stored / executed slots per word as built, after the bounded deterministic exchange sweeps
a build could afford, and after a long random pairwise-exchange search (what any cheap rule is bounded by).
Gate: stored trips must fall by >= 3 % for the device version to be worth building."""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from vireo_amd import synth  # noqa: E402

G, U, WAVES, RW, SLAB_ROWS, MAX_BLOCK = 16, 4, 16, 96, 512, 64
NR = RW // G


def form1_words(v):
    """vrx_form1_words (vrx_balance.h): entries of at most three significant bits, largest first"""
    v = np.abs(v.astype(np.int64))
    n = np.zeros(v.shape, np.int64)
    while np.any(v != 0):
        nz = v != 0
        ln = np.zeros(v.shape, np.int64)
        ln[nz] = np.floor(np.log2(v[nz])).astype(np.int64) + 1
        sh = np.maximum(ln - 3, 0)
        v = np.where(nz, v - ((v >> sh) << sh), 0)
        n += nz
    return n


def greedy_fn():
    lib = os.environ.get("VIREO_LIB", os.path.join(ROOT, "vireo_amd", "libvireo_hip.so"))
    names = [l.split()[-1] for l in subprocess.run(["nm", "-D", lib], capture_output=True, text=True,
                                                   check=True).stdout.splitlines() if "vrx_balance_tile" in l]
    assert len(names) == 1, names
    fn = getattr(C.CDLL(lib), names[0])
    fn.restype = None
    vp = C.c_void_p
    fn.argtypes = [vp, C.c_int64, vp, vp, vp, C.c_int64, C.c_int, C.c_int, C.c_int, vp, vp]
    return fn


def tile_rows(ptr, tile):
    """tile_layout (vrx_engine.hip) for rows that are not cut into pieces: rows by length, descending and stable,
    16 at a time to the waves in snake order, stratum j = round j.  -> rows of the tile in position order"""
    n = ptr.size - 1
    order = np.argsort(-(ptr[1:] - ptr[:-1]), kind="stable")
    n_tile = -(-n // (WAVES * RW))
    n_wave = n_tile * WAVES
    rowmap = np.full(n_wave * RW, -1, np.int64)
    for u in range(-(-n // G)):
        j, i = divmod(u, n_wave)
        w = n_wave - 1 - i if j & 1 else i
        rows = order[u * G:(u + 1) * G]
        rowmap[w * RW + j * G:w * RW + j * G + rows.size] = rows
    return rowmap[tile * WAVES * RW:(tile + 1) * WAVES * RW], n_tile


def cost(Lr):
    """Lr: (rounds, 16, slabs) word counts -> (stored trips, sum of the rounds' longest rows)"""
    m = Lr.max(1)
    return int(((m + U - 1) // U).sum()), int(m.sum())


def exchange_gain(A, B):
    """best single exchange (row i of round A <-> row j of round B): (gain in trips, gain in sum max, i, j)"""
    def wo(X):      # the round's longest row per slab without row i: (16, slabs)
        s = np.sort(X, 0)
        m1, m2 = s[-1], s[-2]
        return np.where(X == m1, np.where((X == m1).sum(0) > 1, m1, m2), m1)
    a_wo, b_wo = wo(A), wo(B)
    na = np.maximum(a_wo[:, None, :], B[None, :, :])         # A without i, with B's j
    nb = np.maximum(b_wo[None, :, :], A[:, None, :])         # B without j, with A's i
    trips = ((na + U - 1) // U).sum(2) + ((nb + U - 1) // U).sum(2)
    summ = na.sum(2) + nb.sum(2)
    t0 = ((A.max(0) + U - 1) // U).sum() + ((B.max(0) + U - 1) // U).sum()
    s0 = A.max(0).sum() + B.max(0).sum()
    key = (t0 - trips) * 100000 + (s0 - summ)
    i, j = np.unravel_index(np.argmax(key), key.shape)
    return int(t0 - trips[i, j]), int(s0 - summ[i, j]), int(i), int(j)


def sweeps(Lr, n_sweep):
    """bounded, deterministic: sweep s pairs round r of wave w with round r of wave w + k_s (round r holds the
    r-th stratum of the rows by length: other strata have other lengths) and applies the best single exchange of
    the pair if it lowers (trips, sum max); R * 256 * slabs operations per sweep, 15 sweeps = every pair once"""
    Lr = Lr.copy()
    R = Lr.shape[0]
    hist = []
    for s in range(n_sweep):
        stride = NR * (1 + (s * 4) % (WAVES - 1))
        for a in range(R):
            b = (a + stride) % R
            if a == b:
                continue
            dt, ds, i, j = exchange_gain(Lr[a], Lr[b])
            if dt > 0 or (dt == 0 and ds > 0):
                Lr[a, i], Lr[b, j] = Lr[b, j].copy(), Lr[a, i].copy()
        hist.append(cost(Lr))
    return Lr, hist


def random_search(Lr, steps, seed=1):
    Lr = Lr.copy()
    rng = np.random.default_rng(seed)
    R = Lr.shape[0]
    per = np.array([[((Lr[r].max(0) + U - 1) // U).sum(), Lr[r].max(0).sum()] for r in range(R)])
    for _ in range(steps):
        a, b = rng.integers(0, R, 2)
        if a == b:
            continue
        i, j = rng.integers(0, G, 2)
        ga, gb = Lr[a].copy(), Lr[b].copy()
        ga[i], gb[j] = Lr[b, j], Lr[a, i]
        ca = (((ga.max(0) + U - 1) // U).sum(), ga.max(0).sum())
        cb = (((gb.max(0) + U - 1) // U).sum(), gb.max(0).sum())
        old = (per[a, 0] + per[b, 0]) * 4 + 0.25 * (per[a, 1] + per[b, 1])
        new = (ca[0] + cb[0]) * 4 + 0.25 * (ca[1] + cb[1])
        if new < old:
            Lr[a], Lr[b], per[a], per[b] = ga, gb, ca, cb
    return Lr


def virtual_rows(N, M, colptr, rowidx, ad, dp):
    """the variant pass's rows (derive_virtual_rows, vrx_engine.hip): row 2 n = the AD counts of variant n, row
    2 n + 1 its BD = DP - AD counts; contracted index = cell >> 1 (a pair of cells, one half row each)"""
    cell = np.repeat(np.arange(M, dtype=np.int64), np.diff(colptr))
    P = (M + 1) // 2
    keys, wds = [], []
    for kind, v in ((0, ad), (1, dp - ad)):
        m = v != 0
        keys.append((2 * rowidx[m].astype(np.int64) + kind) * P + (cell[m] >> 1))
        wds.append(form1_words(v[m]))
    key, wd = np.concatenate(keys), np.concatenate(wds)
    del keys, wds, cell
    o = np.argsort(key, kind="stable")
    key, wd = key[o], wd[o]
    first = np.flatnonzero(np.r_[True, key[1:] != key[:-1]])
    words = np.add.reduceat(wd, first)
    key = key[first]
    ptr = np.zeros(2 * N + 1, np.int64)
    np.cumsum(np.bincount(key // P, minlength=2 * N), out=ptr[1:])
    return ptr, np.ascontiguousarray(key % P, np.int32), words, P


def main():
    tiles = [int(x) for x in (sys.argv[1] if len(sys.argv) > 1 else "0,16").split(",")]
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 200000
    which = sys.argv[3] if len(sys.argv) > 3 else "cell"
    N, M, K, dens = synth.CONFIGS[os.environ.get("GATE_CONFIG", "c3")]
    w = bench.donor_workload(N, M, K, dens, seed=0)
    ptr = np.asarray(w["colptr"], np.int64)                  # cell pass: rows = cells, contracted = variants
    idx = np.ascontiguousarray(w["rowidx"], np.int32)
    ad, dp = np.asarray(w["ad"], np.int64), np.asarray(w["dp"], np.int64)
    if which == "variant":
        ptr, idx, words, n_contract = virtual_rows(N, M, ptr, idx, ad, dp)
        M, N = 2 * N, n_contract                             # (rows, contracted)
    else:
        words = form1_words(ad) + form1_words(dp - ad)
    words = np.minimum(words, 255).astype(np.uint8)
    n_slab = -(-N // SLAB_ROWS)
    fn = greedy_fn()
    print("%s stream of %s: %d rows x %d contracted, %d slabs of %d, %.3f words per entry"
          % (which, os.environ.get("GATE_CONFIG", "c3"), M, N, n_slab, SLAB_ROWS, words.sum() / words.size), flush=True)
    for tile in tiles:
        pos_rows, n_tile = tile_rows(ptr, tile)
        rows = np.ascontiguousarray(pos_rows[pos_rows >= 0], np.int32)
        posmap = np.full(N, -1, np.int32)
        perm = np.zeros(n_slab * SLAB_ROWS, np.int32)
        t0 = time.time()
        fn(rows.ctypes.data, rows.size, ptr.ctypes.data, idx.ctypes.data, words.ctypes.data, N, n_slab, SLAB_ROWS,
           MAX_BLOCK, posmap.ctypes.data, perm.ctypes.data)
        t_greedy = time.time() - t0
        L = np.zeros((WAVES * RW, n_slab), np.int64)         # words of tile position p in slab s
        for p, r in enumerate(pos_rows):
            if r >= 0:
                e = slice(ptr[r], ptr[r + 1])
                np.add.at(L[p], posmap[idx[e]] // SLAB_ROWS, words[e])
        total = L.sum()
        Lr = L.reshape(WAVES * NR, G, n_slab)                # position = wave * RW + round * G + group
        t_b, s_b = cost(Lr)
        print("tile %d of %d (%d rows, greedy %.1f s): %d words; as built: stored %.4f executed %.4f slots per word"
              % (tile, n_tile, rows.size, t_greedy, total, t_b * U * G / total, s_b * G / total), flush=True)
        t0 = time.time()
        _, hist = sweeps(Lr, 15)
        for s in (0, 1, 3, 7, 14):
            print("   %2d deterministic sweeps: stored %.4f (%+.2f %%) executed %.4f (%+.2f %%)"
                  % (s + 1, hist[s][0] * U * G / total, (hist[s][0] / t_b - 1) * 100,
                     hist[s][1] * G / total, (hist[s][1] / s_b - 1) * 100))
        print("   (%.1f s for 15 sweeps in numpy)" % (time.time() - t0), flush=True)
        if steps:
            t0 = time.time()
            t_r, s_r = cost(random_search(Lr, steps))
            print("   random exchange search, %d steps (%.0f s): stored %.4f (%+.2f %%) executed %.4f (%+.2f %%)"
                  % (steps, time.time() - t0, t_r * U * G / total, (t_r / t_b - 1) * 100, s_r * G / total,
                     (s_r / s_b - 1) * 100), flush=True)


if __name__ == "__main__":
    main()
