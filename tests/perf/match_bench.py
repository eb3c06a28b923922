"""Genotype distance (genotype_distance / vrx_geno_dist) at the sizes of a donor-matching run, n_GT = 3:
a pool of 16 donors against 16, 256 and 2 048 genotyped individuals.  Per shape, after a warm-up call, the
median over the repeats of
  kernel_ms     the library's ms_out: hipEvents around the pass and the sum of every slab
  wall_s        host clock around the whole call, upload of both operands included
and the kernel's share of its two bounds: the algorithmic bytes 8 n_GT n_var (k1 + k2) over the 8 TB/s HBM
figure, and 2 n_var k1 k2 n_GT fp64 VALU operations (a subtraction and an add per term) over the 78.6
TFLOP/s fp64 vector figure the other roofline lines use (that figure counts a fused multiply-add as two:
a stream of plain adds can reach half of it).
Baseline: optimal_match, the host double loop, on the same machine, timed ONCE (no warm-up, no repeat): in
full at the first shape; at the other two a 16 x 8 block of donor pairs, scaled by the number of pairs
(host_scaled_from_pairs).
A shape whose operands do not fit the host's available memory (the largest holds a 49 GB panel) is recorded
as not run, with the reason, and 1 000 000 x 16 x 512 -- still many default slabs -- is measured in its place.
One JSON line; --out FILE writes it too.

    python tests/perf/match_bench.py [--reps R] [--shapes 100000x16x16,100000x16x256,1000000x16x2048] [--out FILE]
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from vireo_amd import _lib, optimal_match                          # noqa: E402
from vireo_amd.vireo_base import _geno_dist                        # noqa: E402

HBM_B_S = 8.0e12
FP64_VALU_OP_S = 78.6e12
G = 3
FALLBACK = (1000000, 16, 512)   # measured when a shape does not fit the host's memory
BASE = 20000                    # larger panels repeat this many variants (the values do not change the work)


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def panel(seed, n_var, k):
    P = np.random.RandomState(seed).dirichlet(np.ones(G), size=(min(n_var, BASE), k))
    if n_var > BASE:
        P = np.tile(P, (-(-n_var // BASE), 1, 1))[:n_var]
    return np.ascontiguousarray(P)


def host_available_bytes():
    with open("/proc/meminfo") as f:
        for line in f:
            if line.startswith("MemAvailable:"):
                return int(line.split()[1]) * 1024
    return None


def main():
    reps = int(arg("--reps", 5))
    shapes = [tuple(int(v) for v in s.split("x"))
              for s in arg("--shapes", "100000x16x16,100000x16x256,1000000x16x2048").split(",")]
    _lib.require_gpu()
    rows = []
    queue = list(shapes)
    while queue:
        n_var, k1, k2 = queue.pop(0)
        need, have = 8.0 * G * n_var * (k1 + k2), host_available_bytes()
        if have is not None and 1.25 * need > have:     # (np.tile holds one more base block on the way)
            rows.append(dict(n_var=n_var, k1=k1, k2=k2, n_GT=G, operand_gb=need * 1e-9, not_run=(
                "the operands need %.1f GB of host memory, %.1f GB are available" % (need * 1e-9, have * 1e-9))))
            if FALLBACK not in shapes and FALLBACK not in queue:
                queue.append(FALLBACK)
            continue
        X, Z = panel(1, n_var, k1), panel(2, n_var, k2)
        ms, wall = [], []
        for r in range(reps + 1):                                  # the first call is a warm-up
            t = time.perf_counter()
            D, kernel_ms = _geno_dist(X, Z)
            w = time.perf_counter() - t
            if r:
                ms.append(kernel_ms)
                wall.append(w)
        # the host loop: every pair at the first shape, else a 16 x 8 block scaled by the pair count
        full = (k1 * k2 <= 256)
        kz = k2 if full else 8
        t = time.perf_counter()
        _, _, Dh = optimal_match(X, Z[:, :kz], return_delta=True)
        host_s = (time.perf_counter() - t) * (k1 * k2) / (k1 * kz)
        assert np.allclose(D[:, :kz], Dh, rtol=1e-9, atol=0)
        med = float(np.median(ms)) * 1e-3
        t_bytes = 8.0 * G * n_var * (k1 + k2) / HBM_B_S
        t_ops = 2.0 * n_var * k1 * k2 * G / FP64_VALU_OP_S
        rows.append(dict(
            n_var=n_var, k1=k1, k2=k2, n_GT=G, operand_gb=8.0 * G * n_var * (k1 + k2) * 1e-9, reps=reps,
            kernel_ms=dict(median=med * 1e3, min=float(min(ms)), max=float(max(ms))),
            wall_s=dict(median=float(np.median(wall)), min=float(min(wall)), max=float(max(wall))),
            bound_bytes_ms=t_bytes * 1e3, bound_fp64_valu_ms=t_ops * 1e3,
            kernel_share_of_bytes_bound=t_bytes / med, kernel_share_of_fp64_valu_bound=t_ops / med,
            host_optimal_match_s=host_s, host_scaled_from_pairs=None if full else [k1, kz],
            speedup_wall_vs_host=host_s / float(np.median(wall))))
        del X, Z
    out = dict(workload="genotype_distance, n_GT=3, operands on the host, default slabs",
               device=_lib.device_info(0)["name"], hbm_b_per_s=HBM_B_S, fp64_valu_op_per_s=FP64_VALU_OP_S, shapes=rows)
    line = json.dumps(out)
    print(line)
    if "--out" in sys.argv:
        with open(arg("--out", ""), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
