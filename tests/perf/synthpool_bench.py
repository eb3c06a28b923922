"""Pooling four samples into one (pool_counts, vrx_pool.h).

Workload: the c3 counts of vireo_amd.synth (100 000 variants x 50 000 cells, ~1e8 entries) cut into four samples of
12 500 cells, pooled by pool_barcodes at its default doublet rate (n / 100 000 = 0.5 here: a third of the pooled
cells are pairs) and at rate 0.3 (about 23 000 of the 50 000 source cells end up in pairs).
Per rate, after a warm-up round, the median over the repeats of
  kernel_ms      hipEvents around the count, scan and emit kernels, sources resident (DevicePool.run)
  device_path_s  host clock around pool_counts(merged=True) on the merged samples: concatenation, upload, kernels,
                 download of the merged arrays
  wall_s         host clock around pool_counts on the merged samples, the two SciPy matrices included
  gb_per_s       the bytes the merge cannot avoid (12 per source entry read, 12 per pooled entry written) over
                 kernel_ms; the count pass reads the row indices of the pairs once more
Baselines on the host, timed once each, results compared with the device's: ``X_all @ P`` for AD and DP (SciPy's
CSC product, one thread), and ``X[:, a] + X[:, b]`` for the pairs beside ``X[:, s]`` for the others, stacked.  The
host's core count is stated; SciPy uses one.
One JSON line; --out FILE writes it too (profiles/synthpool_bench.json).

    python tests/perf/synthpool_bench.py [--reps R] [--rates default,0.3] [--config c3] [--out FILE]
"""
import json
import os
import sys
import time

import numpy as np
from scipy.sparse import csc_matrix, hstack

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from vireo_amd import _lib, synth                                    # noqa: E402
from vireo_amd import synth_pool as SP                               # noqa: E402

N_SAMPLE = 4


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def cut(w, n_sample):
    """the workload's columns as n_sample merged samples and their barcodes"""
    n_var, n_cell = w["shape"]
    each = n_cell // n_sample
    samples, barcodes = [], []
    for k in range(n_sample):
        c0, c1 = k * each, (k + 1) * each if k < n_sample - 1 else n_cell
        a, b = int(w["colptr"][c0]), int(w["colptr"][c1])
        samples.append(((n_var, c1 - c0), w["colptr"][c0:c1 + 1] - a, w["rowidx"][a:b], w["ad"][a:b], w["dp"][a:b]))
        barcodes.append(["CELL%07d-1" % i for i in range(c0, c1)])
    return samples, barcodes


def note(text):
    print("[synthpool_bench] %s" % text, file=sys.stderr, flush=True)


def bench_rate(samples, barcodes, AD, DP, rate, reps):
    out = SP.pool_barcodes(barcodes, None, rate, seed=1)
    plan = SP.pool_plan(barcodes, out)
    pairs = int(np.sum(plan.src1 >= 0))
    kern, path, wall = [], [], []
    pool = SP.DevicePool(samples)
    for r in range(reps + 1):                                        # the first round is a warm-up
        tm = {}
        pool.run(plan, timing=tm, download=False)
        if r:
            kern.append(tm["kernel_ms"])
    pool.close()
    note("rate %s: %d pooled cells, %d pairs, kernels %s ms" % (rate, plan.n_pool, pairs, ["%.2f" % x for x in kern]))
    for r in range(reps + 1):
        t = time.perf_counter()
        merged = SP.pool_counts(samples, plan, merged=True)
        d = time.perf_counter() - t
        t = time.perf_counter()
        gA, gD = SP.pool_counts(samples, plan)
        w = time.perf_counter() - t
        if r:
            path.append(d)
            wall.append(w)
    note("rate %s: device path %s s, wall %s s" % (rate, ["%.2f" % x for x in path], ["%.2f" % x for x in wall]))
    P = plan.matrix()
    t = time.perf_counter()
    wA, wD = (AD @ P).tocsc(), (DP @ P).tocsc()
    product_s = time.perf_counter() - t
    two = plan.src1 >= 0
    t = time.perf_counter()
    parts = []
    for X in (AD, DP):
        one = X[:, plan.src0[~two]]
        both = X[:, plan.src0[two]] + X[:, plan.src1[two]]
        order = np.argsort(np.concatenate([np.flatnonzero(~two), np.flatnonzero(two)]), kind="stable")
        parts.append(hstack([one, both], format="csc")[:, order])
    columns_s = time.perf_counter() - t
    note("rate %s: SciPy product %.2f s, column sums %.2f s" % (rate, product_s, columns_s))
    for got, want, alt in ((gA, wA, parts[0]), (gD, wD, parts[1])):
        want.eliminate_zeros()
        assert got.shape == want.shape and got.nnz == want.nnz and (got != want).nnz == 0
        assert (got != alt).nnz == 0
    lens = np.concatenate([np.diff(s[1]) for s in samples])
    src_entries = int(lens[plan.src0].sum() + lens[plan.src1[two]].sum())
    out_entries = int(merged[1][-1])
    med_k = float(np.median(kern))
    bytes_min = 12 * (src_entries + out_entries)
    return dict(doublet_rate="default" if rate is None else rate, source_cells=plan.n_src, pooled_cells=plan.n_pool,
                pairs=pairs, source_entries=src_entries, pooled_entries=out_entries, reps=reps, kernel_ms=med_k,
                kernel_ms_all=[float(x) for x in kern], gb_per_s=bytes_min / (med_k * 1e-3) / 1e9,
                device_path_s=float(np.median(path)),
                wall_s=dict(median=float(np.median(wall)), min=float(min(wall)), max=float(max(wall))),
                scipy_product_s=product_s, scipy_columns_s=columns_s,
                speedup_wall_vs_scipy_product=product_s / float(np.median(wall)),
                speedup_device_path_vs_scipy_product=product_s / float(np.median(path)),
                speedup_kernel_vs_scipy_product=product_s / (med_k * 1e-3))


def main():
    reps = int(arg("--reps", 3))
    rates = [None if x == "default" else float(x) for x in arg("--rates", "default,0.3").split(",")]
    cfg = arg("--config", "c3")
    _lib.require_gpu()
    w = synth.donor_workload(*synth.CONFIGS[cfg], seed=0)
    note("workload %s generated" % cfg)
    samples, barcodes = cut(w, N_SAMPLE)
    AD = csc_matrix((w["ad"].astype(np.int64), w["rowidx"], w["colptr"]), shape=w["shape"])
    DP = csc_matrix((w["dp"].astype(np.int64), w["rowidx"].copy(), w["colptr"].copy()), shape=w["shape"])
    rows = [bench_rate(samples, barcodes, AD, DP, rate, reps) for rate in rates]
    out = dict(workload="pool_counts: %s cut into %d samples, merged on the host, pooled by pool_barcodes(seed=1)"
               % (cfg, N_SAMPLE), shape=list(w["shape"]), entries=int(w["rowidx"].size),
               device=_lib.device_info(0)["name"], host_cores=len(os.sched_getaffinity(0)), scipy_threads=1,
               wave_limit=int(_lib.lib().vrx_pool_wave_limit()), rates=rows)
    line = json.dumps(out)
    print(line)
    if "--out" in sys.argv:
        with open(arg("--out", ""), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
