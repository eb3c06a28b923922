"""Per-variant clone mixtures (variant_mixture_gain / vrx_varmix_*) at three shapes, variants x cells:
  2000x20000      depth ~20, every cell covered with probability 0.5
  500x200000      depth ~50, every cell covered: the clone-mode shape, every row fitted by a workgroup
  50000x5000      sparse: a cell covers a variant with probability 0.02, depth ~5; every row fitted by a wave
A tenth of the rows carry a planted two-level clone, the rest are one allele rate.  K = 2, the defaults of the
function (max_iter 200, min_iter 20, epsilon_conv 1e-2).  Per shape, after a warm-up call, the median over the
repeats of
  wall_s        host clock around variant_mixture_gain: merge of the counts, CSR build, upload, fit, download
  fit_wall_s    host clock around VariantMixtures.fit on a resident handle
  kernel_ms     hipEvents around the one launch
  kernel_share_of_flop_bound
                a row of n entries that stops at iteration `it` is read by pass 0 and by it + 1 iteration passes.
                An iteration pass costs an entry about 3 K multiply-adds for L, K exp, one log, one division and
                5 K multiply-adds for the sums: FLOP_PER_ENTRY_K2 double operations at K = 2 (exp and log at 20
                each); pass 0 has no exp or log: 3 divisions and 2 K multiply-adds beside the start weights,
                FLOP_PASS0_K2.  The sum over the rows of n (FLOP_PASS0_K2 + (it + 1) FLOP_PER_ENTRY_K2) over the
                78.6 TFLOP/s vector fp64 figure is the bound; the entry bytes (8 per entry and pass) are far below
                the HBM figure and rows of this size stay in cache between passes
Baseline: the host loop of the NumPy restatement (tests/varmix_np.py, one variant at a time over its covered
cells), timed ONCE on SUBSET evenly spaced rows and scaled by the number of rows (host_scaled_from_subset).
The device's n_iter on that subset must equal the restatement's and the gains agree to 1e-5.
One JSON line; --out FILE writes it too (profiles/varmix_bench.json).

    python tests/perf/varmix_bench.py [--reps R] [--shapes 2000x20000,500x200000,sparse50000x5000] [--out FILE]
"""
import json
import os
import sys
import time

import numpy as np
from scipy.sparse import csr_matrix

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from vireo_amd import _lib, variant_mixture_gain, VariantMixtures    # noqa: E402
from tests import varmix_np as VN                                    # noqa: E402

FP64_FLOP_S = 78.6e12
FLOP_PER_ENTRY_K2 = 2 * (3 * 2) + 20 * 2 + 20 + 10 + 2 * (5 * 2)
FLOP_PASS0_K2 = 6 * 2 + 3 * 10 + 2 * (2 * 2) + 2
SUBSET = 24
K = 2
SHAPES = {"2000x20000": (2000, 20000, 0.5, 20), "500x200000": (500, 200000, 1.0, 50),
          "sparse50000x5000": (50000, 5000, 0.02, 5)}


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def counts(seed, n_var, n_cell, cover, depth):
    """CSR (AD, DP), row by row so that no dense n_var x n_cell array is ever formed"""
    rng = np.random.default_rng(seed)
    ptr, idx, ad, dp = [0], [], [], []
    for v in range(n_var):
        cells = np.flatnonzero(rng.random(n_cell) < cover) if cover < 1.0 else np.arange(n_cell)
        d = rng.poisson(depth, cells.size) + 1
        p = np.where(rng.random(cells.size) < 0.3, 0.3, 0.02) if v % 10 == 0 else np.full(cells.size, rng.choice([0.02, 0.1, 0.5]))
        idx.append(cells.astype(np.int32))
        dp.append(d.astype(np.int32))
        ad.append(rng.binomial(d, p).astype(np.int32))
        ptr.append(ptr[-1] + cells.size)
    idx, ptr = np.concatenate(idx), np.array(ptr, dtype=np.int64)
    return (csr_matrix((np.concatenate(ad), idx, ptr), shape=(n_var, n_cell)),
            csr_matrix((np.concatenate(dp), idx.copy(), ptr.copy()), shape=(n_var, n_cell)))


def main():
    reps = int(arg("--reps", 3))
    shapes = arg("--shapes", ",".join(SHAPES)).split(",")
    _lib.require_gpu()
    rows = []
    for k, spec in enumerate(shapes):
        n_var, n_cell, cover, depth = SHAPES[spec]
        AD, DP = counts(k + 1, n_var, n_cell, cover, depth)
        wall, fit_wall, kern = [], [], []
        vm = VariantMixtures(AD, DP)
        for r in range(reps + 1):                                    # the first round is a warm-up
            t = time.perf_counter()
            gain = variant_mixture_gain(AD, DP, n_clone=K)
            w = time.perf_counter() - t
            t = time.perf_counter()
            fit = vm.fit(n_clone=K)
            f = time.perf_counter() - t
            assert fit["gain"].tobytes() == gain.tobytes()
            if r:
                wall.append(w)
                fit_wall.append(f)
                kern.append(vm.kernel_ms)
        vm.close()
        sub = np.unique(np.linspace(0, n_var - 1, min(SUBSET, n_var)).astype(int))
        t = time.perf_counter()
        host = []
        for v in sub:
            a, d = AD[v].toarray().ravel(), DP[v].toarray().ravel()
            cov = d > 0
            r_ = VN.fit_row(a[cov], d[cov], K)
            host.append((r_["n_iter"], r_["elbo"] - VN.elbo_one(a[cov], d[cov]), abs(r_["elbo"])))
        host_s = (time.perf_counter() - t) * n_var / sub.size
        assert np.array_equal(fit["n_iter"][sub], [h[0] for h in host])
        assert np.all(np.abs(fit["gain"][sub] - [h[1] for h in host]) <= 1e-5 * np.maximum(1.0, [h[2] for h in host]))
        n_cov = fit["n_covered"].astype(np.float64)
        passes = float(np.sum(n_cov * (fit["n_iter"] + 1)))                  # iteration passes; pass 0 beside them
        t_flop = (passes * FLOP_PER_ENTRY_K2 + float(np.sum(n_cov)) * FLOP_PASS0_K2) / FP64_FLOP_S
        med_k = float(np.median(kern)) * 1e-3
        rows.append(dict(
            shape=spec, n_var=n_var, n_cell=n_cell, nnz=int(DP.nnz), depth=depth, n_clone=K, reps=reps,
            n_iter=dict(min=int(fit["n_iter"].min()), median=float(np.median(fit["n_iter"])), max=int(fit["n_iter"].max())),
            passed=int(np.sum(fit["gain"] > 0)),
            wall_s=dict(median=float(np.median(wall)), min=float(min(wall)), max=float(max(wall))),
            fit_wall_s=float(np.median(fit_wall)), kernel_ms=med_k * 1e3,
            iteration_entry_passes=passes, flop_bound_ms=t_flop * 1e3, kernel_share_of_flop_bound=t_flop / med_k,
            host_restatement_s=host_s, host_scaled_from_subset=[int(sub.size), n_var],
            speedup_wall_vs_host_restatement=host_s / float(np.median(wall)),
            speedup_kernel_vs_host_restatement=host_s / med_k))
        del AD, DP
    out = dict(workload="variant_mixture_gain, K = 2, default stop rule, counts on the host",
               device=_lib.device_info(0)["name"], fp64_flop_per_s=FP64_FLOP_S, shapes=rows)
    line = json.dumps(out)
    print(line)
    if "--out" in sys.argv:
        with open(arg("--out", ""), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
