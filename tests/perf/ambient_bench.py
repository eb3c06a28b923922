"""Ambient-RNA step (predit_ambient) at the c3 shape, K = 16, planted donors: the split of one call
(ELBO gain, Dirichlet draws, compaction, EM kernel, download), cells per second, the iteration
histogram and the EM kernel's work against its fp64 vector bound.  One JSON line.

    python tests/perf/ambient_bench.py [--reps R]
"""
import io
import contextlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.getcwd())
from vireo_amd import predit_ambient, synth, _lib                 # noqa: E402
from vireo_amd.counts import DeviceCounts                        # noqa: E402
from vireo_amd.vireo_doublet import LAST_AMBIENT                 # noqa: E402

FP64_VECTOR_TFLOPS = 78.6       # MI355X spec: 256 CUs x 2.4 GHz x 128 fp64 flop / clk


def main():
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 3
    N, M, K, dens = synth.CONFIGS["c3"]
    t = time.perf_counter()
    w = synth.donor_workload(N, M, K, dens, seed=0)
    t_gen = time.perf_counter() - t
    t = time.perf_counter()
    counts = DeviceCounts.from_merged(w["shape"], w["colptr"], w["rowidx"], w["ad"], w["dp"])
    t_build = time.perf_counter() - t
    soft = 0.98
    GT = np.full((N, K, 3), (1 - soft) / 2)
    np.put_along_axis(GT, w["GT"][:, :, None], soft, axis=2)
    ID = np.full((M, K), (1 - soft) / (K - 1))
    ID[np.arange(M), w["z"]] = soft
    class V:                                                      # noqa: E306
        pass
    vobj = V()
    vobj.ID_prob, vobj.GT_prob, vobj.beta_mu, vobj.n_donor = ID, GT, np.array([[0.01, 0.5, 0.99]]), K
    runs = []
    for r in range(reps + 1):                                     # the first call is a warm-up
        np.random.seed(5)
        t = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            psi, var, llr = predit_ambient(vobj, counts, None)
        wall = time.perf_counter() - t
        if r:
            runs.append(dict(LAST_AMBIENT, wall_s=wall))
    best = min(runs, key=lambda d: d["wall_s"])
    it = best["n_iter"]
    # selected non-zero entries per cell (host, from the same arrays)
    rowsel = np.zeros(N, bool)
    from tests.ambient_np import elbo_gain                        # noqa: E402
    from scipy.sparse import csc_matrix
    AD = csc_matrix((w["ad"], w["rowidx"], w["colptr"]), shape=w["shape"])
    DP = csc_matrix((w["dp"], w["rowidx"], w["colptr"]), shape=w["shape"])
    rowsel = elbo_gain(ID, AD, DP) >= np.sqrt(M) / 3.0
    keep = (rowsel[w["rowidx"]] & (w["dp"] > 0)).astype(np.int64)
    per_cell = np.add.reduceat(keep, w["colptr"][:-1]) * (np.diff(w["colptr"]) > 0)
    # EM kernel work: (it + 2) passes per cell (it + 1 updates, the last log-likelihood, the variance /
    # null pass); per entry and donor ~10 fp64 flop (t1, t0: 2 FMA + 1 sub; r: 2 FMA + 1 sub)
    passes = (it.astype(np.int64) + 2)
    flop = float(np.sum(passes * per_cell) * K * 10)
    em_s = best["em_ms"] * 1e-3
    theta_bytes = float(np.sum(passes * per_cell) * K * 8 * 2)    # theta read twice per pass
    hist = np.bincount(np.minimum(it, 199) // 10 * 10, minlength=200)[::10]
    out = dict(workload="predit_ambient at c3: N=%d variants x M=%d cells, K=%d, nnz=%d" % (N, M, K, counts.nnz),
               device=_lib.device_info(0)["name"], reps=reps,
               split_s=dict(gain=best["gain_s"], draws=best["draws_s"], compaction=best["compaction_ms"] * 1e-3,
                            em_kernel=em_s, download=best["download_ms"] * 1e-3),
               wall_s=best["wall_s"], all_wall_s=[d["wall_s"] for d in runs],
               cells_per_s=M / best["wall_s"], em_cells_per_s=M / em_s,
               n_selected=best["n_selected"],
               entries_per_cell=dict(min=int(per_cell.min()), median=float(np.median(per_cell)),
                                     max=int(per_cell.max()), total=int(per_cell.sum())),
               iterations=dict(min=int(it.min()), median=float(np.median(it)), max=int(it.max()),
                               histogram_by_10={"%d-%d" % (10 * i, 10 * i + 9): int(h)
                                                for i, h in enumerate(hist) if h}),
               em_fp64_tflops=flop / em_s * 1e-12, em_fp64_fraction_of_peak=flop / em_s * 1e-12 / FP64_VECTOR_TFLOPS,
               em_theta_read_tb_per_s=theta_bytes / em_s * 1e-12,
               lds_theta_cache_entries=int((int(os.environ.get("VIREO_AMBIENT_LDS", 16384)) - ((2 * K + 128) * 8 + 256))
                                           // ((K | 1) * 8)),
               host_s=dict(generate=t_gen, build=t_build),
               nan_cells=int(np.isnan(llr).sum()))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
