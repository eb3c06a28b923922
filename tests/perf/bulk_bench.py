"""Bulk donor-abundance EM (VireoBulk.fit) at 1 M x 16 and 10 M x 16 variants x donors, n_GT = 3: wall time
of the upload (create), milliseconds per EM iteration from hipEvents around the passes (warm-up, repeats,
median and spread), achieved bytes per second of the pass against its algorithmic bytes
8 N K G + 16 N and the 8 TB/s HBM figure, and the NumPy restatement on the host as context.  One JSON line.

    python tests/perf/bulk_bench.py [--reps R] [--iters I] [--sizes 1000000,10000000] [--out FILE]

Under a kernel trace, ``--trace-fit I`` runs ONE fit of I iterations at the first size and nothing else,
so that the trace shows I + 1 launches of vrx_bulk_pass.
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.getcwd())
from vireo_amd import VireoBulk, device_bulk, _lib                 # noqa: E402
from tests import bulk_np as B                                    # noqa: E402

HBM_TB_S = 8.0                  # MI355X spec, as in the other roofline lines
BASE = 1_000_000                # larger pools repeat this one (the values do not change the traffic)


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def pool(n_var, K, G):
    AD, DP, GT, psi, theta = B.synth_pool(min(n_var, BASE), K, G, seed=0, private=False)
    if n_var > BASE:
        r = -(-n_var // BASE)
        AD, DP, GT = np.tile(AD, r)[:n_var], np.tile(DP, r)[:n_var], np.tile(GT, (r, 1, 1))[:n_var]
    return AD, DP, np.ascontiguousarray(GT), theta


def main():
    reps, iters = int(arg("--reps", 7)), int(arg("--iters", 20))
    sizes = [int(x) for x in arg("--sizes", "1000000,10000000").split(",")]
    K, G = 16, 3
    if "--trace-fit" in sys.argv:
        n = int(arg("--trace-fit", 12))
        AD, DP, GT, theta = pool(sizes[0], K, G)
        np.random.seed(1)
        m = VireoBulk(K, theta_init=list(theta))
        m.fit(AD, DP, GT, max_iter=n, min_iter=n)
        print(json.dumps(dict(trace_fit_iterations=len(m.logLik_all) + 1, expected_pass_launches=n + 1)))
        return
    rows = []
    for n_var in sizes:
        AD, DP, GT, theta = pool(n_var, K, G)
        t = time.perf_counter()
        data = device_bulk(AD, DP, GT)
        create_s = time.perf_counter() - t
        ms, wall = [], []
        for r in range(reps + 1):                                  # the first fit is a warm-up
            np.random.seed(1)
            m = VireoBulk(K, theta_init=list(theta))
            t = time.perf_counter()
            m.fit(data, max_iter=iters, min_iter=iters)            # no stop: iters + 1 passes in one batch
            w = time.perf_counter() - t
            assert len(m.logLik_all) == iters - 1
            if r:
                ms.append(m.fit_ms_ / (iters + 1))
                wall.append(w)
        t = time.perf_counter()
        data.loglik(np.stack([m.psi, np.full(K, 1.0 / K)]), m.theta)
        t = time.perf_counter()
        data.loglik(np.stack([m.psi, np.full(K, 1.0 / K)]), m.theta)
        ll_s = time.perf_counter() - t
        data.close()
        pass_bytes = 8.0 * n_var * K * G + 16.0 * n_var
        med = float(np.median(ms))
        row = dict(n_var=n_var, n_donor=K, n_GT=G, gt_prob_gb=8.0 * n_var * K * G * 1e-9, create_wall_s=create_s,
                   ms_per_iteration=dict(median=med, min=float(min(ms)), max=float(max(ms)), reps=reps,
                                         iterations_per_fit=iters),
                   pass_bytes=pass_bytes, achieved_tb_per_s=pass_bytes / (med * 1e-3) * 1e-12,
                   fraction_of_hbm_8tb_s=pass_bytes / (med * 1e-3) * 1e-12 / HBM_TB_S,
                   fit_wall_s=dict(median=float(np.median(wall)), min=float(min(wall))),
                   lik_ratio_two_psi_wall_s=ll_s)
        if n_var <= BASE:   # context only: the NumPy restatement on the host stands in for the reference
            np.random.seed(1)
            psi0, _ = B.init(K, G)
            t = time.perf_counter()
            B.fit_chunked(AD, DP, GT, psi0, theta, max_iter=3, min_iter=3, dtype=np.float64)
            row["host_numpy_float64_s_per_iteration_context"] = (time.perf_counter() - t) / 4
        rows.append(row)
    out = dict(workload="VireoBulk.fit, learn_theta=True, n_GT=3", device=_lib.device_info(0)["name"], sizes=rows)
    line = json.dumps(out)
    print(line)
    if "--out" in sys.argv:
        with open(arg("--out", ""), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
