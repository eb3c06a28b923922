"""A cohort of bulk samples on one donor panel: the loop the parent commit offers (``set_counts`` + ``BulkData.fit``
per sample, S times) against ``set_cohort`` + ``fit_cohort``, in one process, alternating, on the same counts.
Both run max_iter = 20 with an epsilon_conv that never fires, so both do 21 passes per sample.

Per shape (n_var, n_donor, n_sample) at n_GT = 3 and per side: host wall time of the fits alone and of uploads +
fits, device milliseconds (hipEvents around the passes; the loop's are summed over its S fits), each as median /
min / max over the repeats; device ms per sample-iteration; the ratios loop / cohort; and the bytes of GT_prob a
sample-iteration reads (the loop streams GT_prob once per sample and pass, the cohort once per chunk and pass).
One JSON line; the file is rewritten after every shape, so a run cut short keeps the shapes it finished.

    python tests/perf/bulk_cohort_bench.py [--reps R] [--iters I] [--shapes 1000000x16x16,100000x16x64] [--out FILE]
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.getcwd())
from vireo_amd import device_bulk, _lib                             # noqa: E402
from tests import bulk_np as B                                    # noqa: E402

SHAPES = "1000000x16x16,100000x16x64,10000x16x64,1000000x64x16"
NEVER = -1e300                   # gain < NEVER is false for every gain: the loop runs to max_iter


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def cohort_pool(n_var, K, G, S):
    """one GT_prob, S samples with a planted psi each -> AD, DP (S, n_var) float64, GT_prob, theta"""
    _, _, GT, _, theta = B.synth_pool(n_var, K, G, seed=0, private=False)
    rng = np.random.default_rng(1)
    tm = np.tensordot(GT, theta, axes=(2, 0))
    AD, DP = np.empty((S, n_var)), np.empty((S, n_var))
    for s in range(S):
        DP[s] = rng.poisson(30.0, size=n_var)
        AD[s] = rng.binomial(DP[s].astype(np.int64), tm @ rng.dirichlet(np.full(K, 2.0)))
    return AD, DP, np.ascontiguousarray(GT), theta


def stats(x):
    return dict(median=float(np.median(x)), min=float(min(x)), max=float(max(x)))


def main():
    reps, iters = int(arg("--reps", 7)), int(arg("--iters", 20))
    shapes = [tuple(int(v) for v in x.split("x")) for x in arg("--shapes", SHAPES).split(",")]
    G = 3
    chunk = int(_lib.lib().vrx_bulk_cohort_chunk())
    fit = dict(max_iter=iters, min_iter=5, epsilon_conv=NEVER)
    out = dict(workload="bulk cohort fit, learn_theta=True, n_GT=3, max_iter=%d, no stop" % iters,
               device=_lib.device_info(0)["name"], cohort_chunk=chunk, reps=reps, shapes=[])
    for n_var, K, S in shapes:
        AD, DP, GT, theta = cohort_pool(n_var, K, G, S)
        rng = np.random.default_rng(2)
        psi0 = rng.dirichlet(np.ones(K), size=S)
        theta0 = np.tile(theta, (S, 1))
        data = device_bulk(AD[0], DP[0], GT)
        loop = dict(wall_fits=[], wall_with_uploads=[], device_ms=[])
        coh = dict(wall_fits=[], wall_with_uploads=[], device_ms=[])
        for r in range(reps + 1):                                   # the first round is a warm-up
            t_up = t_fit = ms = 0.0
            psi_loop = np.empty((S, K))
            for s in range(S):
                t = time.perf_counter()
                data.set_counts(AD[s], DP[s])
                t_up += time.perf_counter() - t
                t = time.perf_counter()
                res = data.fit(psi0[s], theta0[s], **fit)
                t_fit += time.perf_counter() - t
                assert res[3] == iters - 1
                ms += res[4]
                psi_loop[s] = res[0]
            t = time.perf_counter()
            data.set_cohort(AD, DP)
            c_up = time.perf_counter() - t
            t = time.perf_counter()
            res = data.fit_cohort(psi0, theta0, **fit)
            c_fit = time.perf_counter() - t
            assert (res[3] == iters - 1).all()
            psi_gap = float(np.abs(res[0] - psi_loop).max())         # the two sides agree (summation order apart)
            assert psi_gap < 1e-9, psi_gap
            if r:
                loop["wall_fits"].append(t_fit), loop["wall_with_uploads"].append(t_fit + t_up)
                loop["device_ms"].append(ms)
                coh["wall_fits"].append(c_fit), coh["wall_with_uploads"].append(c_fit + c_up)
                coh["device_ms"].append(res[4])
        data.close()
        n_si = S * (iters + 1)                                      # sample-iterations (passes) per side
        n_chunk = -(-S // chunk)
        row = dict(n_var=n_var, n_donor=K, n_GT=G, n_sample=S, passes_per_sample=iters + 1,
                   max_abs_psi_gap_loop_vs_cohort=psi_gap)
        for name, side in (("loop", loop), ("cohort", coh)):
            row[name] = dict(wall_fits_s=stats(side["wall_fits"]), wall_with_uploads_s=stats(side["wall_with_uploads"]),
                             device_ms=stats(side["device_ms"]),
                             device_ms_per_sample_iteration=float(np.median(side["device_ms"])) / n_si)
        row["loop"]["gt_prob_bytes_per_sample_iteration"] = 8.0 * n_var * K * G
        row["cohort"]["gt_prob_bytes_per_sample_iteration"] = 8.0 * n_var * K * G * n_chunk / S
        row["ratio_loop_over_cohort"] = {
            key: row["loop"][key]["median"] / row["cohort"][key]["median"]
            for key in ("wall_fits_s", "wall_with_uploads_s", "device_ms")}
        out["shapes"].append(row)
        line = json.dumps(out)
        if "--out" in sys.argv:
            with open(arg("--out", ""), "w") as f:
                f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
