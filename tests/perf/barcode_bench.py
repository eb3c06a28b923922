"""Barcode selection (variant_select / vrx_barcode_*) at the sizes of a panel VCF: 100 000 and 1 000 000
variants x 16 samples, 1 000 000 x 64, three categories, with var_count; and one sparse shape
(P(value != 0) = 0.1, 200 000 x 24) that needs many rounds.  Per shape, after a warm-up call, the median
over the repeats of
  wall_s            host clock around the whole variant_select call: checks, transpose, upload and rounds
  round_kernel_ms   per round, hipEvents: the entropy kernel, and the kernels after it (maximum, tie flags,
                    compaction, sort, median, second compaction)
  entropy_kernel_share_of_bytes_bound
                    the ALGORITHMIC bytes of a round, n_var K genotype bytes + 8 n_var entropy bytes, over
                    the 8 TB/s HBM figure, divided by the entropy kernel's time.  The kernel reads the
                    genotype bytes three times (number of terms, normalising sum, entropy); the second and
                    third reads are meant to come from cache, so the bound counts them once.
Baseline: the NumPy restatement of the reference's loop (tests/variant_select_np.py, vectorised over the
variants -- far faster than the reference's own per-variant Python loop) on the same machine, timed ONCE on
the first 20 000 variants and scaled by the number of variants (host_scaled_from_subset).  The device's
selection on that subset must equal the restatement's.
One JSON line; --out FILE writes it too.

    python tests/perf/barcode_bench.py [--reps R] [--shapes 100000x16,1000000x16,1000000x64,sparse200000x24] [--out FILE]
"""
import contextlib
import io
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from vireo_amd import _lib, variant_select                         # noqa: E402
from vireo_amd.variant_select import BarcodeRounds                 # noqa: E402
from tests import variant_select_np as V                           # noqa: E402

HBM_B_S = 8.0e12
SUBSET = 20000
N_CAT = 3


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def panel(seed, n_var, K, sparse):
    rs = np.random.RandomState(seed)
    if sparse:
        GT = (rs.randint(1, N_CAT, (n_var, K), dtype=np.uint8) * (rs.rand(n_var, K) < 0.1)).astype(np.uint8)
    else:
        GT = rs.randint(0, N_CAT, (n_var, K), dtype=np.uint8)
    return GT, rs.randint(21, 200, n_var).astype(float)


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def timed_rounds(GT, vc, seed):
    """the selection's own loop with the library's per-round event times"""
    dev = BarcodeRounds(GT, vc)
    np.random.seed(seed)
    now, ent_ms, rest_ms, chosen = 0, [], [], []
    while True:
        top, _, n_kept = dev.round()
        ent_ms.append(dev.ms[0])
        rest_ms.append(dev.ms[1])
        if top == now:
            break
        i, now = dev.pick(np.random.randint(n_kept))
        chosen.append(int(i))
        dev.choose(GT[i])
    dev.close()
    return ent_ms, rest_ms, chosen


def main():
    reps = int(arg("--reps", 3))
    shapes = arg("--shapes", "100000x16,1000000x16,1000000x64,sparse200000x24").split(",")
    _lib.require_gpu()
    rows = []
    for k, spec in enumerate(shapes):
        sparse = spec.startswith("sparse")
        n_var, K = (int(v) for v in spec.replace("sparse", "").split("x"))
        GT, vc = panel(k + 1, n_var, K, sparse)
        wall, ent_ms, rest_ms, n_rounds = [], [], [], 0
        for r in range(reps + 1):                                  # the first call is a warm-up
            t = time.perf_counter()
            _, _, chosen = quiet(variant_select, GT, vc, rand_seed=0)
            w = time.perf_counter() - t
            e, f, chosen2 = timed_rounds(GT, vc, 0)
            assert chosen2 == [int(i) for i in chosen]
            if r:
                wall.append(w)
                ent_ms.append(float(np.median(e)))
                rest_ms.append(float(np.median(f)))
                n_rounds = len(e)
        sub = min(SUBSET, n_var)
        t = time.perf_counter()
        host = V.select(GT[:sub], vc[:sub], rand_seed=0)
        host_s = (time.perf_counter() - t) * n_var / sub
        assert [int(i) for i in quiet(variant_select, GT[:sub], vc[:sub], rand_seed=0)[2]] == host["chosen"]
        med_ent = float(np.median(ent_ms)) * 1e-3
        t_bytes = (float(n_var) * K + 8.0 * n_var) / HBM_B_S
        rows.append(dict(
            shape=spec, n_var=n_var, n_donor=K, categories=N_CAT, sparse=sparse, with_var_count=True, reps=reps,
            rounds=n_rounds, chosen=len(chosen),
            wall_s=dict(median=float(np.median(wall)), min=float(min(wall)), max=float(max(wall))),
            round_kernel_ms=dict(entropy_median=med_ent * 1e3, after_entropy_median=float(np.median(rest_ms))),
            algorithmic_bytes_per_round=float(n_var) * K + 8.0 * n_var, bound_bytes_ms=t_bytes * 1e3,
            entropy_kernel_share_of_bytes_bound=t_bytes / med_ent,
            host_restatement_s=host_s, host_scaled_from_subset=None if sub == n_var else [sub, n_var],
            speedup_wall_vs_host_restatement=host_s / float(np.median(wall))))
        del GT, vc
    out = dict(workload="variant_select, 3 categories, with var_count, genotypes on the host",
               device=_lib.device_info(0)["name"], hbm_b_per_s=HBM_B_S, shapes=rows)
    line = json.dumps(out)
    print(line)
    if "--out" in sys.argv:
        with open(arg("--out", ""), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
