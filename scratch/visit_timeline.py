"""Per-visit timeline of the LDS passes' workgroup 0 at c3 (profiles/r08_visit_timeline.txt): when, inside a
slab visit, the waves of a SIMD finish their rounds.  Needs a probe build of the library
(`scratch/build_variant.sh NAME -DVRX_PROBE_VISITS [-DVRX_WAVE_PRIO=...]`, selected with VIREO_LIB): lane 0 of every
wave of workgroup 0 records the cycle counter behind the second slab barrier and at the end of its last round.
usage: VIREO_LIB=scratch/lib_NAME.so python scratch/visit_timeline.py LABEL [iterations=40] [FILE]"""
import collections
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vireo_amd import _lib, synth  # noqa: E402
from vireo_amd.counts import DeviceCounts  # noqa: E402
from vireo_amd.engine import DeviceModel  # noqa: E402
from vireo_amd.vireo_model import Vireo  # noqa: E402

label = sys.argv[1]
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 40
N, M, K, d = synth.CONFIGS["c3"]
w = synth.donor_workload(N, M, K, d, seed=0)
counts = DeviceCounts.from_merged(w["shape"], w["colptr"], w["rowidx"], w["ad"], w["dp"], device=0,
                                  balance=os.environ.get("VIREO_BALANCE", "1") != "0")
np.random.seed(1)
host = Vireo(n_var=N, n_cell=M, n_donor=K)
dm = DeviceModel(counts, _lib.KIND_VIREO, K, n_gt=3)
dm.set_state(host.ID_prob, host.GT_prob, host.beta_mu, host.beta_sum)
dm.set_prior(host.ID_prior, host.GT_prior, host.theta_s1_prior, host.theta_s2_prior)
dm.run_iters(iters, theta_from_iter=0)

h = _lib.lib()
cap = C.c_int(0)
n = (C.c_uint * 16)()
log = np.zeros((1 << 13, 16, 4), dtype=np.uint64)
rc = h.vrx_probe_visits(log.ctypes.data_as(C.c_void_p), n, C.byref(cap))
assert rc == 0 and cap.value == log.shape[0], (rc, cap.value)
n = np.array(list(n))
assert (n == n[0]).all(), n          # every wave of the workgroup makes every visit
keep = min(int(n[0]), cap.value)
idx = np.arange(int(n[0]) - keep, int(n[0])) % cap.value
rec = log[idx].astype(np.int64)      # [visit][wave][barrier, end, tag, item]
tag = rec[:, 0, 2]
lines = ["%s: %d iterations at c3, %d visits of workgroup 0 recorded (the last %d kept)" % (label, iters, n[0], keep)]
for rows, rw in sorted(set((int(t >> 32), int((t >> 16) & 0xffff)) for t in tag)):
    v = rec[(tag >> 32 == rows) & ((tag >> 16) & 0xffff == rw)]
    t0 = v[:, :, 0].min(axis=1, keepdims=True)           # the first wave through the barrier
    end = v[:, :, 1] - t0                                # [visit][wave]
    phase = end.max(axis=1)                              # the trips phase of the visit
    lines.append("  pass with %d output rows (RW %d): %d visits, trips phase median %d clk"
                 % (rows, rw, len(v), np.median(phase)))
    lines.append("    finish of wave 0..15, median clk after the barrier: " + " ".join("%d" % x for x in np.median(end, axis=0)))
    for simd in range(4):
        e = end[:, simd::4]                              # waves simd, simd + 4, simd + 8, simd + 12
        order = collections.Counter(tuple(int(simd + 4 * k) for k in np.argsort(r, kind="stable")) for r in e)
        top, cnt = order.most_common(1)[0]
        spread = e.max(axis=1) - e.min(axis=1)
        lines.append("    SIMD %d: finish order %s (%d %% of visits); first-to-last spread median %d clk = %.1f %% of the phase"
                     % (simd, "<".join(map(str, top)), 100 * cnt // len(e), np.median(spread), 100 * np.median(spread / phase)))
    spread = np.stack([end[:, s::4].max(axis=1) - end[:, s::4].min(axis=1) for s in range(4)], axis=1).mean(axis=1)
    lines.append("    mean over the SIMDs of the first-to-last spread: median %d clk = %.1f %% of the trips phase"
                 % (np.median(spread), 100 * np.median(spread / phase)))
if len(sys.argv) > 3:                  # also kept as a file
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[3])), exist_ok=True)
    with open(sys.argv[3], "w") as f:
        f.write("\n".join(lines) + "\n")
print("\n".join(lines))
