"""The ambient-RNA kernels on the device, one update at a time, against the extended-precision restatement.

``vrx_amb_em`` (the per-cell EM behind ``predit_ambient``) was held by whole fits only -- psi at 1e-12 absolute,
llr at 1e-9 -- and an EM run to convergence forgets a defect of a single update; ``vrx_amb_gain`` (the digamma /
logsumexp of ``variant_ELBO_gain``) at 1e-9 + 1e-12 |gain| on a sample of variants, 1e3 .. 1e5 units wide on a
variant of a few reads.  Here ``vrx_problem_ambient`` is forced to a length (``min_iter = max_iter``,
``epsilon = 0``: the stop rule never fires, every cell reports ``n_iter = max_iter - 1``) and psi, var and llr
of every cell, and the gain of every variant, are held to their own error units (tests/exact_np.py
``ambient_cell``, ``elbo_gain``), by the rule of tests/test_gpu_update_exact.py:

    u_dev = |device - exact| / unit  <=  4 * max(u_orc, 1)

with u_orc the distance of tests/ambient_np.py in float64 on the same input; the bound is never formed from
the device's own value.  The cases (tests/exact_ambient.py) sit on the 64-entry chunks of ``vrx_amb_pass``, the
second trip of its lane-strided loops (K > 64), the LDS capacity and the edge states of psi and theta; each
runs under the default budget, VIREO_AMBIENT_LDS=0, an all-cached budget where 64 KiB hold it and a small cap,
one route judged against exact and the others bit for bit equal to it, with the route of every constructed
cell asserted from the library's own cap (``vrx_ambient_info``).  The same sweep runs on the CPU with float64
NumPy in the device's place (tests/test_exact_ambient_cpu.py).

The gain's variant pass is created inside the library, so a ``DeviceModel`` of the same configuration on the
same counts is created beside each call and its ``info()`` asserted: a STAND-IN, as in
tests/test_gpu_postfit_exact.py.

VIREO_AMBIENT_UNITS_OUT=<file> writes the table of the run (profiles/ambient_exact_units.txt).
"""
import os
import time

import pytest

from tests import exact_ambient as XA

pytestmark = pytest.mark.gpu

# (step, case, output) whose device arithmetic is legitimate and further out than the rule allows: nothing is
# added here without an 80-bit arbitration written beside it -- none
PINNED = {}

_ROWS = []


@pytest.fixture(scope="module")
def va():
    import vireo_amd
    from vireo_amd import _lib
    _lib.require_gpu()                  # fail loudly: there is no CPU fallback
    start = time.time()
    yield vireo_amd
    path = os.environ.get("VIREO_AMBIENT_UNITS_OUT")
    if path:
        _write_table(path, time.time() - start)


def _write_table(path, seconds):
    with open(path, "w") as f:
        f.write("# distance from the extended-precision restatement of the ambient EM at a forced length and of the\n"
                "# ELBO gain, in error units (tests/exact_np.py): the device's, the float64 side's, and the bound\n"
                "# 4 * max(float64, 1); the largest over the counted cells (the variants) of a case\n"
                "# em, long, chain: vrx_problem_ambient at min_iter = max_iter = 2 (em, chain) or n, epsilon = 0;\n"
                "# gain: vrx_problem_elbo_gain under VIREO_LDS = 0 / 1\n"
                "# %d rows in %.1f s (the device's calls and the host's 80-bit side)\n"
                "#\n# worst case of each output (largest device distance; largest share of its bound)\n"
                % (len(_ROWS), seconds))
        for step in ("em", "long", "chain", "gain"):
            for out in sorted({r[2] for r in _ROWS if r[0] == step}):
                rows = [r for r in _ROWS if r[0] == step and r[2] == out]
                far = max(rows, key=lambda r: r[3])
                tight = max(rows, key=lambda r: r[3] / r[5])
                f.write("# %-8s %-8s %8.3f units in %-32s %5.2f of the bound in %s\n"
                        % (step, out, far[3], far[1], tight[3] / tight[5], tight[1]))
        f.write("\n%-8s %-32s %-8s %10s %10s %10s\n" % ("step", "case", "output", "device", "float64", "bound"))
        for row in _ROWS:
            f.write("%-8s %-32s %-8s %10.3f %10.3f %10.3f\n" % row)


def _clean_env(monkeypatch):
    for k in ("VIREO_BUILD", "VIREO_ENTRY_FMT", "VIREO_LDS", "VIREO_LDS_BLOCKS", "VIREO_CELL_FORM", "VIREO_VAR_FORM",
              "VIREO_AMBIENT_LDS"):
        monkeypatch.delenv(k, raising=False)


class DeviceSide(XA.Float64Side):
    """the calls of a case on the device"""

    def __init__(self, monkeypatch):
        self.mp = monkeypatch
        self.counts = None

    def open(self, p):
        from vireo_amd.counts import DeviceCounts
        _clean_env(self.mp)
        self.mp.setenv("VIREO_ENTRY_FMT", str(p.spec.fmt))
        self.counts = DeviceCounts.from_merged(p.shape, p.colptr, p.rowidx, p.ad, p.dp)
        # the format the case asks for is the one that was built
        assert self.counts.entry_format() == (p.spec.fmt, p.spec.fmt), (p.name, self.counts.entry_format())

    def close(self):
        if self.counts is not None:
            self.counts.close()
            self.counts = None

    def _budget(self, budget):
        if budget is None:
            self.mp.delenv("VIREO_AMBIENT_LDS", raising=False)
        else:
            self.mp.setenv("VIREO_AMBIENT_LDS", str(budget))

    def fit(self, p, psi0, rule, budget):
        self._budget(budget)
        return XA.run_ambient(self.counts, p.K, p.theta, p.sel, psi0, *rule)

    def caps(self, p):
        out = {}
        for name, budget in p.routes:
            self._budget(budget)
            cap, lds = XA.library_plan(p.K)
            assert lds == XA.amb_lds_bytes(p.K, cap) <= XA.LDS_MAX, (p.name, name, cap, lds)
            out[name] = cap
        return out

    def gain(self, g, lds):
        from vireo_amd import _lib, variant_ELBO_gain
        from vireo_amd.counts import DeviceCounts
        from tests.test_gpu_postfit_exact import _assert_stand_in
        _clean_env(self.mp)
        self.mp.setenv("VIREO_LDS", lds)
        counts = DeviceCounts(g.AD, g.DP)
        try:
            # the variant pass of the call: a clone-mode model of K + 1 columns (ID_prob and a column of ones)
            _assert_stand_in(counts, _lib.KIND_BMM, g.K + 1, lds == "1", "gain", sides=("lds_variant",))
            return variant_ELBO_gain(g.ID, counts, None, pseudocount=g.pc)
        finally:
            counts.close()


def test_amb_cap_agrees_with_the_library(va, monkeypatch):
    for budget in (None, 0, 4408, 16384, 65536):
        if budget is None:
            monkeypatch.delenv("VIREO_AMBIENT_LDS", raising=False)
        else:
            monkeypatch.setenv("VIREO_AMBIENT_LDS", str(budget))
        for K in (1, 2, 3, 8, 16, 33, 63, 64, 65, 130):
            cap, lds = XA.library_plan(K)
            assert cap == XA.route_cap(K, budget) and lds == XA.amb_lds_bytes(K, cap), (K, budget, cap, lds)


@pytest.mark.parametrize("name", list(XA.EM))
def test_ambient_em_against_exact(va, monkeypatch, name):
    p = XA.problem(name)
    side = DeviceSide(monkeypatch)
    side.open(p)
    try:
        XA.RUN[p.spec.kind](p, side, _ROWS, PINNED)
    finally:
        side.close()


@pytest.mark.parametrize("name", list(XA.GAIN))
def test_elbo_gain_against_exact(va, monkeypatch, name):
    XA.run_gain(name, DeviceSide(monkeypatch), _ROWS, PINNED)
