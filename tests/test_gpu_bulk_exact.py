"""The bulk donor-abundance EM on the device, one update at a time, against the extended-precision
restatement.

``vrx_bulk_pass`` / ``vrx_bulk_finish``, ``vrx_bulk_ll`` / ``vrx_bulk_ll_sum`` and the four
``vrx_bulk_cohort_*`` kernels were held by whole fits at 1e-12: nothing looked at one pass alone, and none
of the kernels' own shape boundaries was approached on purpose.  Here ``BulkData.fit(max_iter=1)`` -- two
passes: update 0, then ``logLik[0]`` of the updated parameters -- ``loglik`` and their cohort forms are held
to the error unit of every output (tests/exact_np.py ``bulk_update``, ``bulk_loglik``), by the rule of
tests/test_gpu_update_exact.py:

    u_dev = |device - exact| / unit  <=  4 * max(u_orc, 1)

with u_orc the distance of tests/bulk_np.py in float64 on the same input; the bound is never formed from
the device's own value.  The cases (tests/exact_bulk.py) sit on the tile size the LDS budget gives, the
slices of phase 2 and its rounds beyond 256 columns, the odd tail of a tile's load, 64 partials per lane
of the reduction, eight psi vectors per log-likelihood pass and four samples per cohort chunk; each
asserts through ``BulkData.info()`` the tile and workgroup counts it is written for.  The same sweep
runs on the CPU with float64 NumPy in the device's place (tests/test_exact_bulk_cpu.py).

VIREO_BULK_UNITS_OUT=<file> writes the table of the run (profiles/bulk_exact_units.txt).
"""
import os

import numpy as np
import pytest

from tests import exact_bulk as XB

pytestmark = pytest.mark.gpu

# (step, case, output) whose device arithmetic is legitimate and further out than the rule allows:
# measured units x 1.25, with an 80-bit argument that the device is the closer side -- none
PINNED = {}

_ROWS = []


@pytest.fixture(scope="module")
def n_cu():
    import vireo_amd                    # noqa: F401
    from vireo_amd import _lib
    _lib.require_gpu()                  # fail loudly: there is no CPU fallback
    yield int(_lib.device_info(0)["n_cu"])
    path = os.environ.get("VIREO_BULK_UNITS_OUT")
    if path:
        _write_table(path)


def _write_table(path):
    with open(path, "w") as f:
        f.write("# distance from the extended-precision restatement of one bulk update or log-likelihood, in error\n"
                "# units (tests/exact_np.py): the device's, the float64 side's, and the bound 4 * max(float64, 1)\n"
                "# fit, chain: vrx_bulk_fit at max_iter = 1; loglik: vrx_bulk_loglik; cohort: vrx_bulk_fit_cohort;\n"
                "# co_ll: vrx_bulk_loglik_cohort\n"
                "#\n# worst case of each output (largest device distance; largest share of its bound)\n")
        for step in ("fit", "chain", "loglik", "cohort", "co_ll"):
            for out in sorted({r[2] for r in _ROWS if r[0] == step}):
                rows = [r for r in _ROWS if r[0] == step and r[2] == out]
                far = max(rows, key=lambda r: r[3])
                tight = max(rows, key=lambda r: r[3] / r[5])
                f.write("# %-8s %-8s %8.3f units in %-44s %5.2f of the bound in %s\n"
                        % (step, out, far[3], far[1], tight[3] / tight[5], tight[1]))
        f.write("\n%-8s %-48s %-8s %10s %10s %10s\n" % ("step", "case", "output", "device", "float64", "bound"))
        for row in _ROWS:
            f.write("%-8s %-48s %-8s %10.3f %10.3f %10.3f\n" % row)


class DeviceSide:
    """the calls of a case on one ``BulkData``"""

    def __init__(self, d):
        from vireo_amd.vireo_bulk import device_bulk
        cohort = d.AD.ndim == 2
        self.h = device_bulk(d.AD[0] if cohort else d.AD, d.DP[0] if cohort else d.DP, d.GT)
        info = self.h.info()
        # the tile and workgroup counts the case is written for, of its own pass; then all four passes
        kt, kw = XB.PASSES[d.which]
        assert (info[kt], info[kw]) == (d.T, d.n_wg) and -(-d.N // info[kt]) == d.tiles, (d.name, info, d.tiles)
        if "stride" in d.name:
            assert d.tiles > 2 * info[kw]
        assert info == d.plan, (d.name, info, d.plan)

    def close(self):
        self.h.close()

    def fit(self, d, psi, theta, max_iter=1, learn_theta=True):
        psi, theta, trace, it, _ = self.h.fit(psi, theta, max_iter=max_iter, learn_theta=learn_theta, delay_fit_theta=0)
        assert it == max_iter - 1 and trace.shape == (max_iter,)
        return psi, theta, trace

    def loglik(self, d, psis, theta):
        return self.h.loglik(psis, theta)

    def fit_cohort(self, d, idx, psi, theta, max_iter=1, learn_theta=True):
        self.h.set_cohort(d.AD[idx], d.DP[idx])
        psi, theta, traces, it, _ = self.h.fit_cohort(psi, theta, max_iter=max_iter, learn_theta=learn_theta,
                                                      delay_fit_theta=0)
        assert np.all(it == max_iter - 1) and traces.shape == (len(idx), max_iter)
        return psi, theta, traces

    def loglik_cohort(self, d, idx, psis, theta):
        self.h.set_cohort(d.AD[idx], d.DP[idx])
        return self.h.loglik_cohort(psis, theta)


def test_cohort_chunk_is_what_the_cases_assume(n_cu):
    from vireo_amd import _lib
    assert int(_lib.lib().vrx_bulk_cohort_chunk()) == XB.COHORT


@pytest.mark.parametrize("name", list(XB.CASES))
def test_bulk_against_exact(n_cu, name):
    d = XB.build(name, n_cu)
    side = DeviceSide(d)
    try:
        XB.RUN[d.spec.kind](d, side, _ROWS, PINNED)
    finally:
        side.close()
