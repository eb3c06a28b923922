"""Every EM update of the device, one at a time, against the extended-precision restatement.

The whole-fit tests compare after several iterations at rtol 1e-5 -- the floor of a chaotic
iteration, ten orders of magnitude above what one float64 update rounds.  Here each update is held
to its own error unit (tests/exact_np.py):

    u_dev = |device - exact| / unit  <=  4 * max(u_orc, 1)

with u_orc the float64 oracle's distance on the same input: 4 is the margin of
tests/test_gpu_postfit_sweep.py (two correct float64 sums in different orders), 1 the rounding of
the result itself; the bound is never formed from the device's own value.

Flow A drives ``DeviceModel.step`` (the unfused kernels), flow B ``run_iters`` (the fit loop's own
kernels: theta finalised inside the GT kernel, the softmax in the cell pass's epilogue, the ELBO
riding in the next theta launch, range sums fused into the dense kernels) in the reference's order;
there every update of every iteration is judged from the float64 state the device itself read back
in front of it (a run of each length from the same state), so what one update rounds is the next
one's input and never its excuse.  Every case asserts through ``info()`` / ``build_info()`` that
the path it names ran, and the cases that switch a fusion of the fit loop count its launches.
Every case is also held, after its updates have run, to the instances of ``vrx_spmm_lds`` its passes
launched (``DeviceModel.lds_launches()``): template arguments, column blocks, gather list, slabs.
The dense cases (``dense_*``) are sized in the grid terms of the device's CU count so that the dense
kernels run past their grid caps -- second and third sweeps of vrx_theta_partial, vrx_gt_update and
vrx_cell_softmax, two and three strides of the shared theta's second stage, two and three trips of the
ELBO's -- and each asserts the route it names from the model's record of its dense launches
(``DeviceModel.dense_launches()``) against the restated grid arithmetic (``exact_cases.dense_grid``)
before any number is compared.
The cases are in tests/exact_cases.py; the same sweep runs on the CPU with the oracle in the
device's place (tests/test_exact_cpu.py).

VIREO_EXACT_UNITS_OUT=<file> writes the table of the run (profiles/update_exact_units.txt).
"""
import os
from types import SimpleNamespace

import numpy as np
import pytest

from tests import exact_cases as EC
from tests import exact_np as X

pytestmark = pytest.mark.gpu

# (case, output) whose device arithmetic is legitimate and further out than the rule allows:
# measured units x 1.25, with the reason -- none so far
PINNED = {}

_ROWS = []
_ROUTES = {}        # dense case -> (flow, the route its launch record showed)


@pytest.fixture(scope="module")
def va():
    import vireo_amd
    from vireo_amd import _lib
    _lib.require_gpu()          # fail loudly: there is no CPU fallback
    EC.set_n_cu(_lib.device_info(0)["n_cu"])     # the dense cases' sizes follow the device's grid caps
    yield vireo_amd
    path = os.environ.get("VIREO_EXACT_UNITS_OUT")
    if path:
        _write_table(path)


def _write_table(path):
    with open(path, "w") as f:
        f.write("# distance from the extended-precision restatement of one update, in error units\n"
                "# (tests/exact_np.py): the device's, the float64 oracle's, and the bound 4 * max(oracle, 1)\n"
                "# flow A: one update through DeviceModel.step; flow B: whole iterations through run_iters\n")
        f.write("%-4s %-28s %-14s %10s %10s %10s\n" % ("flow", "case", "output", "device", "oracle", "bound"))
        for row in _ROWS:
            f.write("%-4s %-28s %-14s %10.3f %10.3f %10.3f\n" % row)
        f.write("\n# worst case of each output (largest device distance; largest share of its bound)\n")
        for flow in ("A", "B"):
            for out in sorted({r[2] for r in _ROWS if r[0] == flow}):
                rows = [r for r in _ROWS if r[0] == flow and r[2] == out]
                far = max(rows, key=lambda r: r[3])
                tight = max(rows, key=lambda r: r[3] / r[5])
                f.write("%-4s %-14s %10.3f units in %-28s %5.2f of the bound in %s\n"
                        % (flow, out, far[3], far[1], tight[3] / tight[5], tight[1]))
        f.write("\n# the dense kernels past their grid caps: the route each case's launch record showed (asserted\n"
                "# before any number was compared), its worst output in units and the largest share of a bound\n")
        f.write("%-4s %-28s %10s %6s  %s\n" % ("flow", "case", "worst", "share", "route"))
        for case, (flow, route) in _ROUTES.items():
            rows = [r for r in _ROWS if r[0] == flow and r[1].split("[")[0] == case]
            if rows:
                f.write("%-4s %-28s %10.3f %6.2f  %s\n" % (flow, case, max(r[3] for r in rows),
                                                          max(r[3] / r[5] for r in rows), route))
        f.write("# not covered:\n")
        for what, why in EC.NOT_COVERED:
            f.write("#   %s -- %s\n" % (what, why))


def _kind(p):
    from vireo_amd import _lib
    return _lib.KIND_VIREO if p.kind == "vireo" else _lib.KIND_BMM


def _counts(p, monkeypatch):
    from vireo_amd.counts import DeviceCounts
    for k, v in p.spec.env.items():
        monkeypatch.setenv(k, v)
    return DeviceCounts(p.AD, p.DP, balance=p.spec.balance)


def _assert_path(p, dm, counts):
    """the kernels, formats and builder the case names are the ones this model runs"""
    seen = dict(dm.info(), **counts.build_info())
    for k, v in p.spec.want.items():
        if k not in EC.LAUNCH_KEYS:
            assert v(seen[k]) if callable(v) else seen[k] == v, (p.spec.name, k, seen[k])
    return seen


def _assert_instances(p, dm, seen):
    """the instances of ``vrx_spmm_lds`` the passes of this case launched, from the model's launch
    record: block by block what the dispatch rule (restated in tests/exact_cases.py) gives for the
    shape, the stream forms and the operand's width; the set a case names (``inst_*``); the gather
    list passed exactly to the balanced streams; and the slab geometry of the cases that set it
    (``slab_fill``).  A pass on the gather kernels has recorded nothing."""
    sp, want, name = p.spec, p.spec.want, p.spec.name
    n_cu = _lib_info()["n_cu"]
    got = dict(zip(("variant", "cell"), dm.lds_launches()))
    rule = dict(zip(("variant", "cell"), EC.expected_launches(p.N, p.M, p.K * sp.restarts, seen["cell_form"],
                                                              seen["var_form"], n_cu)))
    if "slab_fill" in want:
        extra = (seen["extra_pieces_variant"], seen["extra_pieces_cell"])
        slabs = dict(zip(("variant", "cell"), EC.expected_slabs(p.N, p.M, seen["cell_form"], seen["var_form"],
                                                                n_cu, want["slab_fill"], extra)))
    for o in ("variant", "cell"):
        print("%-28s %-7s launches %s" % (name, o, [tuple(int(v) for v in l) for l in got[o]]))
        if not seen["lds_" + o]:
            assert got[o] == [], (name, o, got[o])
            continue
        assert [tuple(l[:7]) for l in got[o]] == rule[o], (name, o, got[o], rule[o])
        if "inst_" + o in want:
            assert {tuple(l[:5]) for l in got[o]} == want["inst_" + o], (name, o, got[o])
        perm = want.get("perm", seen["balanced_" + o])
        assert perm == seen["balanced_" + o] and all(l.perm == perm for l in got[o]), (name, o, perm, got[o])
        if "slab_fill" in want:
            for l in got[o]:
                assert (l.slab_rows, l.n_slab) == slabs[o], (name, o, l, slabs[o])
                assert l.slab_rows % 16 == 0 and l.slab_rows >= 64, (name, o, l)


def _assert_route(p, dm, flow):
    """a dense case took the route it declares: the model's record of its dense launches
    (``DeviceModel.dense_launches()``) against the restated grid arithmetic (``EC.dense_grid``) for this
    device's CU count, and that arithmetic against the sweeps / strides / trips the case names.  After
    flow A the last shared-theta update was finalised by vrx_theta_final and the last ELBO came from
    vrx_elbo_final; after flow B's longest run the finalisation is the fused or the separate one by the
    count of partials, and every ELBO but the last rode in the next theta launch where the case turns
    that on."""
    sp = p.spec
    if not callable(sp.data):
        return
    rec = dm.dense_launches()
    n_cu = rec["n_cu"]
    assert n_cu == EC.N_CU == _lib_info()["n_cu"], (sp.name, rec)
    assert EC.route_misses(sp, n_cu) == [], (sp.name, EC.route_misses(sp, n_cu))
    g = EC.dense_route(sp, p.N, p.M, n_cu)
    shared = p.kind == "vireo" and not sp.ase
    fused_cells = flow == "B" and bool(sp.fused_softmax)
    want = dict(nb_theta=g.nb_theta, n_cell_part=g.n_cell_part, n_gt_part=g.n_gt_part, n_th_part=g.n_th_part,
                elbo_carrier="kernel", cell_source="cell_pass" if fused_cells else "softmax")
    if shared:
        want.update(theta_parts=g.nb_theta, theta_final="fused" if flow == "B" and g.fuse else "kernel")
    if p.kind == "vireo":
        want["nb_gt"] = g.nb_gt
    if not fused_cells:
        want.update(nb_cell=g.nb_cell, KP=g.KP)
    rides = (flow == "B" and sp.iters >= 2 and sp.env.get("VIREO_ELBO_RIDE") == "1"
             and (shared or p.kind != "vireo"))
    if rides:
        want.update(ride_cell_part=g.n_cell_part, ride_gt_part=g.n_gt_part, ride_th_part=g.n_th_part)
    got = {k: rec[k] for k in want}
    print("%-28s route %s" % (sp.name, rec))
    assert got == want, (sp.name, got, want)
    took = ["%s=%s" % (k, getattr(g, k)) for k in EC.ROUTE_KEYS if k in sp.route]
    took += ["nb_theta=%d" % g.nb_theta, "nb_gt=%d" % rec["nb_gt"], "nb_cell=%d" % rec["nb_cell"], "KP=%d" % rec["KP"],
             "parts=%d/%d/%d" % (g.n_cell_part, g.n_gt_part, g.n_th_part)]
    if rides:
        took.append("ride+kernel")
    _ROUTES[sp.name] = (flow, " ".join(took))


def _lib_info():
    from vireo_amd import _lib
    return _lib.device_info(0)


class DeviceBackend:
    """``DeviceModel`` in the oracle's place: every update starts from the case's state"""

    def __init__(self, p, counts):
        from vireo_amd import _lib
        from vireo_amd.engine import DeviceBatch, DeviceModel
        self.p, self.L = p, _lib
        sp, pri = p.spec, p.pri
        kw = dict(n_gt=p.T, learn_gt=sp.learn_gt, ase_mode=sp.ase, fix_beta_sum=sp.fix)
        self.dm = DeviceModel(counts, _kind(p), p.K, **kw)
        self.dm.set_prior(pri.ID_prior, pri.GT_prior, pri.th1, pri.th2)
        self.batch, self.launches, self.ran, self.at = None, {}, None, None
        if sp.restarts > 1:
            self.batch = DeviceBatch(counts, _kind(p), p.K, sp.restarts, **kw)
            self.batch.set_prior(pri.ID_prior, pri.GT_prior, pri.th1, pri.th2)

    def reset(self, r=0):
        s = self.p.states[r]
        self.dm.set_state(s.ID, s.GT, s.mu, s.sm)

    def theta(self):
        self.reset()
        self.dm.step(self.L.STEP_THETA)
        return self.dm.get_state(want_GT=False)[2:]

    def gt(self):
        self.reset()
        self.dm.step(self.L.STEP_GT)
        return self.dm.get_state()[1]

    def id(self):
        self.reset()
        self.dm.step(self.L.STEP_ID)
        return self.dm.get_loglik(), self.dm.get_state(want_GT=False)[0]

    def elbo(self, L):
        self.reset()
        self.dm.set_loglik(L)
        total = self.dm.step(self.L.STEP_ELBO)
        parts = self.dm.elbo_parts()
        assert total == parts[0] - parts[1] - parts[2] - parts[3]
        return parts

    def elbo_recomputed(self):
        self.reset()
        self.dm.step(self.L.STEP_LOGLIK)
        L = self.dm.get_loglik()
        self.dm.step(self.L.STEP_ELBO)
        return L, self.dm.elbo_parts()

    def run(self, r, n):
        """n iterations of the fit loop from restart r's state -> what the device holds after them.
        A batch runs all its restarts at once; slot r moves to the single model to be read (its
        logLik_ID does not: L = None)."""
        if self.batch is None:
            self.reset(r)
            self.dm.profile(True)
            trace, _ = self.dm.run_iters(n, 0)
            self.launches[n] = self.dm.profile_read()[1]
            self.dm.profile(False)
            parts, L = self.dm.elbo_parts(), self.dm.get_loglik()
        else:
            if self.at != n:                      # (the batch holds one run at a time)
                for i, s in enumerate(self.p.states):
                    self.batch.set_restart(i, s.ID, s.GT, s.mu, s.sm)
                self.ran, self.at = (self.batch.run_iters(n, 0)[0], self.batch.elbo_parts()), n
            self.batch.copy_to(self.dm, r)
            trace, parts, L = self.ran[0][r], self.ran[1][r], None
        ID, GT, mu, sm = self.dm.get_state()
        return SimpleNamespace(ID=ID, GT=GT, mu=mu, sm=sm, L=L, trace=trace, parts=parts)


def _assert_launches(p, be):
    """VIREO_FUSE_SOFTMAX / VIREO_ELBO_RIDE: the fusion the case names is observed, not inferred from
    its preconditions -- the dense launches the profile counted over the whole run.  The run opens
    with one (psi and KL_theta of the state just set); an iteration launches the theta kernel, the
    GT kernel (Vireo), the cell softmax unless it ran in the cell pass's epilogue, and the ELBO
    kernel unless that ELBO rode in the next iteration's theta launch (every iteration but the last)."""
    sp = p.spec
    if sp.fused_softmax is None:
        return
    ride = sp.env.get("VIREO_ELBO_RIDE") == "1"
    per_iter = (2 if p.kind == "vireo" else 1) + (0 if sp.fused_softmax else 1) + 1
    assert sorted(be.launches) == list(range(1, sp.iters + 1))
    for n, got in be.launches.items():
        want = 1 + n * per_iter - (n - 1 if ride else 0)
        assert got[be.L.KERN_DENSE] == want, (sp.name, n, "dense launches", int(got[be.L.KERN_DENSE]), want)


def _judge(flow, case, u_dev, u_orc):
    bad = []
    for k in u_dev:
        limit = PINNED.get((case, k), X.bound(u_orc[k]))
        _ROWS.append((flow, case, k, u_dev[k], u_orc[k], limit))
        print("%s %-28s %-14s device %9.3f  oracle %9.3f  bound %9.3f" % (flow, case, k, u_dev[k], u_orc[k], limit))
        if not u_dev[k] <= limit:
            bad.append((k, u_dev[k], u_orc[k], limit))
    assert not bad, "%s %s: (output, device, oracle, bound) %s" % (flow, case, bad)


def test_state_round_trip_is_exact(va, monkeypatch):
    """what ``set_state`` takes is what ``get_state`` / ``get_loglik`` return: the float64 state is
    the exact input of every comparison below"""
    p = EC.problem_a("gather")
    be = DeviceBackend(p, _counts(p, monkeypatch))
    be.reset()
    s = p.s0
    for got, want in zip(be.dm.get_state(), (s.ID, s.GT, s.mu, s.sm)):
        assert np.array_equal(got, want)
    L = np.random.default_rng(0).normal(size=(p.M, p.K))
    be.dm.set_loglik(L)
    assert np.array_equal(be.dm.get_loglik(), L)


def test_model_finaliser_keeps_its_problem(va, monkeypatch):
    """``vrx_model_destroy`` reads the model's ``vrx_problem``.  A failed case of this file leaves
    model and problem in one reference cycle (the traceback's frames); the collector then ran their
    finalisers in any order, and a problem destroyed first left the model's destructor reading freed
    memory -- seen as ``invalid device ordinal`` from the next launch that asked for the last error.
    The model's finaliser now holds the problem until it has run."""
    import gc
    import weakref
    p = EC.problem_a("gather")
    counts = _counts(p, monkeypatch)
    be = DeviceBackend(p, counts)
    fin_model, fin_counts, alive = be.dm._fin, counts._fin, weakref.ref(counts)
    assert any(a is counts for a in fin_model.peek()[2])
    ring = [be, counts]
    ring.append(ring)                              # model and problem die in one collection
    del be, counts, ring
    gc.collect()
    assert not fin_model.alive and not fin_counts.alive and alive() is None


@pytest.mark.parametrize("name", list(EC.CASES_A))
def test_each_update_against_exact(va, monkeypatch, name):
    p = EC.problem_a(name)
    counts = _counts(p, monkeypatch)
    be = DeviceBackend(p, counts)
    seen = _assert_path(p, be.dm, counts)
    out = EC.run_a(p, be)
    _assert_route(p, be.dm, "A")
    _assert_instances(p, be.dm, seen)
    u_dev = EC.distances_a(p, out)
    u_orc = EC.distances_a(p, EC.run_a(p, EC.OracleBackend(p)))
    _judge("A", name, u_dev, u_orc)


@pytest.mark.parametrize("name", list(EC.CASES_B))
def test_fit_loop_iterations_against_exact(va, monkeypatch, name):
    p = EC.problem_b(name)
    counts = _counts(p, monkeypatch)
    be = DeviceBackend(p, counts)
    seen = _assert_path(p, be.batch or be.dm, counts)
    orc = EC.OracleBackend(p)
    for r in range(p.spec.restarts):
        snaps = EC.run_b(p, be, r)
        if r == 0:
            _assert_route(p, be.batch or be.dm, "B")
        u_dev = EC.distances_b(p, snaps, r)
        if r == 0:
            _assert_launches(p, be)
            _assert_instances(p, be.batch or be.dm, seen)
        u_orc = EC.distances_b(p, EC.run_b(p, orc, r), r)
        _judge("B", name if p.spec.restarts == 1 else "%s[%d]" % (name, r), u_dev, u_orc)
