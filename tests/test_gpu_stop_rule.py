"""Every device stop rule against the reference's loop, case by case, with no tolerance anywhere.

The five device loops (engine Vireo / clone mode, bulk single / cohort, ambient, variant mixtures) call
csrc/vrx_stop.h.  Every expectation here is tests/stop_np.replay -- the reference's ``for it in range(max_iter)`` over
a zero-initialised array -- applied to the DEVICE'S OWN unruled trace U, so a comparison that sits exactly on a
threshold is part of the test: with d_j = U[j] - U[j - 1], ``eps = nextafter(d_j, inf)`` stops at j and
``eps = d_j`` does not (the test is strict).  A ruled fit must then return U[:it + 1] and the state of the unruled
run cut at it, bit for bit.  Which cases exist and where the stops land is computed from replay alone, and the
coverage of the poll-batch positions is asserted before a fit runs.

VIREO_STOP_CASES_OUT=<file> writes the counts of the run (profiles/stop_rule_cases.txt)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import bulk_np as B
from tests import gold
from tests import stop_np as S
from tests import varmix_np as VN
from tests.exact_ambient import run_ambient

pytestmark = pytest.mark.gpu

T = 40                       # iterations of the unruled run
FIT_BATCH = 4                # VIREO_FIT_BATCH, read once per process: its default
BULK_BATCH = 8               # VRX_BULK_BATCH (vrx_bulk.h)
POSITIONS = ("first judged", "last of first batch", "first of second batch", "mid-batch")
COUNTS = {}                  # what the run did, for the report


def count(key, n=1):
    COUNTS[key] = COUNTS.get(key, 0) + n


@pytest.fixture(scope="module")
def va():
    import vireo_amd
    from vireo_amd import _lib
    _lib.require_gpu()                  # fail loudly: there is no CPU fallback
    yield vireo_amd
    path = os.environ.get("VIREO_STOP_CASES_OUT")
    if path:
        with open(path, "w") as f:
            f.write("# tests/test_gpu_stop_rule.py: cases per loop, stops per poll-batch position, rows per verdict of\n"
                    "# the planted table, rows on which two forms disagree.  Every case is an exact comparison of a\n"
                    "# ruled device fit with tests/stop_np.replay on the device's own unruled trace.\n")
            for key in sorted(COUNTS):
                f.write("%-64s %d\n" % (key, COUNTS[key]))


def bits(a, b):
    return S.same_bits(a, b)


def positions(it, mn, mx, first_end, batch):
    """the poll-batch positions of a stop at ``it``: the host enqueues [0, first_end), then ``batch`` at a time"""
    out = set()
    if it == max(mn + 1, 0):
        out.add("first judged")
    e1 = min(mx, first_end)
    if it == e1 - 1:
        out.add("last of first batch")
    if it == e1:
        out.add("first of second batch")
    lo = 0 if it < e1 else e1 + (it - e1) // batch * batch
    hi = e1 if it < e1 else min(mx, lo + batch)
    if lo < it < hi - 1:
        out.add("mid-batch")
    return out


def engine_first_end(mn):
    return max(mn + 2, FIT_BATCH)                               # vrx_model_fit, enqueue_batch


def bulk_first_end(mn):
    return max(max(mn, 0) + 3, BULK_BATCH) - 1                  # bulk_run_passes: pass p closes iteration p - 1


def build_cases(form, traces, first_end, batch, min_iters, reach, allow_negative=True, min_max_iter=1, nan_eps=True):
    """Rules (min_iter, max_iter, eps) built from the unruled traces (one per restart / sample / row that shares the
    rule): thresholds on and beside their own differences, then the rules every loop must take.  -> the list and
    the positions replay says the stops land on."""
    traces = [np.asarray(u) for u in traces]
    n = len(traces[0])
    cases = []
    for u in traces[:2]:
        d = np.diff(u)
        for mn in min_iters:
            for j in range(max(mn + 1, 1), min(mn + 1 + reach, n - 1)):
                if S.decreased(form, u[j - 1], u[j]):
                    continue
                cases.append((mn, n, float(np.nextafter(d[j - 1], np.inf))))     # stops at j at the latest
                cases.append((mn, n, float(d[j - 1])))                           # not at j: the test is strict
    for eps in (0.0, -1.0, np.inf) + ((np.nan,) if nan_eps else ()):
        cases.append((2, n, eps))
    cases += [(10, 10, 1e-2), (12, 10, 1e-2), (n, n, 1e-2)]                      # min_iter >= max_iter
    cases += [(3, mx, np.inf) for mx in (1, 2, 4, 5) if mx >= min_max_iter]      # max_iter 1, 2, min_iter + 1, + 2
    if allow_negative:
        cases += [(-1, mx, eps) for mx in (1, 2, n) for eps in (1e-2, np.inf) if mx >= min_max_iter]
        cases += [(-3, 2, np.inf)]
    seen, out = set(), []
    for c in cases:
        key = (c[0], c[1], np.float64(c[2]).tobytes())
        if key not in seen:
            seen.add(key)
            out.append(c)
    def lands(mn, mx, eps):
        got = set()
        for u in traces:
            it = S.replay(form, u, mn, mx, eps)[0]
            if it < mx - 1:
                got |= positions(it, mn, mx, first_end(mn), batch)
        return got

    landed = set()
    for c in out:
        landed |= lands(*c)
    # a batch position no rule above lands on: look for a threshold of the first trace that does (replay decides)
    d = np.diff(traces[0])
    for mn in range(-1 if allow_negative else 0, n - 4):
        for j in range(max(mn + 1, 1), min(mn + 12, n - 1)):
            if landed >= set(POSITIONS):
                break
            c = (mn, n, float(np.nextafter(d[j - 1], np.inf)))
            new = lands(*c) - landed
            if new:
                out.append(c)
                landed |= new
    return out, landed


# ======================================================================================================================
# the engine: Vireo and clone mode, single models and restart batches
# ======================================================================================================================
class Engine:
    """one problem, one model shape, R starts; every run begins at the saved starts"""

    def __init__(self, va, kind, AD, DP, K, R, seed):
        from vireo_amd import _lib
        from vireo_amd.counts import DeviceCounts
        from vireo_amd.engine import DeviceBatch, DeviceModel
        self.kind, self.R, self.K = kind, R, K
        self.counts = DeviceCounts(AD, DP)
        N, M = AD.shape
        rng = np.random.RandomState(seed)
        self.form = S.BMM if kind == _lib.KIND_BMM else S.VIREO
        if kind == _lib.KIND_VIREO:
            host = va.Vireo(n_cell=M, n_var=N, n_donor=K, ID_prob_init=np.ones((M, K)), GT_prob_init=np.ones((N, K, 3)))
            mu, sm = np.linspace(0.01, 0.99, 3)[None, :], np.full((1, 3), 50.0)
            self.starts = [(rng.dirichlet(np.ones(K), M), rng.dirichlet(np.ones(3), (N, K)), mu, sm) for _ in range(R)]
            push = host._set_device_prior
        else:
            host = va.BinomMixtureVB(n_cell=M, n_var=N, n_donor=K, ID_prob_init=np.ones((M, K)))
            mu, sm = np.full((N, K), 0.5), np.full((N, K), 30.0)
            self.starts = [(rng.dirichlet(np.ones(K), M), None, mu, sm) for _ in range(R)]
            push = host._push_prior
        self.one = DeviceModel(self.counts, kind, K)
        push(self.one)
        self.dm = self.one if R == 1 else DeviceBatch(self.counts, kind, K, R)
        if R > 1:
            push(self.dm)
        self.after = {}

    def close(self):
        if self.dm is not self.one:
            self.dm.close()
        self.one.close()
        self.counts.close()

    def reset(self):
        for r, (ID, GT, mu, sm) in enumerate(self.starts):
            if self.R == 1:
                self.dm.set_state(ID, GT, mu, sm)
            else:
                self.dm.set_restart(r, ID, GT, mu, sm)

    def states(self):
        out = []
        for r in range(self.R):
            if self.R > 1:
                self.dm.copy_to(self.one, r)
            out.append(self.one.get_state())
        return out

    def unruled(self, n, delay):
        """-> (traces [R][n], states) of n iterations from the starts"""
        self.reset()
        tr = np.atleast_2d(self.dm.run_iters(n, delay)[0])
        return tr, self.states()

    def state_after(self, n, delay):
        if n not in self.after:
            self.after[n] = self.unruled(n, delay)[1]
        return self.after[n]

    def fit(self, mx, mn, eps, delay):
        tr, it, flags = self.dm.fit(mx, mn, eps, delay)
        if self.R == 1:
            return [tr], [int(it)], [int(flags)]
        return tr, [int(i) for i in it], [int(f) for f in flags]


def same_state(a, b):
    return all((x is None and y is None) or bits(x, y) for x, y in zip(a, b))


def engine_cases(eng, U, tag):
    min_iters = (-1, 1, 2, 5) if eng.R == 1 else (-1, 2, 5)
    cases, landed = build_cases(eng.form, U, engine_first_end, FIT_BATCH, min_iters, 7 if eng.R == 1 else 6)
    assert landed >= set(POSITIONS), (tag, sorted(landed))     # coverage by construction, from replay alone
    return cases


def check_engine(eng, delay, tag):
    U, full = eng.unruled(T, delay)
    eng.after[T] = full
    cases = engine_cases(eng, U, tag)
    second = mixed = 0
    for mn, mx, eps in cases:
        want = [S.replay(eng.form, U[r], mn, mx, eps) for r in range(eng.R)]
        mixed += len({w[0] for w in want}) > 1 and min(w[0] for w in want) < mx - 1
        eng.reset()
        traces, its, flags = eng.fit(mx, mn, eps, delay)
        got = eng.states()
        for r in range(eng.R):
            it, warn, _ = want[r]
            where = (tag, r, mn, mx, eps, its[r], it)
            assert (its[r], flags[r]) == (it, warn), where
            assert bits(traces[r], U[r][:it + 1]), where
            assert same_state(got[r], eng.state_after(it + 1, delay)[r]), where      # frozen where it stopped
            if it < mx - 1:
                for p in positions(it, mn, mx, engine_first_end(mn), FIT_BATCH):
                    count("engine %s: stops at position '%s'" % (tag.split(" ")[0], p))
        count("engine %s: ruled fits" % tag.split(" ")[0])
        # a second fit behind a stop == the same second fit behind the unruled run (same length for every restart)
        if second < 3 and len({w[0] for w in want}) == 1 and want[0][0] < mx - 1:
            second += 1
            a = eng.fit(8, 1, 1e-2, delay) + (eng.states(),)
            eng.unruled(want[0][0] + 1, delay)
            b = eng.fit(8, 1, 1e-2, delay) + (eng.states(),)
            assert a[1] == b[1] and a[2] == b[2], (tag, mn, mx, eps)
            assert all(bits(x, y) for x, y in zip(a[0], b[0]))
            assert all(same_state(x, y) for x, y in zip(a[3], b[3]))
            count("engine %s: second fits behind a stop" % tag.split(" ")[0])
    assert second >= 1 or eng.R > 1
    assert mixed >= 1 or eng.R == 1       # some restart stopped and stayed frozen while the others ran on
    count("engine %s: fits whose restarts stop at different iterations" % tag.split(" ")[0], int(mixed))


def _engine_data(name):
    from vireo_amd import _lib, synth
    if name == "c1":
        return (_lib.KIND_VIREO,) + gold.c1() + (4,)
    if name == "mito":
        return (_lib.KIND_BMM,) + gold.mito() + (3,)
    return (_lib.KIND_BMM,) + synth.clone_workload(40, 2000, 3) + (3,)


@pytest.fixture(scope="module")
def engines(va):
    made = {}

    def get(name, R):
        if (name, R) not in made:
            kind, AD, DP, K = _engine_data(name)
            made[name, R] = Engine(va, kind, AD.tocsc(), DP.tocsc(), K, R, seed=17 + R)
        return made[name, R]
    yield get
    for e in made.values():
        e.close()


ENGINE_RUNS = [("c1", 0), ("c1", 3), ("mito", 0), ("clone", 0)]


@pytest.mark.parametrize("ride", [0, 1])
@pytest.mark.parametrize("pipeline", [0, 1])
@pytest.mark.parametrize("R", [1, 5])
@pytest.mark.parametrize("name,delay", ENGINE_RUNS)
def test_engine_stop_rule(engines, monkeypatch, name, delay, R, pipeline, ride):
    monkeypatch.setenv("VIREO_FIT_PIPELINE", str(pipeline))
    monkeypatch.setenv("VIREO_ELBO_RIDE", str(ride))
    assert os.environ.get("VIREO_FIT_BATCH") in (None, str(FIT_BATCH))
    eng = engines(name, R)
    eng.after = {}                                            # (the unruled states of THIS configuration)
    check_engine(eng, delay, "%s delay=%d R=%d pipeline=%d ride=%d" % (name, delay, R, pipeline, ride))


# ======================================================================================================================
# bulk, single and cohort
# ======================================================================================================================
def bulk_check(form_tag, U, fit, unruled_state, n_sample):
    """U [S][T]; fit(mn, mx, eps) -> (psi [S][K], theta [S][G], traces [S][mx] zero padded, it [S])"""
    cases, landed = build_cases(S.EM, U, bulk_first_end, BULK_BATCH, (-1, 0, 3), 8)
    assert landed >= set(POSITIONS), sorted(landed)
    both, mixed = set(), 0
    for mn, mx, eps in cases:
        psi, theta, traces, its = fit(mn, mx, eps)
        want_its = [S.replay(S.EM, U[s], mn, mx, eps)[0] for s in range(n_sample)]
        mixed += len(set(want_its)) > 1 and min(want_its) < mx - 1
        for s in range(n_sample):
            it, _, kept = S.replay(S.EM, U[s], mn, mx, eps)
            where = (form_tag, s, mn, mx, eps, int(its[s]), it)
            assert int(its[s]) == it, where
            want = np.zeros(mx)
            want[:it + 1] = U[s][:it + 1]
            assert bits(traces[s], want), where
            wpsi, wtheta = unruled_state(it + 1)
            assert bits(psi[s], wpsi[s]) and bits(theta[s], wtheta[s]), where
            if it < mx - 1:
                both |= positions(it, mn, mx, bulk_first_end(mn), BULK_BATCH)
                for p in positions(it, mn, mx, bulk_first_end(mn), BULK_BATCH):
                    count("bulk %s: stops at position '%s'" % (form_tag, p))
        count("bulk %s: ruled fits" % form_tag)
    return both, mixed


def test_bulk_single_stop_rule(va):
    from vireo_amd.vireo_bulk import BulkData
    AD, DP, GT = B.c1_bulk()
    psi0, theta0 = np.random.RandomState(3).dirichlet(np.ones(GT.shape[1])), np.array([0.01, 0.5, 0.99])
    with BulkData(AD, DP, GT) as bd:
        def run(mn, mx, eps):
            psi, theta, tr, it, _ = bd.fit(psi0, theta0, max_iter=mx, min_iter=mn, epsilon_conv=eps)
            full = np.zeros(mx)
            full[:it + 1] = tr
            return [psi], [theta], [full], [it]
        U = [run(T, T, 0.0)[2][0]]
        assert run(T, T, 0.0)[3] == [T - 1]
        cache = {}

        def state(n):
            if n not in cache:
                cache[n] = run(n, n, 0.0)[:2]
            return cache[n]
        bulk_check("single", U, run, state, 1)


def test_bulk_cohort_stop_rule(va):
    from vireo_amd import _lib
    from vireo_amd.vireo_bulk import BulkData
    g = gold.load("c1_bulk_cohort")
    _, _, GT = B.c1_bulk()
    n_s = g["AD"].shape[0]
    chunk = int(_lib.lib().vrx_bulk_cohort_chunk())
    assert n_s == 6 and 1 < chunk < n_s and n_s % chunk != 0       # a chunk boundary, and a last chunk not full
    AD, DP = g["AD"].astype(np.int64), g["DP"].astype(np.int64)
    with BulkData(AD[0], DP[0], GT) as bd:
        bd.set_cohort(AD, DP)

        def run(mn, mx, eps):
            psi, theta, tr, it, _ = bd.fit_cohort(g["psi0"], g["theta0"], max_iter=mx, min_iter=mn, epsilon_conv=eps)
            return psi, theta, tr, it
        U = run(T, T, 0.0)[2]
        cache = {}

        def state(n):
            if n not in cache:
                cache[n] = run(n, n, 0.0)[:2]
            return cache[n]
        _, mixed = bulk_check("cohort", U, run, state, n_s)
        assert mixed >= 1      # under some rule the samples stop at different iterations: a stopped one stays frozen
        count("bulk cohort: fits whose samples stop at different iterations", int(mixed))


# ======================================================================================================================
# variant mixtures
# ======================================================================================================================
def test_varmix_stop_rule(va):
    from vireo_amd import _lib
    from vireo_amd.variant_mixture import VariantMixtures
    wave = int(_lib.lib().vrx_varmix_wave_rows())
    lengths = [wave + 70, wave + 1, wave, wave - 1, 129, 128, 65, 64, 63, 17, 5, 2, 1, 0] + list(range(3, 300, 1))[:226]
    AD, DP = VN.gen_rows(lengths, seed=77)
    assert 200 <= len(lengths) <= 400
    Tv = 30
    with VariantMixtures(AD, DP) as vm:
        for K in (2, 3):
            full = vm.fit(n_clone=K, max_iter=Tv, min_iter=Tv, epsilon_conv=0.0, return_trace=True)
            U = full["trace"]
            assert all(len(u) == Tv for u in U)
            cache = {Tv: full}

            def cut(n):
                if n not in cache:
                    cache[n] = vm.fit(n_clone=K, max_iter=n, min_iter=n, epsilon_conv=0.0)
                return cache[n]
            # rules on and beside the differences of a long row and a short one, then the common ones
            # (vrx_varmix_fit takes no negative min_iter, no max_iter below 2 and no NaN epsilon_conv)
            cases, _ = build_cases(S.BMM, [U[0], U[9]], lambda mn: 0, 1, (0, 2), 5, allow_negative=False, min_max_iter=2,
                                   nan_eps=False)
            n_stop = 0
            for mn, mx, eps in cases:
                got = vm.fit(n_clone=K, max_iter=mx, min_iter=mn, epsilon_conv=eps, return_trace=True)
                for v in range(len(lengths)):
                    it, warn, _ = S.replay(S.BMM, U[v], mn, mx, eps)
                    where = (K, v, mn, mx, eps, int(got["n_iter"][v]), it)
                    assert (int(got["n_iter"][v]), int(got["warn"][v])) == (it, warn), where
                    assert bits(got["trace"][v], U[v][:it + 1]), where
                    assert bits([got["elbo"][v]], [U[v][it - 1]]), where
                    want = cut(it + 1)
                    for key in ("beta_mu", "beta_sum", "size", "elbo_one"):
                        assert bits(got[key][v], want[key][v]), where + (key,)
                    n_stop += it < mx - 1
                count("varmix K=%d: ruled fits" % K)
            count("varmix K=%d: rows stopped by the rule" % K, int(n_stop))
            assert n_stop > 0


# ======================================================================================================================
# ambient: no trace is exposed
# ======================================================================================================================
def test_ambient_stop_rule(va):
    from vireo_amd.counts import DeviceCounts
    AD, DP, theta, sel, psi0 = S.ambient_inputs()
    K = theta.shape[1]
    # (the rule gives at most 8 distinct counts by the restatement alone: tests/test_stop_rule_cpu.py)
    counts = DeviceCounts(AD, DP)
    try:
        r = S.AMBIENT_RULE
        psi, var, llr, n_iter = run_ambient(counts, K, theta, sel, psi0, r["min_iter"], r["max_iter"], r["eps"])
        groups = sorted(set(n_iter.tolist()))
        assert len(groups) <= 8 and len(groups) >= 3
        assert all(r["min_iter"] < it <= r["max_iter"] - 1 for it in groups)
        for it in groups:
            fpsi, fvar, fllr, fit = run_ambient(counts, K, theta, sel, psi0, it + 1, it + 1, 0.0)
            assert np.all(fit == it)
            cells = n_iter == it
            assert bits(psi[cells], fpsi[cells]) and bits(var[cells], fvar[cells]) and bits(llr[cells], fllr[cells]), it
            count("ambient: cells leaving at it = %d" % it, int(cells.sum()))
        count("ambient: forced calls", len(groups))
    finally:
        counts.close()


# ======================================================================================================================
# the device compile of the judge
# ======================================================================================================================
def test_device_judge_equals_the_restatement_on_the_planted_table(va):
    from vireo_amd import _lib
    ri, rd = S.table()
    want_v, want_p = S.table_verdicts(ri, rd)
    n = len(ri)
    got_v, got_p = np.full(n, -7, np.int32), np.full(n, -7.0)
    ri_c, rd_c = np.ascontiguousarray(ri, np.int32), np.ascontiguousarray(rd, np.float64)
    i32 = C.POINTER(C.c_int32)
    _lib.check(_lib.lib().vrx_stop_verdicts(0, n, ri_c.ctypes.data_as(i32), _lib.dptr(rd_c), got_v.ctypes.data_as(i32),
                                            _lib.dptr(got_p)))
    bad = np.flatnonzero(got_v != want_v)
    assert bad.size == 0, (ri[bad[:5]], rd[bad[:5]], got_v[bad[:5]], want_v[bad[:5]])
    assert bits(got_p, want_p)
    for form in S.FORMS:
        for v in range(4):
            count("judge %s: rows with verdict %s" % (S.FORM_NAMES[form], S.VERDICT_NAMES[v]),
                  int(np.sum((ri[:, 0] == form) & (got_v == v))))
    a, b, c = (got_v[ri[:, 0] == f] for f in S.FORMS)
    count("judge: rows on which vireo and bmm disagree", int(np.sum(a != b)))
    count("judge: rows on which vireo and em disagree", int(np.sum(a != c)))
    assert np.sum(a != b) > 0 and np.sum(a != c) > 0
