"""Long-lived device models held to their visible state, call by call (tests/seq_np.py).

Property 1, history independence: a call on a ``DeviceModel`` / ``DeviceBatch`` with a history gives
the bits it gives on a fresh model that was handed the visible state sigma -- results, ELBO parts,
and sigma afterwards.  Both sides take the same entry point under the same environment and the
library has no atomics: there is no tolerance.  Property 2, observation is true: what the device
returned and shows after a sequence is what the float64 oracle driven through the same sequence
holds, within the tolerance of tests/test_gpu_fuzz.py for chains of a few iterations (KL_ID and
KL_GT with the absolute floor of their float64 sums, seq_np.part_floors: at a posterior that still
sits at its prior they are residues of 1e-11).

Three families of sequences per configuration: every ordered pair of the alphabet behind the common
prelude (one test per first call), the production sequences of restarts.py and bmm_model.py, and
eight seeded walks of twelve calls.  The configurations name their data and environment the way
tests/exact_cases.py does, and ``info()`` must report the path before anything is compared.

What this file decided: a fit DOES leave logLik_ID of its last iteration on the device on every
path, tiled cell streams with several ranges or split rows included (the softmax kernel stores the
row it summed) -- ``get_loglik`` after ``fit`` / ``run_iters`` is the oracle's logLik_ID, and a fresh
model given it through ``set_loglik`` computes the same ELBO bits.

The run appends one line per configuration to profiles/model_sequences_cases.txt: sequences, calls,
the worst oracle distance of property 2 and where it sits, seconds.
"""
import copy
import os
import time

import numpy as np
import pytest

from tests import exact_cases as EC
from tests import seq_np as Q
from tests.test_gpu_fuzz import ATOL, RTOL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "model_sequences_cases.txt")
_STATS = {}


@pytest.fixture(scope="module")
def va():
    import vireo_amd
    from vireo_amd import _lib
    _lib.require_gpu()          # fail loudly: there is no CPU fallback
    assert (_lib.STEP_THETA, _lib.STEP_GT, _lib.STEP_ID, _lib.STEP_LOGLIK, _lib.STEP_ELBO, _lib.STEP_SOFTMAX) == (
        Q.STEP_THETA, Q.STEP_GT, Q.STEP_ID, Q.STEP_LOGLIK, Q.STEP_ELBO, Q.STEP_SOFTMAX)
    yield vireo_amd
    if _STATS:
        with open(PROFILE, "a") as f:
            for name, s in _STATS.items():
                f.write("%-20s sequences %4d  calls %6d  worst distance %.3e at %-12s %7.2f s\n"
                        % (name, s["sequences"], s["calls"], s["worst"], s["where"], s["seconds"]))


class DeviceFactory:
    """the device's models of a configuration, in the place of seq_np.RefFactory"""

    def __init__(self, cfg, monkeypatch):
        from vireo_amd import _lib
        from vireo_amd.counts import DeviceCounts
        for k, v in cfg.env.items():
            monkeypatch.setenv(k, v)
        self.cfg, self.L = cfg, _lib
        self.AD, self.DP = EC.data(cfg.data)
        self.counts = DeviceCounts(self.AD, self.DP)
        self.kind = _lib.KIND_VIREO if cfg.kind == "vireo" else _lib.KIND_BMM
        self.kw = dict(n_gt=cfg.T if cfg.kind == "vireo" else 3, learn_gt=cfg.learn_gt, learn_theta=cfg.learn_theta,
                       ase_mode=cfg.ase, fix_beta_sum=cfg.fix)
        self.refusals = (_lib.VrxError,)

    def single(self):
        from vireo_amd.engine import DeviceModel
        return DeviceModel(self.counts, self.kind, self.cfg.K, **self.kw)

    def batch(self):
        from vireo_amd.engine import DeviceBatch
        return DeviceBatch(self.counts, self.kind, self.cfg.K, self.cfg.R, **self.kw)

    def assert_path(self):
        """the kernels and tilings the configuration names are the ones its models run"""
        m = self.batch() if self.cfg.R > 1 else self.single()
        seen = dict(m.info(), **self.counts.build_info())
        m.close()
        for k, v in self.cfg.want.items():
            assert v(seen[k]) if callable(v) else seen[k] == v, (self.cfg.name, k, seen[k])


class _Tally:
    def __init__(self, name):
        self.name, self.t0, self.bad = name, time.perf_counter(), []
        cfg = Q.CONFIGS[name]
        self.floors = Q.part_floors(cfg, *EC.data(cfg.data)[0].shape)
        self.s = _STATS.setdefault(name, dict(sequences=0, calls=0, worst=0.0, where="-", seconds=0.0))

    def judge(self, tag, diff, dev, ref):
        """diff: what property 1 found; property 2: dev against ref"""
        d, where = Q.distance(dev, ref, ATOL, self.floors)
        print("%-18s %-34s property 1: %-12s property 2: %.3e %s" % (self.name, tag, diff or "same bits", d, where or ""))
        self.s["sequences"] += 1
        if d > self.s["worst"]:
            self.s["worst"], self.s["where"] = d, where
        if diff:
            self.bad.append((tag, "history shows in", diff))
        if not d <= RTOL:
            self.bad.append((tag, "oracle distance", d, where))

    def calls(self, *trails):
        self.s["calls"] += sum(t.calls for t in trails)

    def done(self):
        self.s["seconds"] += time.perf_counter() - self.t0
        assert not self.bad, self.bad


def _tail(trail, n=1):
    t = Q.Trail()
    t.results, t.parts, t.after_refusal = trail.results[-n:], trail.parts[-n:], trail.after_refusal[-n:]
    t.seen = trail.seen
    return t


def _copy_shadow(sh):
    sh = copy.copy(sh)
    sh.stage = dict(sh.stage)
    return sh


PAIR_CASES = [(name, a.name) for name in Q.GPU_CONFIGS if 1 in Q.CONFIGS[name].families
              for a in Q.alphabet(Q.CONFIGS[name])]


@pytest.mark.parametrize("name,first", PAIR_CASES, ids=["%s-%s" % c for c in PAIR_CASES])
def test_every_pair_behind_one_first_call(va, monkeypatch, name, first):
    """family 1: prelude, a, b for every b.  History side: one model through all of it.  Fresh side:
    sigma behind a -- itself reached by fresh models call by call -- uploaded to a new model, then b."""
    cfg = Q.CONFIGS[name]
    x, f, rf = Q.arguments(cfg), DeviceFactory(cfg, monkeypatch), Q.RefFactory(cfg)
    f.assert_path()
    tally = _Tally(name)
    P = Q.prelude(cfg)
    a = Q.pairs_from(cfg, first)[0][0]
    pre = Q.twin(f, P + [a], x)
    tally.calls(pre)
    ref_sys, ref_sh = Q.System(rf), Q._Shadow(cfg)
    Q.run(rf, P + [a], x, ref_sys, ref_sh, watch=False)
    for _, b in Q.pairs_from(cfg, first):
        straight = Q.run(f, P + [a, b], x)
        fresh = Q.twin(f, [b], x, start=(pre.sigma, pre.shadow))
        diff = Q.differences(straight, fresh, last_only=True)
        if not all(Q.same_bits(p, q) for p, q in zip(straight.results[-2] or [], pre.results[-1] or [])):
            diff.append("result of the first call")
        ref = Q.run(rf, [b], x, ref_sys.clone(), _copy_shadow(ref_sh))
        tally.judge("%s,%s" % (first, b.name), diff, _tail(straight), ref)
        tally.calls(straight, fresh)
    tally.done()


@pytest.mark.parametrize("name", [n for n in Q.GPU_CONFIGS if 2 in Q.CONFIGS[n].families])
def test_production_sequences(va, monkeypatch, name):
    """family 2: the restart search of restarts.py (run / submit, snapshot on each new best, winner with
    its refinement) or clone mode's initialisation loop, as one model lives through them"""
    cfg = Q.CONFIGS[name]
    x, f, rf = Q.arguments(cfg), DeviceFactory(cfg, monkeypatch), Q.RefFactory(cfg)
    f.assert_path()
    tally = _Tally(name)
    for tag, seq in Q.production(cfg).items():
        straight, fresh, ref = Q.run(f, seq, x), Q.twin(f, seq, x), Q.run(rf, seq, x)
        tally.judge(tag, Q.differences(straight, fresh), straight, ref)
        tally.calls(straight, fresh)
    tally.done()


@pytest.mark.parametrize("name", [n for n in Q.GPU_CONFIGS if 3 in Q.CONFIGS[n].families])
def test_seeded_walks(va, monkeypatch, name):
    """family 3: eight walks of twelve calls behind the prelude"""
    cfg = Q.CONFIGS[name]
    x, f, rf = Q.arguments(cfg), DeviceFactory(cfg, monkeypatch), Q.RefFactory(cfg)
    f.assert_path()
    tally = _Tally(name)
    P = Q.prelude(cfg)
    for k, w in enumerate(Q.walks(cfg)):
        seq = P + w
        straight, fresh, ref = Q.run(f, seq, x), Q.twin(f, seq, x), Q.run(rf, seq, x)
        tally.judge("walk%d %s" % (k, ",".join(c.name for c in w)), Q.differences(straight, fresh), straight, ref)
        tally.calls(straight, fresh)
    tally.done()


def test_refused_calls_leave_sigma_alone(va, monkeypatch):
    """the three refusals of the alphabet on a model in the middle of its life: nothing visible moves,
    bit for bit, and the ELBO parts of the call before are still there"""
    cfg = Q.CONFIGS["gather_fused"]
    x, f = Q.arguments(cfg), DeviceFactory(cfg, monkeypatch)
    A = {c.name: c for c in Q.alphabet(cfg)}
    sysm, sh = Q.System(f), Q._Shadow(cfg)
    try:
        m = sysm.single
        m.set_prior(*x.default_prior)
        m.set_state(*x.start[0])
        trace, _ = m.run_iters(3, 0)
        parts = m.elbo_parts()
        before = Q.read_sigma(sysm)
        for c in (A["restore"], A["staged_0"], A["step_unknown"]):
            assert c.refused(sh)
            with pytest.raises(f.refusals):
                c.fn(sysm, x)
            after = Q.read_sigma(sysm)
            for p, q in zip(before.state + (before.L,), after.state + (after.L,)):
                assert Q.same_bits(p, q), c.name
            assert Q.same_bits(parts, m.elbo_parts()), c.name
        assert trace[-1] == parts[0] - parts[1] - parts[2] - parts[3]
    finally:
        sysm.close()
