"""The sequence machinery of tests/seq_np.py before it meets a GPU.

* ``RefModel`` driven through the reference's own sequences gives the pinned NumPy fits of the real
  reference (tests/golden/c1_onestep, c1_trace_seed2), bit for bit.
* ``twin`` on RefModel, and on LazyRef without a planted defect, is an identity: a deferral handled
  right is invisible.
* Every planted defect of LazyRef is caught by property 1 (history independence, bit for bit) or
  property 2 (observation against RefModel) in EACH of family 1 (ordered pairs) and family 3 (seeded
  walks); the table of which pair catches which defect is printed.  A defect only a production
  sequence catches would mean the alphabet is too small.
No GPU.
"""
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import vireo_oracle as O
from tests import gold
from tests import seq_np as Q
from tests.test_gpu_fuzz import ATOL, RTOL


def eq(a, b):
    np.testing.assert_array_equal(np.asarray(a), np.asarray(b))


def _c1_model():
    AD, DP = gold.c1()
    cfg = SimpleNamespace(name="c1", kind="vireo", K=4, T=3, ase=False, fix=False, learn_gt=True, learn_theta=True, R=1)
    m = Q.RefModel(cfg, AD, DP)
    m.set_prior(*Q.default_prior(cfg))
    return m, AD, DP


def _check_state(m, g, pre):
    for got, k in zip(m.get_state(), ("ID_prob", "GT_prob", "beta_mu", "beta_sum")):
        eq(got, g[pre + k])


def test_refmodel_steps_are_the_references():
    g = gold.load("c1_onestep")
    m, AD, DP = _c1_model()
    m.set_state(*(g["s0_" + k] for k in ("ID_prob", "GT_prob", "beta_mu", "beta_sum")))
    m.step(Q.STEP_THETA)
    _check_state(m, g, "s1_")
    m.step(Q.STEP_GT)
    _check_state(m, g, "s2_")
    m.step(Q.STEP_ID)
    _check_state(m, g, "s3_")
    eq(m.get_loglik(), g["logLik_ID"])
    assert m.step(Q.STEP_ELBO) == g["ELBO"]
    p = m.elbo_parts()
    assert p[0] - p[1] - p[2] - p[3] == g["ELBO"]
    m.set_loglik(np.zeros_like(g["logLik_ID"]))
    m.step(Q.STEP_LOGLIK)                              # get_ELBO(None, AD, DP): logLik_ID recomputed
    assert m.step(Q.STEP_ELBO) == g["ELBO_recompute"]


def test_refmodel_warm_restart_is_the_references():
    """Vireo.fit twice on one model (vireo_model.py:278-315): the restart's fit, then the refinement"""
    g = gold.load("c1_trace_seed2")
    m, AD, DP = _c1_model()
    const = O.binom_const(AD, DP)
    m.set_state(*(g["init_" + k] for k in ("ID_prob", "GT_prob", "beta_mu", "beta_sum")))
    tr, it, _ = m.fit(20, 5, 1e-2, 3)
    assert it == int(g["n_first"]) == 19 and len(tr) == it + 1
    _check_state(m, g, "mid_")
    m.snapshot()
    tr2, it2, _ = m.fit(200, 5, 1e-2, 0)
    eq(np.append(tr[:it] + const, tr2[:it2] + const), g["ELBO_"])
    _check_state(m, g, "end_")
    m.restore()
    _check_state(m, g, "mid_")


CPU = ("cpu_single", "cpu_batch", "cpu_clone")


def _sequences(cfg):
    """(family, name, sequence) of a configuration, the prelude in front of families 1 and 3"""
    P = Q.prelude(cfg)
    for a in Q.alphabet(cfg):
        for _, b in Q.pairs_from(cfg, a.name):
            yield 1, "%s,%s" % (a.name, b.name), P + [a, b]
    for name, seq in Q.production(cfg).items():
        yield 2, name, seq
    for k, w in enumerate(Q.walks(cfg)):
        yield 3, "walk%d" % k, P + w


@pytest.mark.parametrize("name", CPU)
@pytest.mark.parametrize("cls", (Q.RefModel, Q.LazyRef))
def test_twin_is_an_identity_on_a_right_model(name, cls):
    """property 1 on the oracle itself, and on the oracle that defers: every result and everything
    visible afterwards is the same bits; LazyRef's results are RefModel's"""
    cfg = Q.CONFIGS[name]
    x, f, ref = Q.arguments(cfg), Q.RefFactory(cfg, cls), Q.RefFactory(cfg)
    n = 0
    for fam, tag, seq in _sequences(cfg):
        if fam == 1 and n % 7:              # (a seventh of the pairs, every walk, every production sequence)
            n += 1
            continue
        n += 1
        straight, tw = Q.run(f, seq, x), Q.twin(f, seq, x)
        assert Q.differences(straight, tw) == [], (name, tag)
        if cls is Q.LazyRef:
            assert Q.differences(straight, Q.run(ref, seq, x)) == [], (name, tag)


def _caught(cfg, x, wrong, fam, tag, seq, ref_trail):
    """-> which property sees the defect on this sequence: "1", "2", "12" or "" """
    f = Q.RefFactory(cfg, Q.LazyRef, wrong=wrong)
    straight = Q.run(f, seq, x)
    how = ""
    if Q.differences(straight, Q.twin(f, seq, x)):
        how += "1"
    if Q.distance(straight, ref_trail, ATOL)[0] > RTOL:
        how += "2"
    return how


@pytest.fixture(scope="module")
def reference_trails():
    out = {}
    for name in CPU:
        cfg = Q.CONFIGS[name]
        x, ref = Q.arguments(cfg), Q.RefFactory(cfg)
        out[name] = {(fam, tag): Q.run(ref, seq, x) for fam, tag, seq in _sequences(cfg)}
    return out


@pytest.mark.parametrize("wrong", Q.DEFECTS)
def test_every_planted_defect_is_caught_in_pairs_and_in_walks(wrong, reference_trails):
    name = "cpu_batch" if wrong in Q.BATCH_DEFECTS else "cpu_single"
    cfg = Q.CONFIGS[name]
    x = Q.arguments(cfg)
    hits = {1: [], 2: [], 3: []}
    for fam, tag, seq in _sequences(cfg):
        how = _caught(cfg, x, wrong, fam, tag, seq, reference_trails[name][fam, tag])
        if how:
            hits[fam].append("%s(%s)" % (tag, how))
    for fam in (1, 2, 3):
        print("%-30s family %d: %3d sequences catch it: %s" % (wrong, fam, len(hits[fam]), " ".join(hits[fam][:12])))
    assert hits[1] and hits[3], (wrong, {k: len(v) for k, v in hits.items()})


def test_the_stop_epsilon_separates_the_slots():
    """the batch fit of the alphabet stops its slots at different iterations"""
    cfg = Q.CONFIGS["cpu_batch"]
    x = Q.arguments(cfg)
    sysm, sh = Q.System(Q.RefFactory(cfg)), Q._Shadow(cfg)
    Q.run(sysm.f, Q.prelude(cfg), x, sysm, sh, watch=False)
    _, its, _ = sysm.batch.fit(Q.STOP_RULE[1], Q.STOP_RULE[0], x.eps_stop)
    assert len(set(its.tolist())) >= 2
