"""The ambient harness checked without a GPU: float64 NumPy stands in the device's place.

* On every output of every case of tests/exact_ambient.py the float64 restatement (tests/ambient_np.py) stays
  inside the a-priori bound of recursive summation -- a cell's entries + K + 16 units for the EM, a variant's
  entries + 16 for the gain.  A degenerate unit or a restatement of something else would show here.
* The rule has teeth: a float64 copy of the device's schedule (64-entry chunks, the fma chains of t1 and t0,
  r_k in entry order, the butterfly of the log-likelihood, the M step's index-order sum; the series digamma and
  the two-pass logsumexp of the gain) passes the rule as it stands and fails it when made wrong the way a kernel
  would be, on the case written for that defect.
* The exact side agrees with two statements written independently of it: ``fit_cell(dtype=np.longdouble)`` and
  the 40-digit gain of tests/test_gpu_postfit_sweep.py.
* The cases are what they say, and the library's cap is what the Python copy says.
"""
import numpy as np
import pytest

from tests import ambient_np as A
from tests import exact_ambient as XA
from tests import exact_np as X


# ---------------------------------------------------------------- the float64 side within its a-priori bound
@pytest.mark.parametrize("name", list(XA.EM))
def test_float64_em_within_a_priori_bound(name):
    rows = []
    p = XA.run(name, XA.ORACLE, rows, {})           # the whole protocol of the case, float64 on both sides
    assert rows
    for n in p.spec.lengths:
        per_cell = XA.cell_distances(p, XA.ORACLE.run(p, p.psi0, n, None), XA.exact_from_start(name, n))
        assert set(per_cell) == set(np.flatnonzero(p.counted))
        for c, u in per_cell.items():
            assert max(u.values()) <= XA.a_priori(p, c), (name, n, c, u)
    far = max(rows, key=lambda r: r[4])
    print("%s: %d cells, worst %.3f units (%s %s)" % (name, p.M, far[4], far[1], far[2]))


@pytest.mark.parametrize("name", list(XA.GAIN))
def test_float64_gain_within_a_priori_bound(name):
    rows = []
    g = XA.run_gain(name, XA.ORACLE, rows, {})
    u = XA.gain_units(g, XA.ORACLE.gain(g, None))
    assert rows and np.all(u <= g.entries + 16), (name, u.max())
    print("%s: worst %.3f units, %d distinct digamma arguments" % (name, u.max(), np.unique(XA.gain_shapes(g)).size))


# ---------------------------------------------------------------- the rule has teeth
def _units(p, side, budget, cells=None):
    n = p.spec.lengths[0]
    per_cell = XA.cell_distances(p, side.run(p, p.psi0, n, budget), XA.exact_from_start(p.name, n))
    if cells is not None:
        per_cell = {c: per_cell[c] for c in cells}
    return XA.worst(per_cell)


# case, defect, VIREO_AMBIENT_LDS of the route (None: default), the outputs that must fail
TEETH = [("teeth_last_read", "skip_last", None, ("psi",)),
         ("teeth_last_read", "twice_64", None, ("psi",)),
         ("teeth_close_theta", "stale_rows", 0, ("psi",)),
         ("teeth_r64", "r64_stale", None, ("psi", "var")),
         ("teeth_last_read", "fisher_b", None, ("var",)),
         ("argmax_change", "old_argmax", None, ("llr",))]


@pytest.mark.parametrize("name,wrong,budget,outputs", TEETH)
def test_a_defect_fails_the_rule(name, wrong, budget, outputs):
    p = XA.problem(name)
    cells = p.flip if wrong == "old_argmax" else None
    u_orc = _units(p, XA.ORACLE, budget, cells)
    u_copy = _units(p, XA.CopySide(), budget, cells)
    u_bad = _units(p, XA.CopySide(wrong), budget, cells)
    for k in XA.OUTPUTS:
        print("%s %-4s float64 %.2f  schedule copy %.2f  %s %.3g" % (name, k, u_orc[k], u_copy[k], wrong, u_bad[k]))
        assert X.held(u_copy[k], u_orc[k]), k           # the copy as it stands is held
    for k in outputs:
        assert not X.held(u_bad[k], u_orc[k]), k


def test_the_defects_are_the_subtle_ones():
    """what each case puts where the defect bites"""
    p = XA.problem("teeth_last_read")
    for c in range(3):                                  # 65 entries: entry 64 is the last one, of one read among 5 000
        a, b, _ = p.cells[c]
        assert a.size == 65 and a[64] + b[64] == 1 and np.all(a[:64] + b[:64] == 5000)
    p = XA.problem("teeth_close_theta")
    assert XA.route_cap(p.K, 0) == 0 and p.n_sel[:3].min() > 64
    step = np.diff(p.theta, axis=0)
    assert np.all(np.abs(step - 1e-7) < 1e-15)
    p = XA.problem("teeth_r64")
    assert p.K == 65 and np.all(p.psi0[:, 64] == 1e-9)
    p = XA.problem("argmax_change")
    assert len(p.flip) >= 1
    for c in p.flip:                                    # the largest component moves between update 1 and update 2
        a, b, th = p.cells[c]
        one = X.ambient_cell(a, b, th, p.psi0[c], 1)["psi"][0]
        two = X.ambient_cell(a, b, th, p.psi0[c], 2)["psi"][0]
        assert np.argmax(one) != np.argmax(two)


def test_the_copy_is_held_on_both_routes():
    """the schedule copy, cached and uncached, on cells of one, two and three chunks"""
    p = XA.problem("K3")
    for budget in (None, 0):
        u_orc, u_copy = _units(p, XA.ORACLE, budget), _units(p, XA.CopySide(), budget)
        for k in XA.OUTPUTS:
            assert X.held(u_copy[k], u_orc[k]), (budget, k, u_copy[k])


def test_gain_defects_fail_the_rule():
    copy = XA.CopySide()
    # the recurrence of digamma stopped at x >= 6 instead of 10: integer shapes of 6 .. 9.5
    g = XA.gain_problem("N256_K7_pc0.5_onehot")
    u_orc = XA.gain_units(g, XA.ORACLE.gain(g, None)).max()
    u_copy = XA.gain_units(g, copy.gain(g, None)).max()
    u_bad = XA.gain_units(g, copy.gain(g, None, switch=6.0)).max()
    print("digamma: float64 %.2f  copy %.2f  switch at 6 %.3g" % (u_orc, u_copy, u_bad))
    assert X.held(u_copy, u_orc) and not X.held(u_bad, u_orc)
    shapes = XA.gain_shapes(g)
    assert ((shapes >= 6) & (shapes < 10)).any()
    # the smallest term of the logsumexp dropped at K = 40
    g = XA.gain_problem("N256_K40_pc0.5_onehot")
    u_orc = XA.gain_units(g, XA.ORACLE.gain(g, None)).max()
    good, bad = copy.gain(g, None), copy.gain(g, None, drop_smallest=True)
    u_copy, u_bad = XA.gain_units(g, good), XA.gain_units(g, bad)
    failing = u_bad > X.bound(u_orc)
    share = -np.expm1(bad - good)                       # what the dropped term was of the sum
    print("logsumexp: float64 %.2f  copy %.2f  smallest term dropped %.3g; it fails on %d of %d variants, the "
          "smallest share that fails %.3g" % (u_orc, u_copy.max(), u_bad.max(), failing.sum(), g.N, share[failing].min()))
    assert g.K == 40 and X.held(u_copy.max(), u_orc) and not X.held(u_bad.max(), u_orc)
    assert share[failing].min() < 1e-6


# ---------------------------------------------------------------- the exact side against independent statements
@pytest.mark.parametrize("name,n", [("K3", 2), ("K16", 2), ("long_small", 3), ("long_K65", 7)])
def test_ambient_cell_agrees_with_fit_cell_in_long_double(name, n):
    p = XA.problem(name)
    seen = 0
    for c, (a, b, th) in enumerate(p.cells):
        if not p.counted[c]:
            continue
        ex = X.ambient_cell(a, b, th, p.psi0[c], n)
        psi, var, llr, it = A.fit_cell(a, b, th, p.psi0[c], min_iter=n, max_iter=n, eps=0.0, dtype=np.longdouble)
        assert it == n - 1
        assert np.max(np.abs(psi - ex["psi"][0]) / ex["psi"][0]) < 1e-17, (name, c)
        assert np.max(np.abs(var - ex["var"][0]) / ex["var"][0]) < 1e-17, (name, c)
        assert abs(llr - ex["llr"][0]) < 1e-17 * abs(ex["llr"][0]), (name, c)
        seen += 1
    assert seen >= 10


def test_elbo_gain_agrees_with_forty_digits():
    """the sweep's exact integer sums and mpmath against the long-double products of ``elbo_gain``"""
    import mpmath
    from tests.test_gpu_postfit_sweep import _exact_gain
    g = XA.gain_problem("N255_K3_pc10_zeros")
    rows = np.arange(0, g.N, 5)
    value, unit = XA.gain_exact(g)
    want = _exact_gain(g.AD, g.DP, g.ID, rows, g.pc)
    far = max(float(abs(X._mp(value[r]) - w)) / float(unit[r]) for r, w in zip(rows, want))
    print("elbo_gain against 40 digits on %d variants: %.2e units" % (rows.size, far))
    assert far < 0.01
    mpmath.mp.dps = 15


def test_empty_cell_is_nan_throughout():
    ex = X.ambient_cell(np.zeros(0), np.zeros(0), np.zeros((0, 4)), np.full(4, 0.25), 2)
    assert all(np.all(np.isnan(np.asarray(v, dtype=np.float64))) for pair in ex.values() for v in pair)
    ex = X.ambient_cell(np.zeros(2), np.zeros(2), np.full((2, 4), 0.5), np.full(4, 0.25), 2)
    assert np.isnan(float(ex["llr"][0])) and ex["psi"][0].shape == (4,)


# ---------------------------------------------------------------- the cases are what they say
def test_em_cases_are_what_they_say():
    em = [sp for sp in XA.EM.values() if sp.kind == "em" and sp.edit is None and sp.name.startswith("K")]
    assert [sp.K for sp in em] == [1, 2, 3, 8, 16, 33, 63, 64, 65, 130]
    for sp in em:
        assert sp.targets == (1, 2, 63, 64, 65, 127, 128, 129) and sp.lengths == (2,)
    assert {sp.cap for sp in em} >= {None, 1, 64, 128}
    assert {sp.top for sp in em} == {40, 300, 5000}
    fmts = [sp.fmt for sp in XA.EM.values()]
    assert all(fmts.count(f) >= 2 for f in (0, 1, 2))
    for name, sp in XA.EM.items():
        p = XA.problem(name)
        assert p.M <= 300 and list(p.n_sel[:len(p.targets)]) == list(p.targets)
        top = int(p.dp.max())                         # 4-byte entries hold counts below 64, 8-byte ones below 65 536
        assert top < (64, 65536, 1 << 31)[sp.fmt], name
        XA.check_routes(p, XA.ORACLE)
        names = [r[0] for r in p.routes]
        assert names[:2] == ["default", "global"] and (sp.cap is None) == (not any(n.startswith("cap_") for n in names))
        assert ("all_cached" in names) == (XA.amb_lds_bytes(sp.K, int(p.n_sel.max())) <= XA.LDS_MAX)
    longs = [sp for sp in XA.EM.values() if sp.kind == "long"]
    assert [sp.K for sp in longs] == [3, 65, 130] and all(sp.lengths == (3, 4, 7) for sp in longs)
    assert "all_cached" not in [r[0] for r in XA.problem("long_K130").routes]
    p = XA.problem("deep_K5")
    assert p.dp.max() > 1000000 and (p.dp == 1).any()
    p = XA.problem("zero_psi")
    assert np.all(p.psi0[:, 1] == 0.0) and np.all(np.abs(p.psi0.sum(axis=1) - 1) < 1e-15)
    assert np.all(XA.problem("tiny_psi").psi0[:, 1] == 1e-300)
    p = XA.problem("near_one_psi")
    assert np.all(p.psi0[:, 0] == 1 - 1e-12) and np.all(np.abs(p.psi0[:, 1:].sum(axis=1) - 1e-12) < 1e-27)
    for name in ("edge_theta_K2", "edge_theta_K5"):
        p = XA.problem(name)
        assert set(np.unique(p.theta)) == {1e-9, 0.5, 1 - 1e-9}
    p = XA.problem("edge_theta_K2")                  # whole rows at either edge, met by counted cells
    t1 = np.concatenate([th @ p.psi0[c] for c, (_, _, th) in enumerate(p.cells) if p.counted[c]])
    assert t1.min() < 2e-9 and 1 - t1.max() < 2e-9
    p = XA.problem("same_theta")
    assert np.all(p.theta == p.theta[:, :1])
    p = XA.problem("alt_ref")
    kinds = [(np.all(b == 0), np.all(a == 0), ((a == 0) & (b > 0)).any()) for a, b, _ in p.cells[:len(p.targets)]]
    assert any(k[0] for k in kinds) and any(k[1] for k in kinds) and any(k[2] and not k[1] for k in kinds)
    p = XA.problem("one_entry_K130")
    assert p.K == 130 and list(p.n_sel[:3]) == [1, 1, 1]


@pytest.mark.parametrize("name", list(XA.EM))
def test_no_argmax_is_decided_by_rounding(name):
    """every counted cell's final psi: a relative gap of 1e-9 or more between its two largest components"""
    p = XA.problem(name)
    for n in p.spec.lengths + ((2, 4) if p.spec.kind == "long" else ()):
        psi = XA.ORACLE.run(p, p.psi0, n, None)[0]
        gap = min(XA.top_gap(psi[c]) for c in np.flatnonzero(p.counted))
        assert gap >= 1e-9, (name, n, gap)


def test_gain_cases_are_what_they_say():
    sps = list(XA.GAIN.values())
    assert {sp.K for sp in sps} == {1, 2, 3, 7, 16, 40, 70} and {sp.pc for sp in sps} == {1e-3, 0.5, 10.0}
    assert {sp.N for sp in sps} == {1, 255, 256, 257} and {sp.kind for sp in sps} == {"random", "zeros", "onehot"}
    for name in XA.GAIN:
        g = XA.gain_problem(name)
        assert np.unique(XA.gain_shapes(g)).size <= 5500, name
        assert g.lds == (("0", "1") if g.N > 1 else ("0",))
        if g.N > 1:
            depth, alt = np.asarray(g.DP.sum(1)).ravel(), np.asarray(g.AD.sum(1)).ravel()
            assert depth[0] == 0 and depth[1] == 1 and alt[2] == depth[2] > 0 and alt[3] == 0 < depth[3]
            assert sorted(g.DP[4].data) == [1, 5000017] and g.entries[5] == g.M
    g = XA.gain_problem("N256_K7_pc0.5_onehot")       # around digamma's switch from the recurrence to the series
    assert {9.5, 10.0, 10.5} <= set(XA.gain_shapes(g))
    g = XA.gain_problem("N257_K16_pc0.001_onehot")    # a donor without reads: ten steps of the recurrence
    assert (XA.gain_shapes(g) == 1e-3).any()
    g = XA.gain_problem("N255_K70_pc10_onehot")       # no recurrence anywhere
    assert XA.gain_shapes(g).min() >= 10.0


# ---------------------------------------------------------------- the library's cap
@pytest.mark.parametrize("budget", [None, 0, 1, 3359, 3360, 3361, 4408, 16384, 65536, 1 << 30])
def test_amb_cap_agrees_with_the_library(monkeypatch, budget):
    """``vrx_ambient_info`` evaluates what ``vrx_problem_ambient`` launches with; it needs no device"""
    if budget is None:
        monkeypatch.delenv("VIREO_AMBIENT_LDS", raising=False)
    else:
        monkeypatch.setenv("VIREO_AMBIENT_LDS", str(budget))
    for K in (1, 2, 3, 8, 16, 33, 63, 64, 65, 130):
        cap, lds = XA.library_plan(K)
        assert cap == XA.route_cap(K, budget) and lds == XA.amb_lds_bytes(K, cap), (K, budget, cap, lds)
    from vireo_amd import _lib
    assert _lib.lib().vrx_ambient_info(0, None, None) != 0 and b"vrx_ambient_info" in _lib.lib().vrx_last_error()
