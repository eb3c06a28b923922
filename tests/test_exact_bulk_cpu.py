"""The bulk harness checked without a GPU: float64 NumPy stands in the device's place.

* On every output of every case of tests/exact_bulk.py the float64 restatement (tests/bulk_np.py) stays
  inside the a-priori bound of recursive summation -- the variants, donors and classes contracted plus 16
  units.  A degenerate unit or a restatement of something else would show here.
* The rule has teeth: a float64 copy of the device's schedule (tiles, slices, per-workgroup partials,
  64 lanes of a reduction) passes the rule as it stands and fails it when made wrong the way a kernel
  would be, on the case written for that defect.
* The exact side agrees with the reference's own first iteration (tests/golden/c1_bulk_maxiter8.npz).
* The tile arithmetic the cases rely on, for a device of 256 CUs.
"""
import numpy as np
import pytest

from tests import bulk_np as B
from tests import exact_bulk as XB
from tests import exact_np as X
from tests import gold

N_CU = 256


@pytest.mark.parametrize("name", list(XB.CASES))
def test_float64_within_a_priori_bound(name):
    rows = []
    d = XB.run(name, N_CU, XB.ORACLE, rows, {})
    limit = XB.a_priori(d)
    worst = max(rows, key=lambda r: r[4])
    print("%s: limit %d, worst %.2f (%s %s)" % (name, limit, worst[4], worst[1], worst[2]))
    assert rows
    for r in rows:
        assert r[4] <= limit, r


# ---------------------------------------------------------------- the tile arithmetic
def test_tiles_of_256_cus():
    """bulk_tile and the grid of vrx_bulk_create, worked by hand from the LDS layouts of csrc/vrx_bulk.h"""
    # (4, 3): 768 fixed doubles, 20 per variant of the fit pass -> (40960 - 6144) / 160 = 217 -> 216
    assert XB.long_input(4, 3, "fit", N_CU) == (216, 1024)
    assert XB.long_input(4, 3, "ll", N_CU) == (256, 1024)
    # a chunk's four sets of accumulators: 3069 fixed doubles, T = 256 -> 65 512 bytes, two workgroups per CU
    assert XB.long_input(4, 3, "co", N_CU) == (256, 512) and XB.lds_bytes(4, 3, 256, "co")[0] == 65512
    # (150, 3): 1508 fixed, 604 per variant -> 5 -> 4; 31 392 bytes a workgroup, four per CU
    assert XB.long_input(150, 3, "fit", N_CU) == (4, 1024) and XB.lds_bytes(150, 3, 4, "fit")[0] == 31392
    assert XB.long_input(150, 3, "ll", N_CU) == (8, 1024)
    assert XB.long_input(150, 3, "co", N_CU) == (2, 512) and XB.long_input(150, 3, "co_ll", N_CU) == (6, 512)
    # the donor limit: nothing left for a tile, the minimum of 2, 65 504 of 65 536 bytes
    assert XB.long_input(454, 3, "fit", N_CU) == (2, 512) and XB.lds_bytes(454, 3, 2, "fit")[0] == 65504
    assert XB.lds_bytes(455, 3, 2, "fit")[0] > XB.LDS_MAX
    assert [XB.n_slice(K, 3) for K in (28, 29, 42, 43, 85, 86)] == [3, 2, 2, 1, 1, 1]
    assert [XB.n_slice(*kg) for kg in ((64, 4), (128, 2), (129, 2), (150, 3))] == [1, 1, 1, 1]
    assert XB.plan(1, 1, 2, N_CU) == dict(T=2, n_wg=1, T_ll=2, n_wg_ll=1, T_co=2, n_wg_co=1, T_co_ll=2, n_wg_co_ll=1)
    assert XB.plan(8195, 150, 3, N_CU)["n_wg"] == 1024 and -(-8195 // 4) == 2 * 1024 + 1


def test_cases_are_what_they_say():
    names = list(XB.CASES)
    fit = [XB.CASES[n] for n in names if XB.CASES[n].kind == "fit"]
    assert {(sp.K + sp.G) & 1 for sp in fit} == {0, 1}                   # the pad in front of (w1, w0)
    assert {sp.G == 3 for sp in fit} == {True, False}                    # both instances
    for name in names:                                                   # small ones: build them all
        sp = XB.CASES[name]
        if sp.K * sp.G <= 64 and "W" not in sp.n:
            d = XB.build(name, N_CU)
            if sp.kind == "fit" and name.startswith("load"):
                assert d.n_wg == d.tiles < 1024
    last = {}
    for name in names:                                                   # nv % n_slice of the last tile
        if name.startswith("slice_"):
            sp = XB.CASES[name]
            T = XB.long_input(sp.K, sp.G, "fit", N_CU)[0]
            nv = eval(sp.n, {"T": T}) - T
            last.setdefault((sp.K, sp.G), set()).add(nv % XB.n_slice(sp.K, sp.G))
    for (K, G), seen in last.items():
        ns = XB.n_slice(K, G)
        assert seen == {0, 1 % ns, ns - 1}, (K, G, seen)
    d = XB.build("load_K3_G3_N=T+1", N_CU)                               # L odd, a last tile of 1: nv L = 9
    assert (d.K * d.G) & 1 and d.N - d.T == 1
    d = XB.build("value_edge_theta_K5", N_CU)
    t1 = np.tensordot(d.GT, d.theta0, axes=(2, 0)) @ d.psi0
    assert t1.min() < 2e-9 and 1 - t1.max() < 2e-9 and 0 < t1.min() and t1.max() < 1
    d = XB.build("value_deep_K5", N_CU)
    assert d.DP.max() > 1e6 and (d.DP == 1).any()
    d = XB.build("value_counts_K5", N_CU)
    assert (d.DP == 0).any() and ((d.AD == d.DP) & (d.DP > 0)).any() and ((d.AD == 0) & (d.DP > 0)).any()
    d = XB.build("value_onehot_gt_K5", N_CU)
    assert set(np.unique(d.GT)) == {0.0, 1.0}
    assert (XB.build("value_tiny_gt_K5", N_CU).GT == 1e-300).any()
    d = XB.build("cohort_K3_G3_N=2*T+1_S3", N_CU)
    assert d.AD.shape == (3, 2 * 256 + 1) and d.DP[1].min() > 9e5 and d.DP[2].max() == 1


# ---------------------------------------------------------------- the rule has teeth
def _pass(AD, BD, GT, psi, theta, T, n_wg, wrong=None):
    """one pass in float64 on the device's schedule -> psi_raw[K], s1[G], s2[G], logLik of (psi, theta).
    ``wrong`` names one defect:
      odd_tail     the last entry of a tile of odd nv L taken from its neighbour
      straddle     the second half of a pair that straddles two rows lands beside the row's first
                   entry, which keeps what the LDS held (zero here)
      last_slice   the last round of a tile with nv % n_slice = 1 (slice 0 alone) left out of phase 2
      partial_64   partial 64 added twice (lane 0 of the reduction takes 0, 64, ...)
      skip_donor   the last donor left out of the fold of theta_s1"""
    N, K, G = GT.shape
    L, ns = K * G, XB.n_slice(K, G)
    sp, s1, s2, ll = np.zeros((n_wg, ns, K)), np.zeros((n_wg, ns, K, G)), np.zeros((n_wg, ns, K, G)), np.zeros(n_wg)
    with np.errstate(all="ignore"):
        for t in range(-(-N // T)):
            wg, n0 = t % n_wg, t * T
            nv = min(T, N - n0)
            P, a, b = GT[n0:n0 + nv].copy(), AD[n0:n0 + nv], BD[n0:n0 + nv]
            if wrong == "odd_tail" and (nv * L) & 1:
                P.reshape(-1)[-1] = P.reshape(-1)[-2]
            if wrong == "straddle" and L & 1:
                P[1::2, 0, 0] = 0.0
            tm = P @ theta
            t1, t0 = tm @ psi, (1 - tm) @ psi
            ll[wg] += np.sum(a * np.log(t1) + b * np.log(1 - t1))
            x1, x0 = (a / t1)[:, None] * (tm * psi), (b / t0)[:, None] * ((1 - tm) * psi)
            for s in range(ns):
                v = np.arange(s, nv, ns)
                if wrong == "last_slice" and s == 0 and nv % ns == 1:
                    v = v[:-1]
                sp[wg, s] += (x1[v] + x0[v]).sum(0)
                s1[wg, s] += np.einsum("vk,vkg->kg", x1[v], P[v])
                s2[wg, s] += np.einsum("vk,vkg->kg", x0[v], P[v])
    kept = slice(0, K - 1 if wrong == "skip_donor" else K)
    part = np.concatenate([sp.sum(1), s1[:, :, kept].sum((1, 2)), s2.sum((1, 2)), ll[:, None]], axis=1)
    lanes = [part[lane::64].sum(0) for lane in range(min(64, n_wg))]
    if wrong == "partial_64" and n_wg > 64:
        lanes[0] = lanes[0] + part[64]
    tot = np.sum(lanes, axis=0)
    return tot[:K], tot[K:K + G], tot[K + G:K + 2 * G], tot[-1]


class CopySide(XB.Float64Side):
    """a fit of one iteration as the device runs it: pass, update, pass"""

    def __init__(self, wrong=None, swap=None):
        self.wrong, self.swap = wrong, swap

    def _one(self, d, AD, BD, psi, theta):
        raw, s1, s2, _ = _pass(AD, BD, d.GT, psi, theta, d.T, d.n_wg, self.wrong)
        psi, theta = raw / raw.sum(), s1 / (s1 + s2)
        return psi, theta, np.array([_pass(AD, BD, d.GT, psi, theta, d.T, d.n_wg, self.wrong)[3]])

    def fit(self, d, psi, theta, max_iter=1, learn_theta=True):
        assert max_iter == 1 and learn_theta
        return self._one(d, d.AD, d.BD, psi, theta)

    def fit_cohort(self, d, idx, psi, theta, max_iter=1, learn_theta=True):
        AD, BD = d.AD.copy(), d.BD.copy()
        if self.swap is not None:              # one variant's counts taken from the next sample
            s, n = self.swap
            AD[s, n], BD[s, n] = d.AD[s + 1, n], d.BD[s + 1, n]
        out = [self._one(d, AD[s], BD[s], psi[i], theta[i]) for i, s in enumerate(idx)]
        return tuple(np.stack([o[j] for o in out]) for j in range(3))


def _fit_units(d, side):
    start = (d.psi0, d.theta0)
    return XB.update_distances(d.AD, d.BD, d.GT, start, side.fit(d, *start))


TEETH = [("teeth_odd_tail", "odd_tail", ("psi", "theta")),
         ("teeth_straddle", "straddle", ("psi", "theta")),
         ("teeth_last_slice", "last_slice", ("psi", "theta")),
         ("reduce_65", "partial_64", ("psi", "theta")),
         ("value_small_psi_K5", "skip_donor", ("theta",)),
         ("value_small_psi_K100", "skip_donor", ("theta",))]


@pytest.mark.parametrize("name,wrong,outputs", TEETH)
def test_a_defect_fails_the_rule(name, wrong, outputs):
    d = XB.build(name, N_CU)
    u_orc = _fit_units(d, XB.ORACLE)
    u_copy = _fit_units(d, CopySide())
    u_bad = _fit_units(d, CopySide(wrong))
    for k in u_orc:
        print("%s %-7s float64 %.2f  schedule copy %.2f  %s %.3g" % (name, k, u_orc[k], u_copy[k], wrong, u_bad[k]))
        assert X.held(u_copy[k], u_orc[k]), k           # the copy as it stands is held
    for k in outputs:
        assert not X.held(u_bad[k], u_orc[k]), k


def test_the_defects_are_the_subtle_ones():
    """what each case puts where the defect bites"""
    d = XB.build("teeth_odd_tail", N_CU)
    assert (d.N * d.K * d.G) & 1 and d.tiles == 1 and 0 < d.GT[-1, -1, -1] <= 1e-13 < d.GT[-1, -1, -2] <= 2e-13
    d = XB.build("teeth_straddle", N_CU)
    assert (d.K * d.G) & 1 and np.all(d.GT[1::2, 0, 0] == 1e-12)
    d = XB.build("teeth_last_slice", N_CU)
    assert (d.N - d.T) % XB.n_slice(d.K, d.G) == 1 and d.DP[-1] == 1 and d.DP.sum() > 1000
    assert XB.build("reduce_65", N_CU).n_wg == 65
    for name in ("value_small_psi_K5", "value_small_psi_K100"):
        d = XB.build(name, N_CU)
        assert 0.9e-9 < d.psi0[-1] < 1.1e-9


def test_counts_of_the_next_sample_fail_the_rule():
    d = XB.build("cohort_K3_G3_N=2*T+1_S3", N_CU)
    idx = [0, 1, 2]
    n = int(np.argmax(d.AD[0] != d.AD[1]))
    good = CopySide().fit_cohort(d, idx, d.psi0, d.theta0)
    bad = CopySide(swap=(0, n)).fit_cohort(d, idx, d.psi0, d.theta0)
    orc = XB.ORACLE.fit_cohort(d, idx, d.psi0, d.theta0)
    for s in idx:
        args = (d.AD[s], d.BD[s], d.GT, (d.psi0[s], d.theta0[s]))
        u_orc, u_copy, u_bad = (XB.update_distances(*args, [x[s] for x in out]) for out in (orc, good, bad))
        print("sample %d" % s, u_orc, u_copy, u_bad)
        for k in u_orc:
            assert X.held(u_copy[k], u_orc[k])
            assert X.held(u_bad[k], u_orc[k]) == (s != 0), (s, k)


# ---------------------------------------------------------------- the exact side against the fixture
def test_exact_update_agrees_with_the_fixture():
    """c1_bulk_maxiter8 holds the reference's trace: its first entry is what one iteration from the
    fixture's start gives, and the exact update and log-likelihood are within the bound of it"""
    g = gold.load("c1_bulk_maxiter8")
    AD, DP, GT, _, _ = B.fixture_inputs(g)
    AD, DP = AD.astype(np.float64), DP.astype(np.float64)
    r = B.fit(AD, DP, GT, g["psi0"], g["theta0"], max_iter=1)
    assert r["logLik"] == g["logLik_all"][0]
    ex = X.bulk_update(AD, DP - AD, GT, g["psi0"], g["theta0"])
    limit = GT.shape[0] + GT.shape[1] + GT.shape[2] + 16
    u = {k: X.distance(r[k], *ex[k]) for k in ("psi", "theta")}
    u["logLik"] = X.distance(g["logLik_all"][0], *X.bulk_loglik(AD, DP - AD, GT, r["psi"], r["theta"]))
    print("c1_bulk_maxiter8, first iteration:", u, "limit", limit)
    assert max(u.values()) <= limit
    assert np.allclose(np.asarray(ex["psi"][0], dtype=np.float64), r["psi"], rtol=1e-13, atol=0)
