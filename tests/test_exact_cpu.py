"""The per-update harness checked without a GPU: the float64 oracle stands in the device's place.

* On every case of the sweep (tests/exact_cases.py) the oracle's distance from the extended-precision
  restatement (tests/exact_np.py), in error units, stays inside the a-priori bound of recursive
  summation -- the longest contracted row or column plus 16.  A unit that were degenerate (too small
  for honest float64 arithmetic) or a restatement that computed something else would show here.
* The checker has teeth: results corrupted the way a kernel would be wrong fail the rule the GPU
  test asserts (``exact_np.held``).
* The cases that name instances of the LDS pass cover all 24 and agree with the restated dispatch; on
  their data, four defects of a slab edge, a column block or a row piece, planted through the oracle,
  fail the rule.
* On the c1_onestep fixture (values of the real reference) the restatement agrees with the golden
  values within the same rule.
"""
import copy
from types import SimpleNamespace

import numpy as np
import pytest
from scipy.sparse import csc_matrix
from scipy.special import betaln, digamma

from oracle import vireo_oracle as O
from tests import exact_cases as EC
from tests import exact_np as X
from tests import gold


def _report(tag, name, us, limit):
    print("%s %-24s limit %6d  " % (tag, name, limit) + "  ".join("%s %.2f" % kv for kv in us.items()))


@pytest.mark.parametrize("name", list(EC.CASES_A))
def test_oracle_stays_within_a_priori_bound_per_update(name):
    p = EC.problem_a(name)
    us = EC.distances_a(p, EC.run_a(p, EC.OracleBackend(p)))
    _report("A", name, us, EC.a_priori(p))
    for k, u in us.items():
        assert u <= EC.a_priori(p), (name, k, u)


@pytest.mark.parametrize("name", list(EC.CASES_B))
def test_oracle_through_whole_iterations(name):
    """the fit loop's flow: every update of every iteration is judged from the float64 state the
    backend read back in front of it, so the same a-priori bound holds for every output"""
    p = EC.problem_b(name)
    for r in range(p.spec.restarts):
        us = EC.distances_b(p, EC.run_b(p, EC.OracleBackend(p), r), r)
        _report("B", "%s[%d]" % (name, r), us, EC.a_priori(p))
        for k, u in us.items():
            assert u <= EC.a_priori(p), (name, r, k, u)


def test_named_states_are_what_they_say():
    """the underflow cases reach exact zeros in both softmaxes, the one-hot and 1e-300 states hold them"""
    for name in ("underflow_id", "underflow_gt", "underflow_lds"):
        p = EC.problem_a(name)
        be = EC.OracleBackend(p)
        L, ID = be.id()
        assert np.ptp(L, axis=1).max() > 745 and (ID == 0).any() and (be.gt() == 0).any()
    s = EC.problem_a("one_hot_id").s0
    assert set(np.unique(s.ID)) == {0.0, 1.0} and np.all(s.ID.sum(1) == 1)
    s = EC.problem_a("tiny_gt").s0
    assert (s.GT == 1e-300).any() and np.allclose(s.GT.sum(2), 1, rtol=0, atol=4e-16)
    p = EC.problem_a("edge_shapes_a")
    s1 = (p.s0.mu * p.s0.sm)[0]
    assert np.allclose(s1[:7], EC.EDGE_SHAPES, rtol=4e-16, atol=0)
    assert s1[2] < 10 <= s1[3] < s1[4]


def test_units_and_rule():
    one = np.ones(3)
    assert X.distance(one + 2 * X.EPS, one, X.EPS * one) == pytest.approx(2.0)
    assert X.distance(np.array([0.0]), X.ld([1e-320]), X.ld([1e-335])) == 0.0     # both underflowed
    assert X.distance(np.array([1e-17]), X.ld([0.0]), X.ld([0.0])) == float("inf")
    assert X.distance(np.array([np.nan]), X.ld([1.0]), X.ld([1.0])) == float("inf")
    assert X.held(4.0, 0.3) and not X.held(4.1, 0.3) and X.held(39.9, 10.0) and not X.held(40.1, 10.0)


# ---------------------------------------------------------------- the checker has teeth
@pytest.fixture(scope="module")
def gather():
    p = EC.problem_a("gather")
    out = EC.run_a(p, EC.OracleBackend(p))
    return p, out, EC.distances_a(p, out)


def _fails(p, out, u_orc, key, value):
    u = EC.distances_a(p, dict(out, **{key: value}))[key]
    print("corrupted %-10s %.3g units against the oracle's %.2f" % (key, u, u_orc[key]))
    return not X.held(u, u_orc[key])


def test_a_dropped_smallest_entry_fails(gather):
    """(a) the entry with the smallest |term| of one row left out of logLik_ID / of the theta sums"""
    p, out, u_orc = gather
    s, k = p.s0, 0
    # logLik_ID[m, k]: the cell with the most entries; its terms per entry (vireo_model.py:190-196)
    m = int(np.argmax(np.diff(p.DP.indptr)))
    rows = p.DP.indices[p.DP.indptr[m]:p.DP.indptr[m + 1]]
    ad, dp = p.AD[rows, m].toarray().ravel(), p.DP[rows, m].toarray().ravel()
    s1, s2 = s.mu * s.sm, (1 - s.mu) * s.sm
    terms = np.sum(s.GT[rows, k, :] * (ad[:, None] * digamma(s1) + (dp - ad)[:, None] * digamma(s2)
                                       - dp[:, None] * digamma(s1 + s2)), axis=1)
    t = terms[np.argmin(np.where(terms != 0, np.abs(terms), np.inf))]
    L = out["logLik_ID"].copy()
    L[m, k] -= t
    assert _fails(p, out, u_orc, "logLik_ID", L)
    # theta: the variant with the most entries; s1[g] loses ad * ID[m, k] * GT[n, k, g] (vireo_model.py:176-179)
    csr = p.AD.tocsr()
    n = int(np.argmax(np.diff(csr.indptr)))
    cells, ad = csr.indices[csr.indptr[n]:csr.indptr[n + 1]], csr.data[csr.indptr[n]:csr.indptr[n + 1]]
    terms = ad * s.ID[cells, k] * s.GT[n, k, 0]
    t = terms[np.argmin(np.where(terms != 0, terms, np.inf))]
    s1, s2 = out["beta_mu"] * out["beta_sum"], (1 - out["beta_mu"]) * out["beta_sum"]
    s1[0, 0] -= t
    assert _fails(p, out, u_orc, "beta_mu", s1 / (s1 + s2))
    assert _fails(p, out, u_orc, "beta_sum", s1 + s2)


def series_digamma(x, switch):
    """digamma for x > 0 the classic way: psi(x) = psi(x + 1) - 1 / x up to x >= switch, then
    ln x - 1 / (2x) - sum_k B_2k / (2k x^2k) with seven terms"""
    x = np.array(x, dtype=np.float64)
    w = np.zeros_like(x)
    while np.any(x < switch):
        low = x < switch
        w[low] += 1.0 / x[low]
        x[low] += 1.0
    z = 1.0 / (x * x)
    y = np.zeros_like(x)
    for c in (1 / 12, -691 / 32760, 1 / 132, -1 / 240, 1 / 252, -1 / 120, 1 / 12):   # B_14/14 .. B_2/2
        y = y * z + c
    return np.log(x) - 0.5 / x - y * z - w


def test_b_digamma_recurrence_stopped_early_fails(monkeypatch):
    """(b) the recurrence stopped at x >= 6 instead of 10: the series' truncation shows (1.6e-13 on
    a shape in [6, 7)); the same scheme with the switch at 10 is held"""
    p = EC.problem_a("shape_in_6_7")
    be = EC.OracleBackend(p)
    ex = EC.exact_a(p)

    def units():
        L, ID = be.id()
        return np.array([X.distance(L, *ex["logLik_ID"]), X.distance(be.gt(), *ex["GT_prob"]),
                         X.distance(ID, *ex["ID_prob"])])

    u_orc = units()
    us = {}
    for switch in (10.0, 6.0):
        monkeypatch.setattr(O, "digamma", lambda x, s=switch: series_digamma(x, s))
        us[switch] = units()
    print("logLik_ID / GT_prob / ID_prob: oracle %s, switch at 10 %s, at 6 %s" % (u_orc, us[10.0], us[6.0]))
    assert all(X.held(u, o) for u, o in zip(us[10.0], u_orc))
    # the logits and the genotype posterior show it; the cells' softmax, whose unit is twice the
    # largest logit's of the row, need not
    assert not X.held(us[6.0][0], u_orc[0]) and not X.held(us[6.0][1], u_orc[1])


def test_c_digamma_of_the_neighbouring_class_fails():
    """(c) KL_theta with class t + 1's digamma for class t, the two shapes 1e-6 apart (relative)"""
    p = EC.problem_a("twin_classes")
    s, pri = p.s0, p.pri
    u_orc = EC.distances_a(p, EC.run_a(p, EC.OracleBackend(p)))["KL_theta"]
    s1, s2 = (s.mu * s.sm)[0], ((1 - s.mu) * s.sm)[0]
    q1, q2 = pri.th1[0], pri.th2[0]
    assert abs(s1[2] / s1[1] - 1 - 1e-6) < 1e-9

    def kl(d1):                                   # vireo_base.py:96-125
        d2, ds = digamma(s2), digamma(s1 + s2)
        cq = betaln(q1, q2) - (q1 - 1) * d1 - (q2 - 1) * d2 + (q1 + q2 - 2) * ds
        cp = betaln(s1, s2) - (s1 - 1) * d1 - (s2 - 1) * d2 + (s1 + s2 - 2) * ds
        return np.sum(cq - cp)

    ex = EC.exact_a(p)["KL_theta"]
    good, bad = digamma(s1), digamma(s1)
    bad[1] = bad[2]
    assert X.held(X.distance(kl(good), *ex), u_orc)
    u = X.distance(kl(bad), *ex)
    print("KL_theta with the neighbour's digamma: %.3g units against %.2f" % (u, u_orc))
    assert not X.held(u, u_orc)


def test_d_partial_added_twice_fails(gather):
    """(d) one partial added a second time, scaled by 1e-9"""
    p, out, u_orc = gather
    s = p.s0
    assert _fails(p, out, u_orc, "LB_p", out["LB_p"] + 1e-9 * np.sum(p.L_given[:64] * s.ID[:64]))
    gt_block = np.sum(s.GT[:43] * (np.log(s.GT[:43]) + np.log(p.T)))      # 43 variants x K = 258 rows
    assert _fails(p, out, u_orc, "KL_GT", out["KL_GT"] + 1e-9 * gt_block)
    mu, sm = out["beta_mu"], out["beta_sum"]
    A = (p.AD @ s.ID)[:256]
    s1, s2 = mu * sm, (1 - mu) * sm
    s1 = s1 + 1e-9 * np.sum(A[:, :, None] * s.GT[:256], axis=(0, 1))
    assert _fails(p, out, u_orc, "beta_mu", s1 / (s1 + s2))
    assert _fails(p, out, u_orc, "beta_sum", s1 + s2)


# ---------------------------------------------------------------- the instance cases
def _named(table):
    return {n: c for n, c in table.items() if "inst_cell" in c.want or "inst_variant" in c.want}


def test_every_instance_of_the_lds_pass_is_named_by_a_case():
    """the 24 instances of vrx_spmm_lds -- pair words: PADK {0, 1} x SPLIT {1, 2, 4} of the variant pass
    (32 rows per wave) and of the cell pass at 64 and at 32 rows; AD/BD words: PADK {0, 1, 2} at 96 and
    32 rows -- each in the ``inst_*`` of some case, and what a case names is what the restated dispatch
    gives for its shape (at the 256 CUs the tile heights were worked out for)"""
    every = {(m, rw, pk, sp, 0) for m, rw in ((0, 32), (1, 64), (1, 32)) for pk in (0, 1) for sp in (1, 2, 4)}
    every |= {(1, rw, pk, 1, 1) for rw in (96, 32) for pk in (0, 1, 2)}
    assert len(every) == 24
    named = set()
    for table in (EC.CASES_A, EC.CASES_B):
        for name, c in _named(table).items():
            N, M = EC.data(c.data)[0].shape
            rule = EC.expected_launches(N, M, c.K * c.restarts, c.want.get("cell_form", 1),
                                        c.want.get("var_form", 3), 256)
            for o, launches in zip(("variant", "cell"), rule):
                if "inst_" + o in c.want:
                    assert {l[:5] for l in launches} == c.want["inst_" + o], (name, o, launches)
                    named |= c.want["inst_" + o]
    assert named == every, named ^ every


def test_slab_edge_data_sits_on_the_edges():
    """the instance cases' data has an entry in the last row of both orientations; the slab-edge sets hold
    exactly one there, one row beyond / short of a nominal slab, and their slabs -- nominal and as
    shortened for the CUs -- end where the cases say: a last slab of 1 and of 63 / 511 / 1023 rows"""
    for name in ("pair_short", "pair_tall", "shallow_tall", "clone", "many"):
        dp = EC.data(name)[1]
        assert dp[-1, :].nnz > 0 and dp[:, -1].nnz > 0, name
    for tag, (N, M) in EC.SLAB_EDGES.items():
        dp = EC.data("slab_edge_" + tag)[1]
        assert dp.shape == (N, M) and dp[-1, :].nnz == 1 and dp[:, -1].nnz == 1 and dp[-1, -1] > 0
    geo = EC.expected_slabs
    assert geo(513, 200, 1, 3, 256, False) == ((512, 1), (512, 2)) and geo(513, 200, 1, 3, 256, True)[1] == (64, 9)
    assert geo(511, 200, 0, 0, 256, False) == ((1024, 1), (512, 1)) and geo(511, 200, 0, 0, 256, True)[1] == (64, 8)
    assert geo(200, 1025, 1, 3, 256, False)[0] == (512, 2) and geo(200, 1025, 1, 3, 256, True)[0] == (64, 9)
    assert geo(200, 1025, 0, 0, 256, False)[0] == (1024, 2) and geo(200, 1025, 0, 0, 256, True)[0] == (64, 17)
    assert geo(200, 1023, 1, 3, 256, False)[0] == (512, 1) and geo(200, 1023, 0, 0, 256, True)[0] == (64, 16)
    # (a problem of the flagship's size keeps its nominal slabs)
    assert geo(40000, 20000, 1, 3, 256, True) == ((512, 20), (512, 79))


# ---------------------------------------------------------------- planted defects on the instance cases
def _with_data(p, ad, dp):
    """the case with other counts in the backend's hands; the exact side (p.C) keeps the true ones"""
    q = copy.copy(p)
    q.AD, q.DP = csc_matrix(ad), csc_matrix(dp)
    return q


def _planted(name, change, keys):
    """the oracle run on counts a defective pass would in effect have summed, judged against the exact
    update of the true counts: every output in ``keys`` must miss the rule"""
    p = EC.problem_a(name)
    u_orc = EC.distances_a(p, EC.run_a(p, EC.OracleBackend(p)))
    ad, dp = p.AD.toarray(), p.DP.toarray()
    change(ad, dp)
    q = _with_data(p, ad, dp)
    u = EC.distances_a(p, EC.run_a(q, EC.OracleBackend(q)))
    for k in keys:
        print("%-28s %-10s %.3g units against the oracle's %.2f" % (name, k, u[k], u_orc[k]))
        assert not X.held(u[k], u_orc[k]), (name, k, u[k], u_orc[k])


# (the outputs that read the counts; flow A's ELBO parts take a given logLik_ID)
SUMS = ("beta_mu", "beta_sum", "GT_prob", "logLik_ID", "ID_prob", "re_logLik_ID")


@pytest.mark.parametrize("tag", list(EC.SLAB_EDGES))
def test_dropped_entry_of_the_last_slab_fails(tag):
    """the single entry of the last contracted row of the last slab (both passes contract it) dropped"""
    def drop(ad, dp):
        ad[-1, -1] = dp[-1, -1] = 0
    _planted("slab_edge_%s_fill0_K16" % tag, drop, SUMS)
    _planted("slab_edge_%s_fill1_pairs_K7" % tag, drop, SUMS)


@pytest.mark.parametrize("name", ["pair_tall_K17", "shallow_tall_K7", "slab_edge_v513_fill1_K7"])
def test_last_entry_of_the_last_output_row_counted_twice_fails(name):
    def twice(ad, dp):
        for a in (ad, dp):                       # last cell: its last variant; last variant: its last cell
            a[np.flatnonzero(dp[:, -1])[-1], -1] *= 2
        n = np.flatnonzero(dp[-1, :])[-1]
        if n != dp.shape[1] - 1 or np.flatnonzero(dp[:, -1])[-1] != dp.shape[0] - 1:
            ad[-1, n], dp[-1, n] = 2 * ad[-1, n], 2 * dp[-1, n]
    _planted(name, twice, SUMS)


@pytest.mark.parametrize("name", ["pair_short_K17", "pair_tall_K17", "shallow_tall_K17", "balanced_K17"])
def test_last_column_taken_from_the_first_fails(name):
    """column 16 of a K = 17 operand (the block of one column) read from column 0: the cell pass's
    logLik_ID column and the variant pass's sums over that donor"""
    p = EC.problem_a(name)
    out = EC.run_a(p, EC.OracleBackend(p))
    u_orc = EC.distances_a(p, out)
    L = out["logLik_ID"].copy()
    L[:, 16] = L[:, 0]
    assert _fails(p, out, u_orc, "logLik_ID", L)
    q = copy.copy(p)                              # the variant pass: ID_prob's column 16 from column 0
    q.states = [copy.copy(p.s0)]
    q.s0 = q.states[0]
    q.s0.ID = p.s0.ID.copy()
    q.s0.ID[:, 16] = q.s0.ID[:, 0]
    bad = EC.OracleBackend(q)
    mu, sm = bad.theta()
    assert _fails(p, out, u_orc, "beta_mu", mu) and _fails(p, out, u_orc, "beta_sum", sm)
    assert _fails(p, out, u_orc, "GT_prob", bad.gt())


def test_a_row_piece_left_out_fails():
    """balanced_split_K16: rows longer than half the mean are cut into P interleaved pieces (entry j of
    a row -> piece j % P, cap = max(64, mean / 2)); one piece of the longest cell and of the longest
    variant left out"""
    name = "balanced_split_K16"
    p = EC.problem_a(name)
    dp0 = p.DP.toarray()

    def pieces(lengths):
        cap = max(64, int(lengths.mean() * 0.5 + 0.5))
        return int(np.argmax(lengths)), -(-int(lengths.max()) // cap)

    def cell_piece(ad, dp):
        m, P = pieces((dp0 > 0).sum(0))
        assert P > 1
        rows = np.flatnonzero(dp0[:, m])[::P]
        ad[rows, m] = dp[rows, m] = 0
    _planted(name, cell_piece, ("logLik_ID", "ID_prob", "re_logLik_ID"))

    def variant_piece(ad, dp):
        n, P = pieces((dp0 > 0).sum(1))
        assert P > 1
        cols = np.flatnonzero(dp0[n, :])[::P]
        ad[n, cols] = dp[n, cols] = 0
    _planted(name, variant_piece, ("beta_mu", "beta_sum", "GT_prob"))


# ---------------------------------------------------------------- the dense kernels past their grid caps
CU_COUNTS = (256, 208, 304)      # (the fixed 256 / 257 / 513 partials need a cap 4 n_cu >= 513)


def _dense(table, names):
    return [(n, table[n]) for n in names]


def test_dense_grid_puts_every_case_on_its_route():
    """the sizes are expressions in the grid terms: for three CU counts ``dense_grid`` gives every dense
    case the sweeps / strides / trips it declares, and together they take every threshold of the dense
    kernels from both sides -- each grid-stride loop twice and three times, the second stage of the
    shared theta at one, two and three strides (fused and as a kernel), every KP of the cell softmax
    past its cap, the ELBO's second stage at one, two and three trips by kernel and at two and three
    in the ride block"""
    every = _dense(EC.CASES_A, EC.DENSE_A) + _dense(EC.CASES_B, EC.DENSE_B)
    assert len(every) == len(EC.DENSE_A) + len(EC.DENSE_B) >= 40
    for n_cu in CU_COUNTS:
        for name, c in every:
            assert c.route and EC.route_misses(c, n_cu) == [], (n_cu, name, EC.route_misses(c, n_cu))
            N, M, _ = EC.dense_shape(c, n_cu)
            assert min(N, M) <= 200, (name, N, M)            # (the other dimension stays tiny)
    seen = {}
    for name, c in every:
        N, M, _ = EC.dense_shape(c, 256)
        g = EC.dense_route(c, N, M, 256)
        flow = "A" if name in EC.DENSE_A else "B"
        rides = flow == "B" and c.iters >= 2
        odd = c.K % 16 != 0
        for k in ("theta_sweeps", "gt_sweeps", "final_strides"):
            if k in c.route:
                seen.setdefault(k, set()).add((c.route[k], odd))
        if "cell_sweeps" in c.route:
            seen.setdefault("cell_sweeps", set()).add((EC.softmax_cap_of(c), g.KP, c.route["cell_sweeps"]))
        if "fuse" in c.route:
            seen.setdefault("fuse", set()).add((flow, c.route["fuse"], g.nb_theta))
        if "elbo_trips" in c.route:
            seen.setdefault("elbo_trips", set()).add(("ride" if rides else "kernel", c.route["elbo_trips"]))
    assert {(2, False), (2, True), (3, True)} <= seen["theta_sweeps"]
    assert {(2, False), (2, True), (3, True)} <= seen["gt_sweeps"]
    assert {(1, True), (2, True), (3, True)} <= seen["final_strides"]
    assert {("B", True, 256), ("B", False, 257)} <= seen["fuse"]
    assert {(4, kp, s) for kp in (16, 32, 64) for s in (2, 3)} | {(4, 8, 2)} | {(1, kp, 2) for kp in (2, 4, 8)} \
        <= seen["cell_sweeps"]
    assert {("kernel", 1), ("kernel", 2), ("kernel", 3), ("ride", 2), ("ride", 3)} <= seen["elbo_trips"]


def _sweep_of(p, nb):
    """(sweep, block) of every (variant, donor) element of a grid-stride kernel of nb blocks"""
    i = np.arange(p.N * p.K).reshape(p.N, p.K)
    return i // (nb * EC.VRX_BLOCK), (i // EC.VRX_BLOCK) % nb


def _theta_np(p, A, B, GT):
    """update_theta_size (vireo_model.py:176-185) in float64 from S and GT_prob, element by element"""
    s1 = p.pri.th1 + np.sum(A[:, :, None] * GT, axis=(0, 1))
    s2 = p.pri.th2 + np.sum(B[:, :, None] * GT, axis=(0, 1))
    return s1 / (s1 + s2), s1 + s2


def _theta_judge(p, s, A, B, GT):
    """(units of a planted theta, units of the honest float64 one) for beta_mu and beta_sum"""
    ex = X.vireo_theta(p.C, s.ID, s.GT, p.pri.th1, p.pri.th2, s.sm)
    A0 = (p.AD @ s.ID)
    B0 = (p.DP @ s.ID) - A0
    out = []
    for got, honest in zip(_theta_np(p, A, B, GT), _theta_np(p, A0, B0, s.GT)):
        key = "beta_mu" if len(out) == 0 else "beta_sum"
        out.append((X.distance(got, *ex[key]), X.distance(honest, *ex[key])))
    return out


def _theta_defect_fails(name, p, s, change):
    A = p.AD @ s.ID
    B = (p.DP @ s.ID) - A
    GT = s.GT.copy()
    A, B, GT = change(A.copy(), B.copy(), GT)
    for (u, u_orc), key in zip(_theta_judge(p, s, A, B, GT), ("beta_mu", "beta_sum")):
        print("%-28s %-9s planted %.3g units against the oracle's %.2f" % (name, key, u, u_orc))
        assert not X.held(u, u_orc), (name, key, u, u_orc)


def _strided_theta(table, names):
    return [n for n in names if table[n].route.get("theta_sweeps", 1) >= 2 and table[n].kind == "vireo"
            and not table[n].ase]


@pytest.mark.parametrize("name", _strided_theta(EC.CASES_A, EC.DENSE_A))
def test_b_elements_past_the_first_sweep_dropped_fails(name):
    """(b) vrx_theta_partial stops after one sweep of its capped grid"""
    p = EC.problem_a(name)
    g = EC.dense_route(p.spec, p.N, p.M, EC.N_CU)
    sweep, _ = _sweep_of(p, g.nb_theta)
    assert sweep.max() + 1 == p.spec.route["theta_sweeps"]

    def drop(A, B, GT):
        GT[sweep >= 1] = 0.0
        return A, B, GT
    _theta_defect_fails(name, p, p.s0, drop)


@pytest.mark.parametrize("name", ["dense_parts257", "dense_parts513", "dense_theta_full_grid", "dense_theta2_K17"])
def test_c_theta_partials_past_255_dropped_fails(name):
    """(c) the second stage of the shared theta takes one partial per thread only"""
    p = EC.problem_a(name)
    g = EC.dense_route(p.spec, p.N, p.M, EC.N_CU)
    _, block = _sweep_of(p, g.nb_theta)
    assert block.max() + 1 == g.nb_theta > 256

    def drop(A, B, GT):
        GT[block >= 256] = 0.0
        return A, B, GT
    _theta_defect_fails(name, p, p.s0, drop)


def test_c_partials_inside_the_first_stride_all_count():
    """the control of (c): at 256 partials the same defect changes nothing"""
    p = EC.problem_a("dense_parts256")
    _, block = _sweep_of(p, EC.dense_route(p.spec, p.N, p.M, EC.N_CU).nb_theta)
    assert block.max() == 255


@pytest.mark.parametrize("name", ["dense_elbo_parts2049", "dense_elbo_parts4097"])
def test_c_elbo_partials_past_2047_dropped_fails(name):
    """(c) the ELBO's second stage stops after its first trip: the cells of the softmax blocks from 2 048 on
    are missing from LB_p and KL_ID"""
    p = EC.problem_a(name)
    g = EC.dense_route(p.spec, p.N, p.M, EC.N_CU)
    out = EC.run_a(p, EC.OracleBackend(p))
    u_orc = EC.distances_a(p, out)
    block = np.arange(p.M) * g.KP // EC.VRX_BLOCK
    assert g.cell_sweeps == 1 and block.max() + 1 == g.n_cell_part > 2048
    keep = block < 2048
    s = p.s0
    assert _fails(p, out, u_orc, "LB_p", np.sum((p.L_given * s.ID)[keep]))
    assert _fails(p, out, u_orc, "KL_ID", np.sum(s.ID[keep] * (np.log(s.ID[keep]) + np.log(p.K))))


def _cell_sweep(p, g):
    """(sweep, the first sweep's cell of the same lanes) of every cell in vrx_cell_softmax"""
    per = g.nb_cell * EC.VRX_BLOCK // g.KP
    cell = np.arange(p.M)
    return cell // per, cell % per


@pytest.mark.parametrize("name", [n for n in EC.DENSE_A if "cell_sweeps" in EC.CASES_A[n].route
                                  and EC.CASES_A[n].route["cell_sweeps"] >= 2])
def test_d_preload_of_the_first_sweep_reused_fails(name):
    """(d) a cell of a later sweep takes the logLik_ID its lanes preloaded for the first sweep's cell"""
    p = EC.problem_a(name)
    g = EC.dense_route(p.spec, p.N, p.M, EC.N_CU)
    sweep, first = _cell_sweep(p, g)
    assert sweep.max() + 1 == p.spec.route["cell_sweeps"]
    out = EC.run_a(p, EC.OracleBackend(p))
    u_orc = EC.distances_a(p, out)
    L = out["logLik_ID"].copy()
    late = sweep >= 1
    L[late, :min(p.K, g.KP)] = L[first[late], :min(p.K, g.KP)]
    prior = p.pri.ID_prior if p.pri.ID_prior is not None else np.ones((1, p.K))
    assert _fails(p, out, u_orc, "ID_prob", O.softmax_log(L + np.log(prior)))


def _stale_k(p, nb):
    """(a): the element a thread reads in sweep s when its k stays the first sweep's -- index i - s step_k"""
    sweep, _ = _sweep_of(p, nb)
    step_k = nb * EC.VRX_BLOCK % p.K
    i = np.arange(p.N * p.K).reshape(p.N, p.K)
    return sweep, i - sweep * step_k


def test_a_stale_k_in_later_sweeps_fails():
    """(a) elements of the later sweeps keep the k of the first (no step_k, no wrap), seen where k is read:
    the per-donor genotype prior of vrx_gt_update, and the batched index of vrx_theta_partial (R > 1:
    S and GT_prob of element i - s step_k).  A K that divides the stride cannot show it."""
    p = EC.problem_a("dense_gt2_prior_row")
    g = EC.dense_route(p.spec, p.N, p.M, EC.N_CU)
    sweep, j = _stale_k(p, g.nb_gt)
    assert sweep.max() == 1 and (j % p.K != np.arange(p.K)).any()
    be = EC.OracleBackend(p)
    good = be.gt()
    ex = X.vireo_gt(p.C, p.s0.ID, p.s0.mu, p.s0.sm, p.pri.GT_prior, p.T)["GT_prob"]
    q = copy.copy(p)
    q.pri = copy.copy(p.pri)
    step_k = g.nb_gt * EC.VRX_BLOCK % p.K
    assert step_k and np.array_equal(j[sweep == 1] % p.K, ((np.arange(p.N * p.K) - step_k) % p.K)[sweep.ravel() == 1])
    q.pri.GT_prior = np.roll(p.pri.GT_prior, step_k, axis=1)       # (one (1, K, T) slab: donor k reads k - step_k)
    stale = EC.OracleBackend(q).gt()
    bad = np.where((sweep >= 1)[:, :, None], stale, good)
    u, u_orc = X.distance(bad, *ex), X.distance(good, *ex)
    print("GT_prob with the stale donor's prior: %.3g units against %.2f" % (u, u_orc))
    assert not X.held(u, u_orc)
    assert EC.grid_terms(EC.N_CU).S2 % 16 == 0           # (K = 16: step_k = 0, nothing to see)
    for name in ("dense_fit_theta2_pairs_R2", "dense_fit_gt2_K7_R3"):
        p = EC.problem_b(name)
        g = EC.dense_route(p.spec, p.N, p.M, EC.N_CU)
        sweep, j = _stale_k(p, g.nb_theta)

        def stale_elements(A, B, GT):
            late = sweep >= 1
            A[late], B[late] = A.ravel()[j[late]], B.ravel()[j[late]]
            GT[late] = GT.reshape(-1, p.T)[j[late]]
            return A, B, GT
        _theta_defect_fails(name, p, p.states[1], stale_elements)


@pytest.mark.parametrize("name", ["dense_fit_theta2_pairs_R2", "dense_fit_gt2_K7_R3"])
def test_e_batch_column_read_from_restart_0_fails(name):
    """(e) in the strided sweeps restart rb reads column block 0: S and GT_prob of restart 0"""
    p = EC.problem_b(name)
    g = EC.dense_route(p.spec, p.N, p.M, EC.N_CU)
    sweep, _ = _sweep_of(p, g.nb_theta)
    s0 = p.states[0]
    A0 = p.AD @ s0.ID
    B0 = (p.DP @ s0.ID) - A0

    def from_restart_0(A, B, GT):
        late = sweep >= 1
        A[late], B[late], GT[late] = A0[late], B0[late], s0.GT[late]
        return A, B, GT
    _theta_defect_fails(name, p, p.states[p.spec.restarts - 1], from_restart_0)


def test_e_cell_rows_read_from_restart_0_fails():
    """(e) on the cell side: a later sweep of vrx_cell_softmax reads restart 0's logLik_ID columns"""
    name = "dense_fit_cell2_R3"
    p = EC.problem_b(name)
    g = EC.dense_route(p.spec, p.N, p.M, EC.N_CU)
    sweep, _ = _cell_sweep(p, g)
    be = EC.OracleBackend(p)
    L0, L2 = be.loglik(be._st(0)), be.loglik(be._st(2))
    ex = X.id_from_loglik(X.ld(L2), X.EPS * np.abs(X.ld(L2)), p.pri.ID_prior, p.K)["ID_prob"]
    bad = np.where((sweep >= 1)[:, None], L0, L2)
    u, u_orc = X.distance(O.softmax_log(bad - np.log(p.K)), *ex), X.distance(O.softmax_log(L2 - np.log(p.K)), *ex)
    print("%s ID_prob from restart 0's logLik_ID: %.3g units against %.2f" % (name, u, u_orc))
    assert not X.held(u, u_orc)


# ---------------------------------------------------------------- the restatement against the fixture
def test_exact_functions_agree_with_the_golden_onestep():
    """c1_onestep holds the real reference's values after each update; the extended-precision
    functions, fed the fixture's float64 states, land within the rule's distance of them"""
    g = gold.load("c1_onestep")
    AD, DP = gold.c1()
    C = X.Counts(AD, DP)
    T = g["s0_GT_prob"].shape[2]
    K = g["s0_ID_prob"].shape[1]
    grid = np.linspace(0.01, 0.99, T)[None, :]
    th1, th2 = grid * 50.0, (1 - grid) * 50.0

    def state(pre):
        return SimpleNamespace(ID=g[pre + "ID_prob"], GT=g[pre + "GT_prob"], mu=g[pre + "beta_mu"],
                               sm=g[pre + "beta_sum"])

    s0, s1, s2, s3 = (state(x) for x in ("s0_", "s1_", "s2_", "s3_"))
    ex = {}
    ex.update(X.vireo_theta(C, s0.ID, s0.GT, th1, th2, s0.sm))
    ex.update(X.vireo_gt(C, s1.ID, s1.mu, s1.sm, None, T))
    ex.update(X.vireo_loglik(C, s2.GT, s2.mu, s2.sm))
    ex.update(X.id_from_loglik(*ex["logLik_ID"], None, K))
    parts = X.vireo_elbo_parts(g["logLik_ID"], s3.ID, s3.GT, s3.mu, s3.sm, None, None, th1, th2)
    ex["ELBO"] = EC._elbo_of(parts)
    ex["ELBO_recompute"] = ex["ELBO"]
    golden = dict(beta_mu=g["s1_beta_mu"], beta_sum=g["s1_beta_sum"], GT_prob=g["s2_GT_prob"],
                  logLik_ID=g["logLik_ID"], ID_prob=g["s3_ID_prob"], ELBO=g["ELBO"],
                  ELBO_recompute=g["ELBO_recompute"])
    # the oracle on the same inputs (it reproduces the fixture bit for bit: tests/test_oracle_golden.py)
    st = O.vireo_new(C.shape[1], C.shape[0], K, beta_mu_init=s0.mu.copy(), beta_sum_init=s0.sm.copy(),
                     ID_prob_init=s0.ID, GT_prob_init=s0.GT)
    st.ID_prob, st.GT_prob = s0.ID.copy(), s0.GT.copy()
    O.vireo_theta_step(st, AD, DP)
    orc = dict(beta_mu=st.beta_mu, beta_sum=st.beta_sum)
    O.vireo_gt_step(st, AD, DP)
    orc["GT_prob"] = st.GT_prob
    orc["logLik_ID"] = O.vireo_id_step(st, AD, DP)
    orc["ID_prob"] = st.ID_prob
    orc["ELBO"] = O.vireo_elbo(st, orc["logLik_ID"])
    orc["ELBO_recompute"] = O.vireo_elbo(st, None, AD, DP)
    for k, v in golden.items():
        u_gold = X.distance(np.reshape(v, np.shape(ex[k][0])), *ex[k])
        u_orc = X.distance(np.reshape(orc[k], np.shape(ex[k][0])), *ex[k])
        print("c1_onestep %-15s golden %.2f oracle %.2f units" % (k, u_gold, u_orc))
        assert X.held(u_gold, u_orc), k
        # (oracle and fixture coincide to the bit, so the line above cannot fail by itself: the
        # restatement is also held to the rule's bound for an oracle two roundings out, which is
        # what summing c1's short rows in float64 costs)
        assert u_gold <= X.bound(2.0), k
