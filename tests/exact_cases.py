"""The per-update sweep shared by tests/test_exact_cpu.py (float64 oracle in the device's place) and
tests/test_gpu_update_exact.py (the device): cases, the two flows, and the judge.

A case names its data, model shape, flags, state, priors, the environment that selects a kernel
path and what ``DeviceModel.info()`` / ``DeviceCounts.build_info()`` must then report, and may name
the instances of ``vrx_spmm_lds`` its passes must launch (``DeviceModel.lds_launches()``; the dispatch
is restated here, and the oracle has no launches: the CPU twin skips that part).  Flow A runs
every update once from the case's state (theta, GT, ID with logLik_ID, ELBO from a given logLik_ID,
ELBO recomputed); flow B runs whole iterations (theta, GT, ID, ELBO in the reference's order,
vireo_model.py:257-264, bmm_model.py:183-188) and judges each of their updates from the float64
state the backend read back in front of it.  A *backend* computes the outputs in float64 -- the
oracle here, the device in the GPU test; ``distances`` expresses them in the error units of
tests/exact_np.py.
"""
import functools
from types import SimpleNamespace

import numpy as np
from scipy.sparse import csc_matrix
from scipy.stats import entropy

from oracle import vireo_oracle as O
from tests import exact_np as X

PARTS = ("LB_p", "KL_ID", "KL_GT", "KL_theta")
EDGE_SHAPES = (1e-3, 0.5, 9.9999999, 10.0, 10.0000001, 1e4, 1e8)   # digamma: recurrence, its switch, pure series


# ------------------------------------------------------------------------------------
# data
# ------------------------------------------------------------------------------------
def _draw(N, M, density, depth, seed, top=None):
    rng = np.random.default_rng(seed)
    dp = (rng.random((N, M)) < density) * (1 + rng.poisson(depth, (N, M)))
    if top:
        dp = np.minimum(dp, top)
    ad = rng.binomial(dp, rng.choice([0.03, 0.5, 0.96], (N, 1)))
    return ad, dp


def _small():
    ad, dp = _draw(300, 200, 0.08, 1.0, 1)
    for m in range(200):                      # every cell has an entry: the fused cell softmax needs it
        if not dp[:, m].any():
            dp[m, m], ad[m, m] = 2, 1
    return ad, dp


def _ragged():
    """empty variants and cells, one variant that covers every cell, one cell that covers every variant"""
    ad, dp = _draw(400, 300, 0.05, 1.0, 5)
    rng = np.random.default_rng(6)
    dp[7, :] = 1 + rng.poisson(2.0, 300)
    dp[:, 11] = 1 + rng.poisson(2.0, 400)
    dp[100:120, :] = 0
    dp[:, 200:230] = 0
    return rng.binomial(dp, 0.4), dp


def _one_beyond():
    """test_deep_counts_with_one_beyond_pair_words: deep counts, two of them beyond the pair words"""
    rng = np.random.default_rng(77)
    N, M = 1300, 700
    dp = (1 + rng.poisson(40.0, (N, M))) * (rng.random((N, M)) < 0.04)
    dp[1111, 5] = 2048
    dp[17, 600] = 5000
    return rng.binomial(dp, rng.choice([0.02, 0.5, 0.97], (N, 1))), dp


def _split():
    """test_fit_loop_and_stepwise_api_agree_on_split_rows: heavy-tailed rows, cut into pieces"""
    from vireo_amd import synth                    # (the generator only: host NumPy)
    return synth.as_scipy(synth.donor_workload(3000, 1500, 6, 0.04, seed=3, skew=(1.5, 1.0)))


def _clone():
    rng = np.random.default_rng(9)
    N, M = 60, 400
    dp = rng.poisson(30, (N, M)) * (rng.random((N, M)) < 0.6)
    af = rng.beta(0.3, 3, (N, 5))
    return rng.binomial(dp, af[:, rng.integers(0, 5, M)]), dp


def _size(N, M):
    def make():
        ad, dp = _draw(N, M, 0.3, 2.0, N + M)
        dp[0, 0] = max(dp[0, 0], 1)
        return np.minimum(ad, dp), dp
    return make


def _edged(ad, dp, depth=9):
    """the last variant and the last cell hold one entry, the same one: it is the only entry of the
    last contracted row of the last slab in both passes (and the last entry of the last output row),
    so a slab edge that loses or repeats it has this entry's whole weight"""
    dp[-1, :], dp[:, -1] = 0, 0
    dp[-1, -1] = depth
    ad = np.minimum(ad, dp)
    ad[-1, -1] = depth // 3
    return ad, dp


def _pair_tall():
    """deep counts on more than two cell-pass slabs (1100 variants > 2 x 512): the 64-row tile of the
    pair-word cell pass; 1100 cells = two such tiles"""
    rng = np.random.default_rng(21)
    N = M = 1100
    dp = np.minimum(1 + rng.poisson(20.0, (N, M)), 255) * (rng.random((N, M)) < 0.03)
    ad = rng.binomial(dp, rng.choice([0.03, 0.5, 0.96], (N, 1)))
    dp[-1, -1], ad[-1, -1] = 31, 12                  # (an entry in the last row of both orientations)
    return ad, dp


def _shallow_tall():
    """depth about 1 on three cell-pass slabs: AD/BD words at the 96-row cell tile; 1600 cells = one
    tile of 1536 rows and one of 64"""
    ad, dp = _draw(1100, 1600, 0.03, 0.3, 22)
    dp[-1, -1], ad[-1, -1] = 3, 1
    return ad, dp


def _slab_edge(N, M):
    def make():
        return _edged(*_draw(N, M, 0.1, 1.0, 7 * N + M))
    return make


# contracted lengths one beyond and one short of a slab: 512 variants in the cell pass, 1024 cells
# in the variant pass (512 pairs of cells under AD/BD virtual rows); about 200 output rows
SLAB_EDGES = {"v513": (513, 200), "v511": (511, 200), "c1025": (200, 1025), "c1023": (200, 1023)}

DATA = {
    "small": _small,
    "mid": lambda: _draw(600, 900, 0.05, 1.0, 2),
    "tiny": lambda: _draw(60, 40, 0.3, 20.0, 5),                # one contracted range: each side inside one slab of 64
    "many": lambda: O.synth_donor(2600, 2300, 6, 0.03, seed=3),  # several slabs per orientation
    "ragged": _ragged,
    "split": _split,
    "clone": _clone,
    "depth3": lambda: _draw(600, 900, 0.05, 1.0, 11, top=3),
    "depth255": lambda: _draw(600, 900, 0.05, 50.0, 12, top=255),
    "depth2047": lambda: _draw(600, 900, 0.05, 1000.0, 13, top=2047),
    "depth_beyond": lambda: _draw(600, 900, 0.05, 3000.0, 14),
    "one_beyond": _one_beyond,
    "deep": lambda: _draw(200, 150, 0.3, 50.0, 15),             # spreads beyond exp's range
    "count_free": lambda: _count_free(),
    "pair_tall": _pair_tall,
    "shallow_tall": _shallow_tall,
}
DATA["pair_short"] = DATA["depth255"]
for _tag, (_n, _m) in SLAB_EDGES.items():
    DATA["slab_edge_" + _tag] = _slab_edge(_n, _m)
for _n, _m in ((255, 1), (1, 63), (256, 64), (257, 65), (1025, 257)):
    DATA["size_%dx%d" % (_n, _m)] = _size(_n, _m)


def _count_free():
    ad, dp = _draw(120, 90, 0.2, 3.0, 16)
    dp[:28, :] = 0                                  # variants whose theta posterior is their prior
    return np.minimum(ad, dp), dp


@functools.lru_cache(maxsize=None)
def data(name):
    ad, dp = DATA[name]()
    return csc_matrix(ad), csc_matrix(dp)


# ------------------------------------------------------------------------------------
# states and priors
# ------------------------------------------------------------------------------------
def _theta_from_shapes(s, s1, s2):
    s1, s2 = np.asarray(s1, dtype=float), np.asarray(s2, dtype=float)
    s.sm = np.broadcast_to(s1 + s2, s.mu.shape).copy()
    s.mu = np.broadcast_to(s1 / (s1 + s2), s.mu.shape).copy()


def st_edge_a(s, p, rng):        # T = 8: s1 and s2 walk through the edge values
    v = np.array(EDGE_SHAPES + (6.5,))
    _theta_from_shapes(s, v, np.roll(v, 3))


def st_edge_b(s, p, rng):        # T = 8: s1 + s2 is (within a rounding) an edge value
    v = np.array(EDGE_SHAPES + (6.5,))
    _theta_from_shapes(s, 0.3 * v, v - 0.3 * v)


def st_twins(s, p, rng):         # classes 0 and 1 equal, class 2 1e-6 away
    _theta_from_shapes(s, [7.25, 7.25, 7.25 * (1 + 1e-6)], [41.5, 41.5, 41.5 * (1 + 1e-6)])


def st_in_6_7(s, p, rng):        # a shape where a recurrence that stops early shows
    _theta_from_shapes(s, [6.4, 25.0, 43.5], [43.6, 25.0, 6.5])


def st_one_hot_id(s, p, rng):
    s.ID[:] = 0.0
    s.ID[np.arange(p.M), rng.integers(0, p.K, p.M)] = 1.0


def st_tiny_gt(s, p, rng):
    s.GT[::3, :, 0] = 1e-300
    s.GT[::3, :, 1:] = O.unit_sum(s.GT[::3, :, 1:])


def st_sharp_gt(s, p, rng):      # confident genotypes on deep data: logLik_ID spreads beyond 745
    g = rng.integers(0, p.T, (p.N, p.K))
    s.GT[:] = 0.01 / (p.T - 1)
    np.put_along_axis(s.GT, g[:, :, None], 0.99, axis=2)
    s.GT = O.unit_sum(s.GT)


def st_random_theta(s, p, rng):
    s.mu = rng.uniform(0.02, 0.98, s.mu.shape)
    s.sm = rng.uniform(3.0, 200.0, s.mu.shape)


def pr_gt_row(p, rng):
    return dict(GT_prior=O.unit_sum(rng.random((1, p.K, p.T)) + 0.05))


def pr_gt_full(p, rng):
    return dict(GT_prior=O.unit_sum(rng.random((p.N, p.K, p.T)) + 0.05))


def pr_id_vector(p, rng):        # not normalised: the reference keeps it as given (vireo_model.py:118)
    return dict(ID_prior=(rng.random((1, p.K)) + 0.1) * 1.7)


def pr_id_cells(p, rng):
    return dict(ID_prior=O.unit_sum(rng.random((p.M, p.K)) + 0.05))


def pr_theta(p, rng):
    rows, cols = (1, p.T) if p.kind == "vireo" else (1, p.K)
    return dict(th1=rng.uniform(0.3, 40.0, (rows, cols)), th2=rng.uniform(0.3, 40.0, (rows, cols)))


def pr_theta_rows(p, rng):
    """per-variant theta priors (ASE mode) with the edge shapes on the count-free variants: the
    update leaves s1 = prior there"""
    th1 = rng.uniform(0.3, 40.0, (p.N, p.T))
    th2 = rng.uniform(0.3, 40.0, (p.N, p.T))
    v = np.array(EDGE_SHAPES)
    for i in range(4):           # 4 x 7 = 28 rows: every (s1, s2) offset of the edge list, class by class
        th1[7 * i:7 * i + 7, :] = v[:, None]
        th2[7 * i:7 * i + 7, :] = np.roll(v, i + 1)[:, None]
    th1[:7, 0], th2[:7, 0] = 0.3 * v, v - 0.3 * v       # s1 + s2 an edge value
    return dict(th1=th1, th2=th2)


def pr_bmm_clones(p, rng):       # differs per clone, one row: broadcast over variants (bmm_model.py:92-98)
    return dict(th1=rng.uniform(0.3, 5.0, (1, p.K)), th2=rng.uniform(0.3, 5.0, (1, p.K)))


# ------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------
CASES_A, CASES_B = {}, {}


def _case(table, name, data, K=4, T=3, kind="vireo", ase=False, fix=False, learn_gt=True, state=(),
          prior=(), env=None, balance=None, want=None, seed=0, restarts=1, iters=1, fused_softmax=None,
          route=None):
    """data: a name of DATA, or a function of the grid terms (``grid_terms``) that gives (N, M, maker) --
    the dense-grid cases, whose sizes follow the device's CU count; route: what ``dense_grid`` and the
    model's launch record must give for them"""
    assert name not in table
    table[name] = SimpleNamespace(name=name, data=data, K=K, T=T, kind=kind, ase=ase, fix=fix,
                                  learn_gt=learn_gt, state=tuple(state), prior=tuple(prior),
                                  env=dict(env or {}), balance=balance, want=dict(want or {}), seed=seed,
                                  restarts=restarts, iters=iters, fused_softmax=fused_softmax,
                                  route=dict(route or {}))


LDS0, LDS1 = {"VIREO_LDS": "0"}, {"VIREO_LDS": "1"}
ON = dict(lds_variant=True, lds_cell=True)
OFF = dict(lds_variant=False, lds_cell=False)
many = lambda v: v > 1                                                    # noqa: E731
some = lambda v: v > 0                                                    # noqa: E731


# ---- which instance of vrx_spmm_lds a launch takes ------------------------------------------
# The dispatch of vrx_engine.hip restated (lds_kernel, lds_kernel_rw, lds_kernel_form1, pick_rw_cell,
# tile_layout): what ``DeviceModel.lds_launches()`` must report for a problem shape, its stream forms
# and the total operand width Kt (restarts x K).  An instance is (MODE, RW, PADK, SPLIT, FORM).
RW_VARIANT, RW_CELL, RW_CELL_PAIR, RW_CELL_SHORT = 32, 96, 64, 32
SLAB_CELL, SLAB_VARIANT, LDS_WAVES = 512, 1024, 16
LAUNCH_KEYS = ("inst_variant", "inst_cell", "perm", "slab_fill")    # ``want`` keys held by the launch record


def _up(a, b):
    return -(-a // b)


def cell_rows_per_wave(n_var, n_cell, cell_form, n_cu):
    """pick_rw_cell: the short tile when the problem has at most two cell-pass slabs and the busiest
    CU's visits x rows per wave come out lower"""
    tall = RW_CELL if cell_form == 1 else RW_CELL_PAIR
    slabs = _up(n_var, SLAB_CELL)

    def cost(rw):
        return _up(_up(n_cell, LDS_WAVES * rw) * slabs, max(1, n_cu)) * rw
    return RW_CELL_SHORT if slabs <= 2 and cost(RW_CELL_SHORT) < cost(tall) else tall


def block_launches(mode, rw, form, Kt):
    """one (MODE, RW, PADK, SPLIT, FORM, kb, ld) per block of 16 columns.  Pair words (FORM 0): 4 / 2
    entries at once when kb <= 4 / 8, element-wise staging when kb % 4 or the rows are strided
    (Kt > 16).  AD/BD words (FORM 1): PADK 0 flat rows of 16 columns, 2 whole 16-B units (kb and ld
    even), 1 element-wise."""
    out = []
    for c0 in range(0, Kt, 16):
        kb, strided = min(16, Kt - c0), Kt > 16
        if form == 1:
            out.append((mode, rw, 0 if kb == 16 and not strided else 2 if (kb | Kt) % 2 == 0 else 1, 1, 1, kb, Kt))
        else:
            out.append((mode, rw, int(kb % 4 != 0 or strided), 4 if kb <= 4 else 2 if kb <= 8 else 1, 0, kb, Kt))
    return out


def expected_launches(n_var, n_cell, Kt, cell_form, var_form, n_cu):
    """(variant pass, cell pass).  The variant pass over AD/BD virtual rows (var_form 3) runs the cell
    pass's kernel (MODE 1, FORM 1) at its tall tile."""
    var = block_launches(1, RW_CELL, 1, Kt) if var_form == 3 else block_launches(0, RW_VARIANT, 0, Kt)
    return var, block_launches(1, cell_rows_per_wave(n_var, n_cell, cell_form, n_cu), cell_form, Kt)


def slab_geometry(n_rows, n_contract, rw, nominal, n_cu, fill):
    """(slab_rows, n_slab) of tile_layout for n_rows row pieces.  VIREO_LDS_FILL_CUS:
    with fewer (tile, slab) visits than CUs the slabs are shortened until every CU has one -- to a
    multiple of 16 rows, 64 at least; one or two slabs are first spread over whole rounds of CUs
    where that leaves four rows per wave."""
    slab, n_slab, n_tile = nominal, _up(n_contract, nominal), _up(n_rows, LDS_WAVES * rw)
    if fill and n_cu > 0:
        def spread(n_tile):
            nt = _up(n_tile * n_slab, n_cu) * n_cu // n_slab
            return nt if nt > n_tile and nt * LDS_WAVES * 16 <= max(n_rows, 1) * 4 else n_tile
        if n_slab <= 2:
            n_tile = spread(n_tile)
        if n_tile * n_slab < n_cu:
            slab = min(nominal, max(64, _up(_up(n_contract, _up(n_cu, n_tile)), 16) * 16))
            n_slab = _up(n_contract, slab)
    return slab, n_slab


def expected_slabs(n_var, n_cell, cell_form, var_form, n_cu, fill, extra=(0, 0)):
    """(variant pass, cell pass): (slab_rows, n_slab); extra: the row pieces beyond one per row
    (``info()``'s extra_pieces_*: the tiles are counted in pieces)"""
    var = (slab_geometry(2 * n_var + extra[0], (n_cell + 1) // 2, RW_CELL, SLAB_CELL, n_cu, fill) if var_form == 3
           else slab_geometry(n_var + extra[0], n_cell, RW_VARIANT, SLAB_VARIANT, n_cu, fill))
    rw = cell_rows_per_wave(n_var, n_cell, cell_form, n_cu)
    return var, slab_geometry(n_cell + extra[1], n_var, rw, SLAB_CELL, n_cu, fill)


# ---- the grids of the dense kernels -------------------------------------------------------------
# vrx_model_create, theta_step, gt_step, softmax_step and cell_pass_softmax of vrx_engine.hip restated:
# what ``DeviceModel.dense_launches()`` must report for a shape, and how many sweeps of a capped grid
# / trips of a second-stage loop that makes.  Each constant with the line it restates:
VRX_BLOCK = 256                   # vrx_kernels.h: constexpr int VRX_BLOCK = 256
VRX_WAVES = VRX_BLOCK // 64       # vrx_kernels.h: constexpr int VRX_WAVES = VRX_BLOCK / 64
XCDS = 8                          # vrx_engine.hip: static constexpr int kXcd = 8
THETA_BLOCKS_PER_CU = 4           # m->nb_theta = std::min(m->nb_nk, p->n_cu * 4)
GT_BLOCKS_PER_CU = 8              # m->nb_gt = std::min(m->nb_nk, p->n_cu * 8)
SOFTMAX_BLOCKS_PER_CU = 4         # env_int("VIREO_SOFTMAX_BLOCKS_PER_CU", 4); 0: no cap
FUSE_THETA_MAX_PARTS = 256        # env_int("VIREO_FUSE_THETA_MAX_PARTS", 256): nb_theta <= fuse_max fuses
THETA_FINAL_IN_FLIGHT = 4         # vrx_theta_final_block: b0 += 4 * VRX_BLOCK
ELBO_IN_FLIGHT = 8                # vrx_elbo_final_block: constexpr int UN = 8
BMM_LANES = 16                    # theta_step: (m->NK * 16 + VRX_BLOCK - 1) / VRX_BLOCK with the range sum fused
N_CU = 256                        # the CU count the sizes of the dense cases are evaluated for (``set_n_cu``)


def pick_kp(K):
    """pick_kp: lanes per cell of vrx_cell_softmax<KP>, the power of two >= K, 64 at most"""
    kp = 1
    while kp < K and kp < 64:
        kp <<= 1
    return kp


def dense_grid(N, M, K, R=1, kind="vireo", ase=False, n_cu=256, softmax_cap=SOFTMAX_BLOCKS_PER_CU,
               fused_cell_pass=False, n_seg=0, fused_range_sum=False):
    """The grids and partial counts of the dense kernels for a model of N variants, M cells, K donors
    (R restarts change none of them: the batch is the grid's y), and the loop trips they imply.
    fused_cell_pass: the cell partials come from the epilogue of the gather cell pass over n_seg
    segments; fused_range_sum (clone mode): vrx_bmm_theta sums the LDS pass's ranges, 16 lanes an element."""
    g = SimpleNamespace(n_cu=n_cu, KP=pick_kp(K))
    nb_nk = _up(N * K, VRX_BLOCK)
    g.nb_gt = min(nb_nk, n_cu * GT_BLOCKS_PER_CU)
    if kind != "vireo":
        g.nb_theta = _up(N * K * BMM_LANES, VRX_BLOCK) if fused_range_sum else nb_nk
    elif ase:
        g.nb_theta = _up(N, VRX_BLOCK)               # vrx_theta_ase: a thread per variant, no stride
    else:
        g.nb_theta = min(nb_nk, n_cu * THETA_BLOCKS_PER_CU)
    shared = kind == "vireo" and not ase
    g.fuse = shared and g.nb_theta <= FUSE_THETA_MAX_PARTS     # (in the fit loop; ``step`` never fuses)
    g.nb_cell = _up(M * g.KP, VRX_BLOCK)
    if softmax_cap > 0:
        g.nb_cell = min(g.nb_cell, n_cu * softmax_cap)
    g.n_cell_part = n_seg // VRX_WAVES if fused_cell_pass else g.nb_cell
    g.n_gt_part = g.nb_gt if kind == "vireo" else 0
    g.n_th_part = 1 if shared else g.nb_theta
    # sweeps of the grid-stride loops, strides of the shared theta's second stage, trips of the ELBO's
    g.theta_sweeps = _up(nb_nk, g.nb_theta) if shared else 1
    g.gt_sweeps = _up(nb_nk, g.nb_gt) if kind == "vireo" else 0
    g.cell_sweeps = _up(M, g.nb_cell * VRX_BLOCK // g.KP)
    g.final_strides = _up(g.nb_theta, VRX_BLOCK) if shared else 0          # (partials per thread)
    g.final_trips = _up(g.nb_theta, THETA_FINAL_IN_FLIGHT * VRX_BLOCK) if shared else 0   # (2 past 256 CUs only)
    g.elbo_trips = _up(max(g.n_cell_part, g.n_gt_part, g.n_th_part), ELBO_IN_FLIGHT * VRX_BLOCK)
    return g


def fused_cell_segments(M):
    """n_seg of build_orient for M cells of one short segment each on one tile: groups of VRX_WAVES
    segments go round the XCDs, every XCD is padded to the longest, whole blocks"""
    return _up(_up(M, VRX_WAVES), XCDS) * XCDS * VRX_WAVES


def grid_terms(n_cu, softmax_cap=SOFTMAX_BLOCKS_PER_CU):
    """what the dense cases write their sizes in: S1 / S2 elements fill the capped grid of
    vrx_theta_partial / vrx_gt_update once, C lanes that of vrx_cell_softmax, B one block; rows(n, K) is
    the fewest rows of K columns that hold n elements"""
    return SimpleNamespace(n_cu=n_cu, B=VRX_BLOCK, S1=THETA_BLOCKS_PER_CU * n_cu * VRX_BLOCK,
                           S2=GT_BLOCKS_PER_CU * n_cu * VRX_BLOCK, C=softmax_cap * n_cu * VRX_BLOCK,
                           rows=_up)


def set_n_cu(n_cu):
    """the device's CU count, for the sizes of the dense cases (the CPU twin keeps 256)"""
    global N_CU
    N_CU = int(n_cu)


def softmax_cap_of(spec):
    return int(spec.env.get("VIREO_SOFTMAX_BLOCKS_PER_CU", SOFTMAX_BLOCKS_PER_CU))


def dense_shape(spec, n_cu):
    """(N, M, maker) of a dense case for a CU count"""
    return spec.data(grid_terms(n_cu, softmax_cap_of(spec)))


def dense_route(spec, N, M, n_cu):
    """``dense_grid`` of a case: flow B's cell partials come from the fused cell pass where the case
    says so (fused_softmax), clone mode on the LDS path fuses its range sum in the fit loop"""
    fused = bool(spec.fused_softmax)
    return dense_grid(N, M, spec.K, spec.restarts, spec.kind, spec.ase, n_cu, softmax_cap_of(spec),
                      fused_cell_pass=fused, n_seg=fused_cell_segments(M) if fused else 0,
                      fused_range_sum=bool(spec.route.get("fused_range_sum")))


ROUTE_KEYS = ("theta_sweeps", "gt_sweeps", "cell_sweeps", "final_strides", "elbo_trips", "fuse", "n_cell_part",
              "n_th_part")


def route_misses(spec, n_cu):
    """[(key, declared, restated)] where ``dense_grid`` does not put the case on the route it declares"""
    N, M, _ = dense_shape(spec, n_cu)
    g = dense_route(spec, N, M, n_cu)
    return [(k, v, getattr(g, k)) for k, v in spec.route.items() if k in ROUTE_KEYS and getattr(g, k) != v]


def _thin(cells_full=False, density=0.15, depth=3.0, full_rows=(), full_cols=()):
    """the dense cases' counts: the other dimension is tiny, so the sparse passes stay trivial;
    full_rows / full_cols: variants / cells with an entry everywhere (long rows are cut into pieces)"""
    def make(N, M):
        ad, dp = _draw(N, M, density, depth, 3 * N + M)
        dp[-1, -1] = max(dp[-1, -1], 2)              # (an entry in the last row of both orientations)
        for n in full_rows:
            dp[n, :] = np.maximum(dp[n, :], 1)
        for m in full_cols:
            dp[:, m] = np.maximum(dp[:, m], 1)
        if cells_full:                                # every cell has an entry: the fused cell softmax needs it
            for m in np.flatnonzero(dp.sum(0) == 0):
                dp[m % N, m] = 2
        return np.minimum(ad, dp), dp
    return make


def _a(*a, **k):
    _case(CASES_A, *a, **k)


def _b(*a, **k):
    _case(CASES_B, *a, **k)


# paths: gather kernels / LDS-resident passes, work-list sizes, one and many contracted ranges
_a("gather", "mid", K=6, env=LDS0, want=OFF)
_a("lds", "mid", K=6, env=LDS1, want=dict(ON, cell_form=1, var_form=3, inst_variant={(1, 96, 2, 1, 1)},
                                           inst_cell={(1, 32, 2, 1, 1)}))     # (AD/BD words, the short cell tile)
for blocks in (1, 16, 1024):
    _a("blocks%d_one" % blocks, "tiny", K=8, env=dict(LDS1, VIREO_LDS_BLOCKS=str(blocks)),
       want=dict(ON, ranges_variant=1, ranges_cell=1))
    _a("blocks%d_many" % blocks, "many", K=6, env=dict(LDS1, VIREO_LDS_BLOCKS=str(blocks)),
       want=dict(ON, ranges_variant=1, ranges_cell=1) if blocks == 1 else
       dict(ON, ranges_variant=many, ranges_cell=many))
for fmt in (0, 1, 2):
    for lds, tag in ((LDS0, "gather"), (LDS1, "lds")):
        _a("fmt%d_%s" % (fmt, tag), "mid", K=5, env=dict(lds, VIREO_ENTRY_FMT=str(fmt)),
           want=dict(ON if lds is LDS1 else OFF, fmt_variant=fmt, fmt_cell=fmt))
for cf, vf in ((0, 0), (1, 3), (0, 3), (1, 0)):
    _a("form_c%d_v%d" % (cf, vf), "depth255", K=5,
       env=dict(LDS1, VIREO_CELL_FORM=str(cf), VIREO_VAR_FORM=str(vf)), want=dict(ON, cell_form=cf, var_form=vf))
# count depths that choose each form by themselves
_a("depth3", "depth3", K=5, env=LDS1, want=dict(ON, cell_form=1, var_form=3))
_a("depth255", "depth255", K=5, env=LDS1, want=dict(ON, cell_form=0, var_form=0))
_a("depth2047", "depth2047", K=5, env=LDS1, want=dict(ON, cell_form=0, var_form=0))
_a("depth_beyond", "depth_beyond", K=5, env=LDS1, want=dict(ON, cell_form=1, var_form=3))
_a("one_beyond", "one_beyond", K=6, env=LDS1, want=dict(ON, cell_form=1, var_form=3))
_a("balanced", "many", K=6, balance=True,
   env=dict(LDS1, VIREO_BUILD="device", VIREO_LDS_SPLIT_X10="60"),
   want=dict(ON, balanced_variant=True, balanced_cell=True, device_built=True))
_a("build_host", "mid", K=6, env=dict(LDS1, VIREO_BUILD="host"), want=dict(ON, device_built=False))
_a("build_device", "mid", K=6, env=dict(LDS1, VIREO_BUILD="device"), want=dict(ON, device_built=True))
# K: padded K % 4, 2 / 4 entries at once, every vrx_cell_softmax<KP>, the K > KP loop
for K in (1, 2, 3, 4, 5, 8, 9, 16, 17, 33, 64, 70):
    _a("K%d_gather" % K, "small", K=K, env=LDS0, want=OFF)
    if K >= 2:                                   # (one column stays on the gather kernels)
        _a("K%d_lds" % K, "small", K=K, env=LDS1,  # (AD/BD words at the short cell tile: flat rows, element-wise)
           want=dict(ON, **({16: dict(inst_cell={(1, 32, 0, 1, 1)}), 5: dict(inst_cell={(1, 32, 1, 1, 1)})}.get(K, {}))))
for T in (2, 3, 4, 8):
    _a("T%d_gather" % T, "small", K=4, T=T, env=LDS0, want=OFF)
    _a("T%d_lds" % T, "small", K=5, T=T, env=LDS1, want=ON)
# sizes around the wave and the block; empty rows and columns; rows that cover everything
for n, m in ((255, 1), (1, 63), (256, 64), (257, 65), (1025, 257)):
    _a("size_%dx%d_gather" % (n, m), "size_%dx%d" % (n, m), K=3, env=LDS0, want=OFF)
    if min(n, m) >= 63:
        _a("size_%dx%d_lds" % (n, m), "size_%dx%d" % (n, m), K=3, env=LDS1, want=ON)
_a("ragged_gather", "ragged", K=7, env=LDS0, want=OFF)
_a("ragged_lds", "ragged", K=7, env=LDS1, want=ON)
_a("split_rows", "split", K=6, env=LDS1, want=dict(ON, extra_pieces_cell=some, extra_pieces_variant=some))
# modes
_a("ase", "small", K=4, ase=True, state=[st_random_theta], env=LDS0, want=OFF)
_a("ase_lds", "small", K=4, ase=True, state=[st_random_theta], env=LDS1, want=ON)
_a("fix_beta_sum", "small", K=4, fix=True, env=LDS0, want=OFF)
_a("ase_fix_beta_sum", "small", K=4, ase=True, fix=True, env=LDS0, want=OFF)
# (``step`` runs the update it is asked for whatever learn_GT says: this case holds that the flag
# changes nothing there.  The W / KL-only variant of the GT kernel runs in every case's ID and ELBO
# steps; the fit loop with learn_GT off is flow B's fixed_gt)
_a("fixed_gt", "small", K=4, learn_gt=False, env=LDS0, want=OFF)
_a("theta_prior", "small", K=4, prior=[pr_theta], env=LDS0, want=OFF)
_a("gt_prior_row", "small", K=4, prior=[pr_gt_row], env=LDS0, want=OFF)
_a("gt_prior_full", "small", K=4, prior=[pr_gt_full], env=LDS0, want=OFF)
_a("gt_prior_full_T4", "small", K=5, T=4, prior=[pr_gt_full], env=LDS1, want=ON)
_a("id_prior_vector", "small", K=4, prior=[pr_id_vector], env=LDS0, want=OFF)
_a("id_prior_cells", "small", K=4, prior=[pr_id_cells], env=LDS0, want=OFF)
_a("id_prior_cells_K17", "small", K=17, prior=[pr_id_cells], env=LDS1, want=ON)
_a("bmm", "clone", K=5, kind="bmm", state=[st_random_theta], env=LDS0, want=OFF)
_a("bmm_lds", "clone", K=5, kind="bmm", state=[st_random_theta], env=LDS1, want=ON)
_a("bmm_clone_priors", "clone", K=5, kind="bmm", state=[st_random_theta], prior=[pr_bmm_clones], env=LDS0, want=OFF)
_a("bmm_fix_beta_sum", "clone", K=5, kind="bmm", fix=True, state=[st_random_theta], prior=[pr_bmm_clones],
   env=LDS0, want=OFF)
_a("bmm_id_prior_K3", "clone", K=3, kind="bmm", state=[st_random_theta], prior=[pr_id_cells], env=LDS1, want=ON)
# states where the special functions and the softmaxes break
_a("edge_shapes_a", "small", K=4, T=8, state=[st_edge_a], env=LDS0, want=OFF)
_a("edge_shapes_b", "small", K=4, T=8, state=[st_edge_b], env=LDS0, want=OFF)
_a("edge_shapes_prior", "count_free", K=3, T=3, ase=True, prior=[pr_theta_rows], env=LDS0, want=OFF)
_a("twin_classes", "small", K=4, state=[st_twins], env=LDS0, want=OFF)
_a("shape_in_6_7", "small", K=4, state=[st_in_6_7], env=LDS0, want=OFF)
_a("one_hot_id", "small", K=5, state=[st_one_hot_id], env=LDS0, want=OFF)
_a("one_hot_id_lds", "small", K=5, state=[st_one_hot_id], env=LDS1, want=ON)
_a("tiny_gt", "small", K=4, state=[st_tiny_gt], env=LDS0, want=OFF)
_a("underflow_id", "deep", K=4, state=[st_sharp_gt], env=LDS0, want=OFF)
_a("underflow_gt", "deep", K=4, state=[st_one_hot_id], env=LDS0, want=OFF)
_a("underflow_lds", "deep", K=4, state=[st_sharp_gt, st_one_hot_id], env=LDS1, want=ON)

# ---- every instance of vrx_spmm_lds, named ---------------------------------------------------
# Each case names the instances its passes must launch (inst_*: sets of (MODE, RW, PADK, SPLIT, FORM));
# the launch record of the model (DeviceModel.lds_launches) is held to them, and to the restated
# dispatch above block by block.  PADK, SPLIT per block of the pair-word passes / PADK of the AD/BD ones:
PAIR_BLOCKS = {2: {(1, 4)}, 3: {(1, 4)}, 4: {(0, 4)}, 6: {(1, 2)}, 7: {(1, 2)}, 8: {(0, 2)}, 11: {(1, 1)}, 15: {(1, 1)},
               16: {(0, 1)}, 17: {(1, 1), (1, 4)}, 18: {(1, 1), (1, 4)}, 33: {(1, 1), (1, 4)}}
F1_BLOCKS = {16: {0}, 7: {1}, 12: {2}, 6: {2}, 17: {1}, 18: {2}}
PAIRS = dict(LDS1, VIREO_CELL_FORM="0", VIREO_VAR_FORM="0")


def _pair_inst(K, rw_cell):
    return dict(inst_variant={(0, RW_VARIANT, pk, sp, 0) for pk, sp in PAIR_BLOCKS[K]},
                inst_cell={(1, rw_cell, pk, sp, 0) for pk, sp in PAIR_BLOCKS[K]})


def _f1_inst(K, rw_cell):      # (the variant pass over virtual rows: the cell pass's kernel at its tall tile)
    return dict(inst_variant={(1, RW_CELL, pk, 1, 1) for pk in F1_BLOCKS[K]},
                inst_cell={(1, rw_cell, pk, 1, 1) for pk in F1_BLOCKS[K]})


# pair words: the six PADK x SPLIT instances of the variant pass and of each cell tile height; K > 16:
# strided blocks of 16 with an odd (17, 33) and an even (18) row stride, and the blocks of 1 and 2 behind them
for K in (2, 4, 6, 8, 11, 16, 17, 18, 33):
    for tag, dat, rw in (("short", "pair_short", RW_CELL_SHORT), ("tall", "pair_tall", RW_CELL_PAIR)):
        _a("pair_%s_K%d" % (tag, K), dat, K=K, env=PAIRS,
           want=dict(ON, cell_form=0, var_form=0, perm=False, **_pair_inst(K, rw)))
# clone mode on the pair words its deep counts choose by themselves (nothing forced)
for K in (3, 8, 16):
    _a("clone_pairs_K%d" % K, "clone", K=K, kind="bmm", state=[st_random_theta], env=LDS1,
       want=dict(ON, cell_form=0, var_form=0, perm=False, **_pair_inst(K, RW_CELL_SHORT)))
# AD/BD words at the 96-row cell tile: flat rows, element-wise, whole units, strided blocks
for K in (16, 7, 12, 17):
    _a("shallow_tall_K%d" % K, "shallow_tall", K=K, env=LDS1,
       want=dict(ON, cell_form=1, var_form=3, perm=False, **_f1_inst(K, RW_CELL)))
# balanced slabs: the permuted gather of each staging path (flat, element-wise, whole units is
# ``balanced`` above), inside column blocks, and over rows cut into pieces
BALANCED = dict(LDS1, VIREO_BUILD="device", VIREO_LDS_SPLIT_X10="60")
for K in (16, 7, 17):
    _a("balanced_K%d" % K, "many", K=K, balance=True, env=BALANCED,
       want=dict(ON, balanced_variant=True, balanced_cell=True, device_built=True, cell_form=1, var_form=3,
                 perm=True, **_f1_inst(K, RW_CELL)))
_a("balanced_split_K16", "many", K=16, balance=True, env=dict(BALANCED, VIREO_LDS_SPLIT_X10="5"),
   want=dict(ON, balanced_variant=True, balanced_cell=True, device_built=True, cell_form=1, var_form=3,
             extra_pieces_cell=some, extra_pieces_variant=some, perm=True, **_f1_inst(16, RW_CELL)))
# (balanced slabs are AD/BD streams: asked for on pair words the build leaves the stream unbalanced and
# the pass gets no gather list -- the pair-word instances have no permuted staging)
_a("balanced_pairs", "pair_tall", K=6, balance=True, env=dict(PAIRS, VIREO_BUILD="device"),
   want=dict(ON, balanced_variant=False, balanced_cell=False, device_built=True, cell_form=0, var_form=0,
             perm=False, **_pair_inst(6, RW_CELL_PAIR)))
# slab edges: a last slab of one row and of one row short, in the flat copy (K = 16: lanes past the
# slab re-read its last unit) and the element-wise staging (K = 7), with the slabs as laid out for
# the CUs (VIREO_LDS_FILL_CUS=1: shortened) and at their nominal height
for tag in SLAB_EDGES:
    for fill in (1, 0):
        for K in (16, 7):
            env = dict(VIREO_LDS_FILL_CUS=str(fill))
            _a("slab_edge_%s_fill%d_K%d" % (tag, fill, K), "slab_edge_" + tag, K=K, env=dict(LDS1, **env),
               want=dict(ON, cell_form=1, var_form=3, perm=False,
                         slab_fill=bool(fill), **_f1_inst(K, RW_CELL_SHORT)))
            _a("slab_edge_%s_fill%d_pairs_K%d" % (tag, fill, K), "slab_edge_" + tag, K=K, env=dict(PAIRS, **env),
               want=dict(ON, cell_form=0, var_form=0, perm=False,
                         slab_fill=bool(fill), **_pair_inst(K, RW_CELL_SHORT)))

# the fit loop's own kernels and fusions
FUSE1, FUSE0 = {"VIREO_FUSE_SOFTMAX": "1"}, {"VIREO_FUSE_SOFTMAX": "0"}
# (fused_softmax: whether the cell softmax runs in the cell pass's epilogue -- small gather problems,
# one restart, K <= 16, no empty or split cell; the GPU test counts the launches of the run)
_b("fused_softmax", "small", K=4, env=dict(LDS0, **FUSE1), want=OFF, fused_softmax=True)
_b("separate_softmax", "small", K=4, env=dict(LDS0, **FUSE0), want=OFF, fused_softmax=False)
_b("fused_softmax_id_prior", "small", K=16, prior=[pr_id_cells], env=dict(LDS0, **FUSE1), want=OFF,
   fused_softmax=True)
_b("ride", "small", K=4, iters=2, env=dict(LDS0, VIREO_ELBO_RIDE="1", **FUSE1), want=OFF, fused_softmax=True)
_b("no_ride", "small", K=4, iters=2, env=dict(LDS0, VIREO_ELBO_RIDE="0", **FUSE1), want=OFF, fused_softmax=True)
_b("ride_lds", "mid", K=6, iters=2, env=dict(LDS1, VIREO_ELBO_RIDE="1"), want=ON, fused_softmax=False)
_b("lds_many_ranges", "many", K=6, env=LDS1, want=dict(ON, ranges_variant=many, ranges_cell=many))
_b("lds_split_rows", "split", K=6, env=LDS1, want=dict(ON, extra_pieces_cell=some, extra_pieces_variant=some))
_b("T8", "small", K=5, T=8, env=LDS0, want=OFF)
_b("ase", "small", K=4, ase=True, env=LDS0, want=OFF)
_b("fix_beta_sum", "small", K=4, fix=True, prior=[pr_theta], env=LDS0, want=OFF)
_b("fixed_gt", "small", K=4, learn_gt=False, iters=2, env=LDS0, want=OFF)
_b("gt_prior_full_lds", "small", K=9, prior=[pr_gt_full], env=LDS1, want=ON)
_b("clone", "clone", K=5, kind="bmm", state=[st_random_theta], iters=2,
   env=dict(LDS0, VIREO_ELBO_RIDE="1", **FUSE0), want=OFF, fused_softmax=False)
_b("clone_lds", "clone", K=5, kind="bmm", state=[st_random_theta], prior=[pr_bmm_clones],
   env=dict(LDS1, VIREO_ELBO_RIDE="0"), want=ON, fused_softmax=False)
_b("batch3", "mid", K=4, restarts=3, env=LDS1, want=dict(ON, n_batch=3))
_b("batch3_gather", "small", K=4, restarts=3, iters=2, env=LDS0, want=dict(OFF, n_batch=3))
# restart batches as one operand: 5 x 3 = 15 columns on pair words (one block, element-wise), 3 x 6 = 18
# columns on AD/BD words (blocks of 16 and 2 with an even row stride: whole 16-B units)
_b("batch5_pairs", "pair_short", K=3, restarts=5, env=PAIRS,
   want=dict(ON, n_batch=5, cell_form=0, var_form=0, perm=False, **_pair_inst(15, RW_CELL_SHORT)))
_b("batch3_blocks", "mid", K=6, restarts=3, env=LDS1,
   want=dict(ON, n_batch=3, cell_form=1, var_form=3, perm=False, **_f1_inst(18, RW_CELL_SHORT)))


# ---- the dense kernels past their grid caps -----------------------------------------------------
# Sizes are expressions in the grid terms (``grid_terms``: S1, S2, C, B, rows), evaluated for the
# device's CU count; ``route`` declares the sweeps / strides / trips the case must take (held to
# ``dense_grid`` on the CPU for three CU counts, and to ``DeviceModel.dense_launches()`` on the device
# before any number is compared).  The other dimension stays tiny.  An element's (n, k) matters only
# to the batched index (R > 1), the fused range sums (npiece[n], vptr), the per-donor and per-variant
# priors, W in planar form and psi in ASE mode: a K that divides the stride (16) never takes the wrap
# branch of the stepping, an odd K does in every sweep.
DENSE_A, DENSE_B = [], []


def _variants(elements, K, M=32, **thin):
    """N = the fewest variants with N K >= elements(g), on M cells"""
    return lambda g: (g.rows(elements(g), K), M, _thin(**thin))


def _cells(cells, N=32, **thin):
    return lambda g: (N, cells(g), _thin(**thin))


def _da(name, *a, **k):
    DENSE_A.append(name)
    _a(name, *a, **k)


def _db(name, *a, **k):
    DENSE_B.append(name)
    _b(name, *a, **k)


# the shared theta's second stage (``step`` runs it as vrx_theta_final): 256 partials = one per thread,
# 257 and 513 = two and three strides, 4 n_cu = the whole capped grid, still one sweep of the first stage
_da("dense_parts256", lambda g: (g.B * g.B // 5, 32, _thin()), K=5, env=LDS0, want=OFF,
    route=dict(theta_sweeps=1, final_strides=1, fuse=True))
_da("dense_parts257", lambda g: (g.B * g.B // 5 + 1, 32, _thin()), K=5, env=LDS0, want=OFF,
    route=dict(theta_sweeps=1, final_strides=2, fuse=False))
_da("dense_parts513", _variants(lambda g: 2 * g.B * g.B + 1, 7), K=7, env=LDS0, want=OFF,
    route=dict(theta_sweeps=1, final_strides=3, fuse=False))
_da("dense_theta_full_grid", lambda g: (g.S1 // 16, 32, _thin()), K=16, env=LDS0, want=OFF,
    route=dict(theta_sweeps=1, gt_sweeps=1, fuse=False))
# vrx_theta_partial past its cap: second and third sweep, step_k = 0 (K = 16) and the wrap (K = 17, 7, 5)
_da("dense_theta2_K16", _variants(lambda g: g.S1 + 1, 16), K=16, env=LDS0, want=OFF,
    route=dict(theta_sweeps=2, gt_sweeps=1))
_da("dense_theta2_K17", _variants(lambda g: g.S1 + 1, 17), K=17, env=LDS0, want=OFF,
    route=dict(theta_sweeps=2, gt_sweeps=1))
_da("dense_theta2_K5_T4", _variants(lambda g: g.S1 + 1, 5), K=5, T=4, env=LDS0, want=OFF,
    route=dict(theta_sweeps=2, gt_sweeps=1))
_da("dense_theta3_K7", _variants(lambda g: 2 * g.S1 + 3, 7), K=7, env=LDS0, want=OFF,
    route=dict(theta_sweeps=3, gt_sweeps=2))
# vrx_gt_update past its cap (learn = 1 in the GT step, learn = 0 in the ID and ELBO steps of every case)
_da("dense_gt2_K16", _variants(lambda g: g.S2 + 1, 16, M=24), K=16, env=LDS0, want=OFF,
    route=dict(theta_sweeps=3, gt_sweeps=2))
_da("dense_gt2_K17", _variants(lambda g: g.S2 + 1, 17, M=24), K=17, env=LDS0, want=OFF,
    route=dict(theta_sweeps=3, gt_sweeps=2))
_da("dense_gt2_K7_T4", _variants(lambda g: g.S2 + 1, 7, M=24), K=7, T=4, env=LDS0, want=OFF,
    route=dict(theta_sweeps=3, gt_sweeps=2))
_da("dense_gt3_K5", _variants(lambda g: 2 * g.S2 + 3, 5, M=24), K=5, env=LDS0, want=OFF,
    route=dict(theta_sweeps=5, gt_sweeps=3))
# what reads an element's (n, k), each on a strided shape with an odd K
_da("dense_gt2_prior_row", _variants(lambda g: g.S2 + 1, 17, M=24), K=17, prior=[pr_gt_row], env=LDS0, want=OFF,
    route=dict(gt_sweeps=2))
_da("dense_gt2_prior_full", _variants(lambda g: g.S2 + 1, 17, M=24), K=17, prior=[pr_gt_full], env=LDS0, want=OFF,
    route=dict(gt_sweeps=2))
_da("dense_gt2_fixed_gt", _variants(lambda g: g.S2 + 1, 17, M=24), K=17, learn_gt=False, env=LDS0, want=OFF,
    route=dict(gt_sweeps=2))
# (wform 0: every gather case above; wform 1: planar W for the AD/BD cell stream, row index n, column k)
_da("dense_gt2_planar_w", _variants(lambda g: g.S2 + 1, 17, M=24), K=17,
    env=dict(LDS1, VIREO_CELL_FORM="1", VIREO_VAR_FORM="3"), want=dict(ON, cell_form=1, var_form=3),
    route=dict(gt_sweeps=2))
_da("dense_gt2_pairs_w", _variants(lambda g: g.S2 + 1, 17, M=24), K=17, env=PAIRS,
    want=dict(ON, cell_form=0, var_form=0), route=dict(gt_sweeps=2))
# (ASE: psi row n.  One mpmath argument per variant and class in the reference, so K is large and N small)
_da("dense_gt2_ase_K63", _variants(lambda g: g.S2 + 1, 63, M=24), K=63, ase=True, state=[st_random_theta],
    env=LDS0, want=OFF, route=dict(gt_sweeps=2))

# the cell softmax past its cap: every KP at two sweeps, 16 / 32 / 64 at three; K inside its KP (5 in 8,
# 17 in 32, 33 in 64); the first sweep's preload must not reach the second
for _K in (16, 17, 33):
    _kp = pick_kp(_K)
    _da("dense_cell2_K%d" % _K, _cells(lambda g, kp=_kp: g.C // kp + 1), K=_K, env=LDS0, want=OFF,
        route=dict(cell_sweeps=2))
    _da("dense_cell3_K%d" % _K, _cells(lambda g, kp=_kp: 2 * (g.C // kp) + 3), K=_K, env=LDS0, want=OFF,
        route=dict(cell_sweeps=3))
_da("dense_cell2_K5", _cells(lambda g: g.C // 8 + 1, N=24), K=5, env=LDS0, want=OFF, route=dict(cell_sweeps=2))
CAP1 = {"VIREO_SOFTMAX_BLOCKS_PER_CU": "1"}
for _K in (2, 3, 8):
    _kp = pick_kp(_K)
    _da("dense_cell2_cap1_K%d" % _K, _cells(lambda g, kp=_kp: g.C // kp + 1, N=24), K=_K, env=dict(LDS0, **CAP1),
        want=OFF, route=dict(cell_sweeps=2))
# id_mode 0 is every case above; 1 and 2; logLik_ID summed from the LDS cell pass's output
_da("dense_cell2_id_vector", _cells(lambda g: g.C // 32 + 1), K=17, prior=[pr_id_vector], env=LDS0, want=OFF,
    route=dict(cell_sweeps=2))
_da("dense_cell2_id_cells", _cells(lambda g: g.C // 32 + 1), K=17, prior=[pr_id_cells], env=LDS0, want=OFF,
    route=dict(cell_sweeps=2))
_da("dense_cell2_lds", _cells(lambda g: g.C // 32 + 1), K=17, env=LDS1, want=ON, route=dict(cell_sweeps=2))

# the ELBO's second stage through vrx_elbo_final (VRX_STEP_ELBO): 2 048 cell partials = one trip, 2 049 = two,
# 4 097 = three, with the softmax's grid uncapped (KP = 64: four cells a block)
CAP0 = {"VIREO_SOFTMAX_BLOCKS_PER_CU": "0"}
for _blocks, _trips in ((2048, 1), (2049, 2), (4097, 3)):
    _da("dense_elbo_parts%d" % _blocks, _cells(lambda g, b=_blocks: 4 * b - 1, N=24), K=33,
        env=dict(LDS0, **CAP0), want=OFF, route=dict(elbo_trips=_trips, cell_sweeps=1, n_cell_part=_blocks))

# the fit loop at these sizes, two iterations (run_iters: no stop rule): the first ELBO rides in the second
# theta launch, the second has its own kernel; past 256 partials the theta finalisation is vrx_theta_final
RIDE1 = {"VIREO_ELBO_RIDE": "1"}
_db("dense_fit_parts256", lambda g: (g.B * g.B // 5, 32, _thin()), K=5, iters=2, env=dict(LDS0, **RIDE1, **FUSE0),
    want=OFF, fused_softmax=False, route=dict(theta_sweeps=1, fuse=True))
_db("dense_fit_parts257", lambda g: (g.B * g.B // 5 + 1, 32, _thin()), K=5, iters=2,
    env=dict(LDS0, **RIDE1, **FUSE0), want=OFF, fused_softmax=False, route=dict(theta_sweeps=1, fuse=False))
_db("dense_fit_theta2_K17", _variants(lambda g: g.S1 + 1, 17), K=17, iters=2, env=dict(LDS0, **RIDE1, **FUSE0),
    want=OFF, fused_softmax=False, route=dict(theta_sweeps=2, fuse=False))
_db("dense_fit_gt2_K7_R3", _variants(lambda g: g.S2 + 1, 7, M=24), K=7, iters=2, restarts=3,
    env=dict(LDS0, **RIDE1), want=dict(OFF, n_batch=3), route=dict(theta_sweeps=3, gt_sweeps=2, fuse=False))
# the range sums fused into the strided kernels: AD/BD virtual rows (var_form 3) and pair words
_db("dense_fit_theta2_virtual", _variants(lambda g: g.S1 + 1, 17), K=17, iters=2,
    env=dict(LDS1, VIREO_CELL_FORM="1", VIREO_VAR_FORM="3", **RIDE1), want=dict(ON, cell_form=1, var_form=3),
    route=dict(theta_sweeps=2, fuse=False))
# (pair words sum their ranges in the kernel only when a tile has several: 130 cells = 3 slabs of 64)
_db("dense_fit_theta2_pairs_R2", _variants(lambda g: g.S1 + 1, 17, M=130), K=17, iters=2, restarts=2,
    env=dict(PAIRS, **RIDE1), want=dict(ON, cell_form=0, var_form=0, n_batch=2, ranges_variant=many),
    route=dict(theta_sweeps=2, fuse=False))
# (rows cut into pieces -- vptr: two variants that cover every one of 200 cells)
_db("dense_fit_theta2_pieces", _variants(lambda g: g.S1 + 1, 17, M=200, full_rows=(5, -1)), K=17, iters=2,
    env=dict(LDS1, VIREO_CELL_FORM="1", VIREO_VAR_FORM="3", **RIDE1),
    want=dict(ON, cell_form=1, var_form=3, extra_pieces_variant=some), route=dict(theta_sweeps=2, fuse=False))
# logLik_ID from the LDS cell pass's ranges (200 variants = 4 slabs of 64), and from a cell cut into pieces
_db("dense_fit_cell2_lds", _cells(lambda g: g.C // 32 + 1, N=200, density=0.1), K=17, iters=2,
    env=dict(LDS1, **RIDE1), want=dict(ON, ranges_cell=many), fused_softmax=False, route=dict(cell_sweeps=2))
_db("dense_fit_cell2_pieces", _cells(lambda g: g.C // 32 + 1, N=200, density=0.1, full_cols=(3, -1)), K=17, iters=2,
    env=dict(LDS1, **RIDE1), want=dict(ON, extra_pieces_cell=some), fused_softmax=False, route=dict(cell_sweeps=2))
_db("dense_fit_cell2_R3", _cells(lambda g: g.C // 8 + 1, N=24), K=5, iters=2, restarts=3, env=dict(LDS1, **RIDE1),
    want=dict(ON, n_batch=3), route=dict(cell_sweeps=2))
# the ELBO's second stage in the ride block: the softmax's grid uncapped, and the fused cell pass (one
# partial per block of VRX_WAVES segments, padded: ``fused_cell_segments``)
_db("dense_fit_elbo_parts2049", _cells(lambda g: 4 * 2049 - 1, N=24), K=33, iters=2,
    env=dict(LDS0, **RIDE1, **CAP0, **FUSE0), want=OFF, fused_softmax=False,
    route=dict(elbo_trips=2, n_cell_part=2049))
_db("dense_fit_fused_cells2056", _cells(lambda g: 8193, N=24, cells_full=True), K=4, iters=2,
    env=dict(LDS0, **RIDE1, **FUSE1), want=OFF, fused_softmax=True, route=dict(elbo_trips=2, n_cell_part=2056))
_db("dense_fit_fused_cells4104", _cells(lambda g: 16385, N=24, cells_full=True), K=16, iters=2,
    env=dict(LDS0, **RIDE1, **FUSE1), want=OFF, fused_softmax=True, route=dict(elbo_trips=3, n_cell_part=4104))
# clone mode with the range sum fused into vrx_bmm_theta: 16 lanes an element, N K / 16 KL_theta partials
# (fused only when a tile has several ranges: 130 cells = 3 slabs of 64.  One iteration: the reference
# costs six mpmath arguments per element and iteration, so this ELBO has vrx_elbo_final for its carrier;
# the ride block's trips are held by the cell partials above -- the same vrx_elbo_final_block)
_db("dense_fit_clone_parts2049", lambda g: (4097, 130, _thin(density=0.5, depth=30.0)), K=8, kind="bmm",
    state=[st_random_theta], iters=1, env=dict(PAIRS, **RIDE1), want=dict(ON, var_form=0, ranges_variant=many),
    route=dict(elbo_trips=2, n_th_part=2049, fused_range_sum=True))

# What the sweep leaves out, with the reason (the run's table repeats it):
NOT_COVERED = (
    ("n_gt_part > 2048", "nb_gt = min(.., 8 n_cu): 2 048 at 256 CUs, never more"),
    ("clone mode without the fused range sum, n_th_part > 2048",
     "needs N K > 524 288 with one mpmath argument per element of the reference; repeated variant rows would "
     "hide an (n, k) mix-up"),
)


# ------------------------------------------------------------------------------------
# a case's problem: data, states, priors, exact counts
# ------------------------------------------------------------------------------------
def _counts_of(spec, n_cu):
    if callable(spec.data):
        N, M, make = dense_shape(spec, n_cu)
        ad, dp = make(N, M)
        return csc_matrix(ad), csc_matrix(dp)
    return data(spec.data)


@functools.lru_cache(maxsize=2)
def _problem(flow, name, n_cu):
    spec = (CASES_A if flow == "A" else CASES_B)[name]
    AD, DP = _counts_of(spec, n_cu)
    p = SimpleNamespace(spec=spec, AD=AD, DP=DP, N=AD.shape[0], M=AD.shape[1], K=spec.K, T=spec.T,
                        kind=spec.kind)
    p.C = X.Counts(AD, DP)
    rng = np.random.default_rng(1000 + spec.seed)
    rows, cols = ((p.N if spec.ase else 1), p.T) if p.kind == "vireo" else (p.N, p.K)
    p.states = []
    for _ in range(spec.restarts):
        s = SimpleNamespace(ID=O.unit_sum(rng.random((p.M, p.K))),
                            GT=O.unit_sum(rng.random((p.N, p.K, p.T))) if p.kind == "vireo" else None)
        if p.kind == "vireo":   # the constructor's theta (vireo_model.py:84-93, bmm_model.py:70-77)
            s.mu = np.ones((rows, cols)) * np.linspace(0.01, 0.99, p.T)
            s.sm = np.full((rows, cols), 50.0)
        else:
            s.mu, s.sm = np.full((rows, cols), 0.5), np.full((rows, cols), 30.0)
        for f in spec.state:
            f(s, p, rng)
        p.states.append(s)
    p.s0 = p.states[0]
    if p.kind == "vireo":       # default priors: vireo_model.py:107-137, bmm_model.py:87-105
        g = np.linspace(0.01, 0.99, p.T)[None, :]
        pri = dict(ID_prior=None, GT_prior=None, th1=g * 50.0, th2=(1 - g) * 50.0)
    else:
        pri = dict(ID_prior=None, GT_prior=None, th1=np.ones((1, p.K)), th2=np.ones((1, p.K)))
    for f in spec.prior:
        pri.update(f(p, rng))
    p.pri = SimpleNamespace(**pri)
    return p


def problem_a(name):
    return _problem("A", name, N_CU)


def problem_b(name):
    return _problem("B", name, N_CU)


# ------------------------------------------------------------------------------------
# the exact side
# ------------------------------------------------------------------------------------
def _elbo_of(parts):
    """LB_p - KL_ID - KL_GT - KL_theta (vireo_model.py:248, bmm_model.py:175); units add"""
    have = [k for k in PARTS if k in parts]
    val = parts["LB_p"][0] - sum(parts[k][0] for k in have[1:])
    return val, sum(parts[k][1] for k in have)


def exact_a(p):
    """name -> (value, unit) of every update from the case's state, and the logLik_ID handed to the
    ELBO (the exact one rounded to float64)"""
    if getattr(p, "_exact_a", None) is None:
        c, s, pri, sp = p.C, p.s0, p.pri, p.spec
        if p.kind == "vireo":
            out = X.vireo_theta(c, s.ID, s.GT, pri.th1, pri.th2, s.sm, ase=sp.ase, fix_beta_sum=sp.fix)
            out.update(X.vireo_gt(c, s.ID, s.mu, s.sm, pri.GT_prior, p.T))
            out.update(X.vireo_loglik(c, s.GT, s.mu, s.sm))
        else:
            out = X.bmm_theta(c, s.ID, pri.th1, pri.th2, s.sm, fix_beta_sum=sp.fix)
            out.update(X.bmm_loglik(c, s.mu, s.sm))
        out.update(X.id_from_loglik(*out["logLik_ID"], pri.ID_prior, p.K))
        p.L_given = out["logLik_ID"][0].astype(np.float64)
        out.update(_exact_parts(p, p.L_given))
        out["re_logLik_ID"] = out["logLik_ID"]
        p._exact_a = out
    return p._exact_a


def _exact_parts(p, L):
    s, pri = p.s0, p.pri
    if p.kind == "vireo":
        out = X.vireo_elbo_parts(L, s.ID, s.GT, s.mu, s.sm, pri.ID_prior, pri.GT_prior, pri.th1, pri.th2)
    else:
        out = X.bmm_elbo_parts(L, s.ID, s.mu, s.sm, pri.ID_prior, pri.th1, pri.th2)
    out["ELBO"] = _elbo_of(out)
    return out


# ------------------------------------------------------------------------------------
# the float64 oracle as a backend
# ------------------------------------------------------------------------------------
def oracle_state(p, s):
    sp, pri = p.spec, p.pri
    st = SimpleNamespace(n_cell=p.M, n_var=p.N, n_donor=p.K, n_GT=p.T, learn_GT=sp.learn_gt,
                         learn_theta=True, ASE_mode=sp.ase, fix_beta_sum=sp.fix,
                         beta_mu=s.mu.copy(), beta_sum=s.sm.copy(), ID_prob=s.ID.copy(),
                         theta_s1_prior=pri.th1, theta_s2_prior=pri.th2)
    st.ID_prior = pri.ID_prior if pri.ID_prior is not None else O.unit_sum(np.ones((p.M, p.K)))
    if p.kind == "vireo":
        st.GT_prob = s.GT.copy()
        # (one (1, K, T) slab: spelled out, update_GT_prob sizes its logits by the prior, vireo_model.py:210)
        st.GT_prior = (np.broadcast_to(pri.GT_prior, s.GT.shape) if pri.GT_prior is not None
                       else O.unit_sum(np.ones((p.N, p.K, p.T))))
    return st


def _bmm_parts(st, L):
    """the terms of bmm_model.py:157-175, apart"""
    s1, s2 = O._shape12(st)
    return (np.sum(L * st.ID_prob), np.sum(entropy(st.ID_prob, st.ID_prior, axis=-1)), 0.0,
            O.beta_kl(np.append(s1[:, None, :], s2[:, None, :], axis=1),
                      np.append(st.theta_s1_prior[:, None, :], st.theta_s2_prior[:, None, :], axis=1)))


class OracleBackend:
    """oracle/vireo_oracle.py's step functions; ``digamma`` may be swapped for the corruption tests"""

    def __init__(self, p):
        self.p = p

    def _st(self, r=0):
        return oracle_state(self.p, self.p.states[r])

    def theta(self):
        st, p = self._st(), self.p
        (O.vireo_theta_step if p.kind == "vireo" else O.bmm_theta_step)(st, p.AD, p.DP)
        return st.beta_mu, st.beta_sum

    def gt(self):
        st = self._st()
        O.vireo_gt_step(st, self.p.AD, self.p.DP)
        return st.GT_prob

    def loglik(self, st=None):
        st, p = st or self._st(), self.p
        if p.kind == "vireo":
            return O._cell_loglik(st.GT_prob, *O._psi3(st), p.AD, p.DP)
        return O.bmm_cell_loglik(st, p.AD, p.DP)

    def id(self):
        st = self._st()
        L = self.loglik(st)
        st.ID_prob = O.softmax_log(L + np.log(st.ID_prior))
        return L, st.ID_prob

    def parts(self, st, L):
        return np.array(O.vireo_elbo_parts(st, L) if self.p.kind == "vireo" else _bmm_parts(st, L))

    def elbo(self, L):
        return self.parts(self._st(), L)

    def elbo_recomputed(self):
        st = self._st()
        L = self.loglik(st)
        return L, self.parts(st, L)

    def run(self, r, n):
        """n iterations from restart r's state (vireo_model.py:257-264, bmm_model.py:183-188)"""
        st, p = self._st(r), self.p
        trace = []
        for _ in range(n):
            if p.kind == "vireo":
                O.vireo_theta_step(st, p.AD, p.DP)
                if p.spec.learn_gt:
                    O.vireo_gt_step(st, p.AD, p.DP)
            else:
                O.bmm_theta_step(st, p.AD, p.DP)
            L = self.loglik(st)
            st.ID_prob = O.softmax_log(L + np.log(st.ID_prior))
            parts = self.parts(st, L)
            trace.append(parts[0] - parts[1] - parts[2] - parts[3])
        return SimpleNamespace(ID=st.ID_prob, GT=getattr(st, "GT_prob", None), mu=st.beta_mu, sm=st.beta_sum,
                               L=L, trace=np.array(trace), parts=parts)


# ------------------------------------------------------------------------------------
# the flows and the judge
# ------------------------------------------------------------------------------------
def _name_parts(out, parts, pre=""):
    for k, v in zip(PARTS, parts):
        out[pre + k] = v
    out[pre + "ELBO"] = parts[0] - parts[1] - parts[2] - parts[3]


def run_a(p, be):
    """every update once, each from the case's state -> name -> float64 result"""
    exact_a(p)                                   # (fixes the logLik_ID handed to the ELBO)
    out = {}
    out["beta_mu"], out["beta_sum"] = be.theta()
    if p.kind == "vireo":
        out["GT_prob"] = be.gt()
    out["logLik_ID"], out["ID_prob"] = be.id()
    _name_parts(out, be.elbo(p.L_given))
    out["re_logLik_ID"], parts = be.elbo_recomputed()
    out["re_LB_p"] = parts[0]
    if p.kind != "vireo":
        del out["KL_GT"]
    return out


def distances_a(p, out):
    ex = dict(exact_a(p))
    ex["re_LB_p"] = _exact_parts(p, out["re_logLik_ID"])["LB_p"]     # its own logLik_ID is the input
    return {k: X.distance(np.reshape(v, np.shape(ex[k][0])), *ex[k]) for k, v in out.items()}


def run_b(p, be, r=0):
    """restart r after 1, 2, ... iterations of the fit loop, each run from the case's state: the
    float64 state, logLik_ID, trace and ELBO parts a backend reads back after each length"""
    return [be.run(r, n) for n in range(1, p.spec.iters + 1)]


def _exact_stages(p, prev, res):
    """one iteration, every update judged on its own: the exact update of the float64 state the
    backend itself read back in front of it (as re_LB_p in flow A), so what an earlier update
    rounded is input here, not error.  prev: the state before the iteration, res: what the backend
    holds after it.  A backend that cannot read its logLik_ID back (a restart batch) leaves
    res.L = None: the exact logLik_ID of its state stands in, and its unit is carried into ID_prob
    (the softmax's rule) and into LB_p (sum of unit(L) * ID_prob)."""
    c, pri, sp = p.C, p.pri, p.spec
    if p.kind == "vireo":
        ex = X.vireo_theta(c, prev.ID, prev.GT, pri.th1, pri.th2, prev.sm, ase=sp.ase, fix_beta_sum=sp.fix)
        if sp.learn_gt:
            ex.update(X.vireo_gt(c, prev.ID, res.mu, res.sm, pri.GT_prior, p.T))
        else:                                     # GT_prob stays, to the bit
            ex["GT_prob"] = (X.ld(prev.GT), np.zeros(prev.GT.shape))
        ex.update(X.vireo_loglik(c, res.GT, res.mu, res.sm))
    else:
        ex = X.bmm_theta(c, prev.ID, pri.th1, pri.th2, prev.sm, fix_beta_sum=sp.fix)
        ex.update(X.bmm_loglik(c, res.mu, res.sm))
    if res.L is None:
        L, uL = ex.pop("logLik_ID")
        ex.update(X.id_from_loglik(L, uL, pri.ID_prior, p.K))
    else:                                         # its own logLik_ID: one rounding of each logit
        L, uL = X.ld(res.L), 0.0
        ex.update(X.id_from_loglik(L, X.EPS * np.abs(L), pri.ID_prior, p.K))
    if p.kind == "vireo":
        parts = X.vireo_elbo_parts(L, res.ID, res.GT, res.mu, res.sm, pri.ID_prior, pri.GT_prior, pri.th1, pri.th2)
    else:
        parts = X.bmm_elbo_parts(L, res.ID, res.mu, res.sm, pri.ID_prior, pri.th1, pri.th2)
    parts["LB_p"] = (parts["LB_p"][0], parts["LB_p"][1] + np.sum(uL * X.ld(res.ID)))
    parts["ELBO"] = _elbo_of(parts)
    ex.update(parts)
    return ex


def distances_b(p, snaps, r=0):
    """name -> distance in units.  The last iteration's outputs carry their plain names, an earlier
    one's end in @<iteration>.  ELBO is the entry of the LONGEST run's trace (the one that rode in
    the next iteration's theta launch), judged from the state the run of that length left; the four
    parts are those of the last iteration."""
    prev, out, last = p.states[r], {}, len(snaps) - 1
    for it, res in enumerate(snaps):
        ex = _exact_stages(p, prev, res)
        got = dict(beta_mu=res.mu, beta_sum=res.sm, ID_prob=res.ID, ELBO=snaps[-1].trace[it])
        if p.kind == "vireo":
            got["GT_prob"] = res.GT
        if res.L is not None:
            got["logLik_ID"] = res.L
        if it == last:
            got.update((k, v) for k, v in zip(PARTS, res.parts) if k in ex)
        for k, v in got.items():
            u = X.distance(np.reshape(v, np.shape(ex[k][0])), *ex[k])
            out[k if it == last else "%s@%d" % (k, it)] = u
        prev = res
    return out


def a_priori(p):
    """what recursive summation of the longest contracted row or column may lose, in units, plus 16
    for forming a term: the float64 oracle has to stay inside, or the unit is degenerate"""
    return p.C.longest + 16
