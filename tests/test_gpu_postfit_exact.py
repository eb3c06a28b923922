"""The steps outside the fit loop on the device, against the extended-precision restatement.

``vrx_problem_doublet`` (the pair-class walk of ``vrx_doublet_w``, the cell pass at K + K (K - 1) / 2
columns, the softmax), ``vrx_problem_cell_loglik`` (results and error paths), ``vrx_problem_donor_reads``
(the variant pass of a clone-mode model of any column count) and ``vrx_varmix_fit`` at its shortest
fit (every instance K = 2 ... 8) were held at 1e-5 ... 1e-12 relative, or by nothing.  Here every
output is held to its own error unit (tests/exact_np.py), by the rule of
tests/test_gpu_update_exact.py:

    u_dev = |device - exact| / unit  <=  4 * max(u_orc, 1)

with u_orc the float64 side's distance on the same input (the oracle's pieces, SciPy's products,
tests/varmix_np.py); the bound is never formed from the device's own value.  All four take explicit
float64 or integer inputs, which the exact side takes as exact; they are called through ctypes, as
tests/test_gpu_postfit_sweep.py calls ``vrx_problem_ambient``.  The cases are in
tests/exact_postfit.py; the same sweep runs on the CPU with float64 NumPy in the device's place
(tests/test_exact_postfit_cpu.py).

The path: ``build_info()`` and ``entry_format()`` of the counts are asserted directly.  The entry
points create their model inside the library, so a ``DeviceModel`` of the same configuration on the
same counts is created beside each call and its ``info()`` asserted (doublets: kind vireo, C donors,
one class; ``cell_loglik``: kind vireo, n_col donors, n_class classes; donor reads: kind bmm, n_col
clones).  That model is a STAND-IN: it shows what a model of that shape runs on these counts under
this environment, not what the call itself ran.

VIREO_POSTFIT_UNITS_OUT=<file> writes the table of the run (profiles/postfit_exact_units.txt).
"""
import os

import numpy as np
import pytest
from scipy.sparse import csr_matrix

from tests import exact_postfit as XP

pytestmark = pytest.mark.gpu

# (step, case, output) whose device arithmetic is legitimate and further out than the rule allows:
# measured units x 1.25, with the reason -- none so far
PINNED = {}

_ROWS = []


@pytest.fixture(scope="module")
def va():
    import vireo_amd
    from vireo_amd import _lib
    _lib.require_gpu()          # fail loudly: there is no CPU fallback
    yield vireo_amd
    path = os.environ.get("VIREO_POSTFIT_UNITS_OUT")
    if path:
        _write_table(path)


def _write_table(path):
    with open(path, "w") as f:
        f.write("# distance from the extended-precision restatement of one post-fit step, in error units\n"
                "# (tests/exact_np.py): the device's, the float64 side's, and the bound 4 * max(float64, 1)\n"
                "# doublet: vrx_problem_doublet; cell: vrx_problem_cell_loglik; reads: vrx_problem_donor_reads;\n"
                "# varmix: vrx_varmix_fit at max_iter = 2, the worst row of each (K, depth) group\n")
        f.write("%-8s %-32s %-10s %10s %10s %10s\n" % ("step", "case", "output", "device", "float64", "bound"))
        for row in _ROWS:
            f.write("%-8s %-32s %-10s %10.3f %10.3f %10.3f\n" % row)
        f.write("\n# worst case of each output (largest device distance; largest share of its bound)\n")
        for step in ("doublet", "cell", "reads", "varmix"):
            for out in sorted({r[2] for r in _ROWS if r[0] == step}):
                rows = [r for r in _ROWS if r[0] == step and r[2] == out]
                far = max(rows, key=lambda r: r[3])
                tight = max(rows, key=lambda r: r[3] / r[5])
                f.write("%-8s %-10s %10.3f units in %-32s %5.2f of the bound in %s\n"
                        % (step, out, far[3], far[1], tight[3] / tight[5], tight[1]))


def _lds_params(table, n_col):
    return [pytest.param(name, tag, id="%s-%s" % (name, tag)) for name, sp in table.items()
            for tag, _, _ in XP.lds_settings(sp.data if hasattr(sp, "data") else "small", n_col(sp))]


def _counts(p, data, n_col, tag, monkeypatch):
    """the counts under the case's VIREO_LDS setting -> (counts, whether the LDS-resident passes must run)"""
    from vireo_amd.counts import DeviceCounts
    env, lds = {t: (e, on) for t, e, on in XP.lds_settings(data, n_col)}[tag]
    for k in ("VIREO_BUILD", "VIREO_ENTRY_FMT", "VIREO_LDS_BLOCKS", "VIREO_CELL_FORM", "VIREO_VAR_FORM"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    counts = DeviceCounts(p.AD, p.DP)
    # small problems, nothing forced: the host builder, no balanced slabs, the narrowest entry format
    info = counts.build_info()
    assert not info["device_built"] and not info["balanced_variant"] and not info["balanced_cell"]
    top = int(p.DP.max())
    fmt = 0 if top < 64 else 1 if top < 65536 else 2
    assert counts.entry_format() == (fmt, fmt)
    return counts, lds


def _assert_stand_in(counts, kind, n_col, lds, data, sides=("lds_variant", "lds_cell"), **kw):
    """``info()`` of a model of the call's configuration on the same counts (see the module text)"""
    from vireo_amd.engine import DeviceModel
    dm = DeviceModel(counts, kind, n_col, **kw)
    seen = dm.info()
    dm.close()
    for side in sides:
        assert seen[side] == lds, (side, seen)
        ranges = seen["ranges_" + side[4:]]
        if lds:
            assert ranges > 1 if data == "many" else ranges >= 1, (side, seen)
    assert (seen["fmt_variant"], seen["fmt_cell"]) == counts.entry_format()
    return seen


def _doublet(counts, p):
    from vireo_amd import _lib
    from vireo_amd._lib import dptr
    L, P = np.full((p.M, p.n_col), -7.0), np.full((p.M, p.n_col), -7.0)
    prior = p.prior_both
    _lib.check(_lib.lib().vrx_problem_doublet(
        counts.handle, p.K, p.T, dptr(p.GT), dptr(p.psi[0]), dptr(p.psi[1]), dptr(p.psi[2]), p.psi[0].shape[0],
        dptr(prior), 0 if prior is None else prior.shape[0], dptr(L), dptr(P)))
    return dict(logLik=L, prob=P)


def _cell_loglik(counts, GT, psi, prior, want_prob=True):
    from vireo_amd import _lib
    from vireo_amd._lib import dptr, f64
    GT, psi = f64(GT), [f64(x) for x in psi]
    M, n_col = counts.n_cell, GT.shape[1]
    L = np.full((M, n_col), -7.0)
    P = np.full((M, n_col), -7.0) if want_prob else None
    prior = None if prior is None else f64(prior)
    _lib.check(_lib.lib().vrx_problem_cell_loglik(
        counts.handle, n_col, GT.shape[2], dptr(GT), dptr(psi[0]), dptr(psi[1]), dptr(psi[2]), psi[0].shape[0],
        dptr(prior), 0 if prior is None else prior.shape[0], dptr(L), dptr(P)))
    return dict(logLik=L, prob=P) if want_prob else dict(logLik=L)


# =============================================================================== doublets
@pytest.mark.parametrize("name,tag", _lds_params(XP.DOUBLET, lambda sp: sp.K + sp.K * (sp.K - 1) // 2))
def test_doublet_step_against_exact(va, monkeypatch, name, tag):
    from vireo_amd import _lib
    p = XP.doublet_problem(name)
    counts, lds = _counts(p, p.spec.data, p.n_col, tag, monkeypatch)
    _assert_stand_in(counts, _lib.KIND_VIREO, p.n_col, lds, p.spec.data, n_gt=1)
    ex = XP.doublet_exact(p)
    u_dev = XP.distances(_doublet(counts, p), ex)
    u_orc = XP.distances(XP.doublet_np(p), ex)
    counts.close()
    XP.judge(_ROWS, PINNED, "doublet", "%s %s" % (name, tag), u_dev, u_orc)


@pytest.mark.parametrize("name", XP.CROSS)
@pytest.mark.parametrize("tag", ["gather", "lds"])
def test_explicit_pair_table_through_cell_loglik(va, monkeypatch, name, tag):
    """the host's add_doublet_GT table (G <= 6 classes) through ``vrx_problem_cell_loglik`` and the
    kernel's own pair walk through ``vrx_problem_doublet``, on the same inputs: both judged against
    the same exact value (the float64 table is rounded, the walk is not a table: not bitwise equal)"""
    from vireo_amd import _lib
    from vireo_amd.vireo_doublet import add_doublet_GT
    p = XP.doublet_problem(name)
    counts, lds = _counts(p, p.spec.data, p.n_col, tag, monkeypatch)
    table = add_doublet_GT(p.GT)
    assert table.shape == (p.N, p.n_col, p.T + p.T * (p.T - 1) // 2) and table.shape[2] <= 6
    _assert_stand_in(counts, _lib.KIND_VIREO, p.n_col, lds, p.spec.data, n_gt=table.shape[2], learn_gt=False)
    ex = XP.doublet_exact(p)
    u_orc = XP.distances(XP.doublet_np(p), ex)
    via_table = _cell_loglik(counts, table, p.psi, p.prior_both)
    via_walk = _doublet(counts, p)
    counts.close()
    XP.judge(_ROWS, PINNED, "cell", "%s table %s" % (name, tag), XP.distances(via_table, ex), u_orc)
    XP.judge(_ROWS, PINNED, "doublet", "%s walk %s" % (name, tag), XP.distances(via_walk, ex), u_orc)


# =============================================================================== cell_loglik
@pytest.mark.parametrize("name,tag", _lds_params(XP.CELL, lambda sp: sp.n_col))
def test_cell_loglik_against_exact(va, monkeypatch, name, tag):
    from vireo_amd import _lib
    p = XP.cell_problem(name)
    sp = p.spec
    counts, lds = _counts(p, "small", p.n_col, tag, monkeypatch)
    _assert_stand_in(counts, _lib.KIND_VIREO, p.n_col, lds, "small", n_gt=p.n_class, learn_gt=False,
                     learn_theta=False, ase_mode=sp.psi_full)
    ex = XP.cell_exact(p)
    out = _cell_loglik(counts, p.GT, p.psi, p.prior, want_prob=sp.mode != "null")
    counts.close()
    XP.judge(_ROWS, PINNED, "cell", "%s %s" % (name, tag), XP.distances(out, ex), XP.distances(XP.cell_np(p), ex))


def test_cell_loglik_refuses_and_stays_usable(va, monkeypatch):
    """nine classes: VRX_ERR_UNSUPPORTED with its message; psi or prior rows that are neither 1 nor
    n: the argument error; after each of them the problem computes what it computed before"""
    from vireo_amd import _lib
    from vireo_amd._lib import dptr
    p = XP.cell_problem("c5_g3")
    counts, _ = _counts(p, "small", p.n_col, "gather", monkeypatch)
    lib = _lib.lib()
    good = _cell_loglik(counts, p.GT, p.psi, None)
    L, P = np.empty((p.M, p.n_col)), np.empty((p.M, p.n_col))
    GT9, psi9 = np.full((p.N, p.n_col, 9), 1.0 / 9), np.zeros((1, 9))
    prior2, psi2 = np.full((2, p.n_col), 0.2), np.zeros((2, 3))
    psi = [np.ascontiguousarray(x) for x in p.psi]
    calls = [
        ((9, dptr(GT9), dptr(psi9), dptr(psi9), dptr(psi9), 1, None, 0), -4, b"9 genotype classes unsupported"),
        ((3, dptr(p.GT), dptr(psi2), dptr(psi2), dptr(psi2), 2, None, 0), -1, b"psi rows must be 1 or n_var"),
        ((3, dptr(p.GT), dptr(psi[0]), dptr(psi[1]), dptr(psi[2]), psi[0].shape[0], dptr(prior2), 2), -1,
         b"ID_prior must have 0, 1 or n_cell rows"),
    ]
    assert p.N != 2 and p.M != 2
    for args, code, text in calls:
        rc = lib.vrx_problem_cell_loglik(counts.handle, p.n_col, *args, dptr(L), dptr(P))
        assert rc == code and text in lib.vrx_last_error(), (rc, lib.vrx_last_error())
        again = _cell_loglik(counts, p.GT, p.psi, None)
        assert np.array_equal(again["logLik"], good["logLik"]) and np.array_equal(again["prob"], good["prob"])
    counts.close()


# =============================================================================== donor reads
@pytest.mark.parametrize("name,tag", _lds_params(XP.READS, lambda sp: sp.n_col))
def test_donor_reads_against_exact(va, monkeypatch, name, tag):
    from vireo_amd import _lib
    p = XP.reads_problem(name)
    counts, lds = _counts(p, p.spec.data, p.n_col, tag, monkeypatch)
    _assert_stand_in(counts, _lib.KIND_BMM, p.n_col, lds, p.spec.data, sides=("lds_variant",))
    ex = XP.reads_exact(p)
    A, D = counts.donor_reads(p.ID)
    counts.close()
    XP.judge(_ROWS, PINNED, "reads", "%s %s" % (name, tag), XP.distances(dict(AD_reads=A, DP_reads=D), ex),
             XP.distances(XP.reads_np(p), ex))


# =============================================================================== per-variant mixtures
@pytest.fixture(scope="module")
def mixtures(va):
    from vireo_amd import _lib
    assert int(_lib.lib().vrx_varmix_wave_rows()) == XP.VM_W
    AD, DP, _ = XP.varmix_rows()
    vm = va.VariantMixtures(csr_matrix(AD), csr_matrix(DP))
    assert np.array_equal(vm.n_covered, (DP > 0).sum(1))
    yield vm
    vm.close()


@pytest.mark.parametrize("K", XP.VM_KS)
def test_varmix_shortest_fit_against_exact(va, mixtures, K):
    """vrx_varmix_fit_k<K> at max_iter = 2, min_iter = 5: iterations 0 and 1 of every row, no stop
    rule.  Distances are the worst over the rows of a (K, depth) group, the device's and float64's alike."""
    fit = mixtures.fit(n_clone=K, return_trace=True, **XP.VM_FIT)
    assert np.all(fit["n_iter"] == 1) and np.all(fit["warn"] == 0)
    trace = np.array(fit["trace"])
    assert trace.shape == (mixtures.n_var, 2)
    assert fit["elbo"].tobytes() == trace[:, 0].tobytes()
    assert fit["gain"].tobytes() == (fit["elbo"] - fit["elbo_one"]).tobytes()
    rows = [{"trace[0]": trace[v, 0], "trace[1]": trace[v, 1], "beta_mu": fit["beta_mu"][v],
             "beta_sum": fit["beta_sum"][v], "size": fit["size"][v], "elbo_one": fit["elbo_one"][v]}
            for v in range(mixtures.n_var)]
    u_dev, u_orc = XP.varmix_distances(K, rows), XP.varmix_distances(K, XP.varmix_np(K))
    failed = []
    for group in sorted({g for g, _ in u_dev}):
        try:
            XP.judge(_ROWS, PINNED, "varmix", "K%d %s" % (K, group), {k: u for (g, k), u in u_dev.items() if g == group},
                     {k: u for (g, k), u in u_orc.items() if g == group})
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, "\n".join(failed)
