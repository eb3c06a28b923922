"""variant_mixture_gain / VariantMixtures on the GPU (vrx_varmix.h) against the NumPy restatement of the contract
(tests/varmix_np.py, proven equal to the oracle in tests/test_varmix_cpu.py): every row length at which the
kernel changes its path, K in {2, 3, 5, 8}, the stop rule per variant, the reference's own fixture, special
rows, deep counts against a 40-digit run, bitwise independence of a row from its call, the public path and
the command.  Bounds: the project's parity bound 1e-5 (smoke(), README "Known deviations").

Observed on an MI355X (worst over all cases, relative as bounded below): elbo 5.0e-12, elbo_one 3.1e-11, gain
1.5e-11, trace 1.2e-11, beta_mu 3.9e-15, beta_sum 2.0e-13, size 3.5e-13; deep counts 1.4e-14 from the 40-digit run
(the float64 restatement: 8.9e-15).  Also in the "Per-variant clone mixtures" paragraph of DESIGN.md."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
from scipy.sparse import csc_matrix, csr_matrix

from tests import varmix_np as VN

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TOL = 1e-5
KS = (2, 3, 5, 8)
PARAMS = dict(max_iter=60, min_iter=2, epsilon_conv=1e-2)


@pytest.fixture(scope="module")
def va():
    import __graft_entry__ as entry
    entry.build()
    import vireo_amd
    from vireo_amd import _lib
    _lib.require_gpu()
    return vireo_amd


def wave_rows():
    from vireo_amd import _lib
    return int(_lib.lib().vrx_varmix_wave_rows())


@functools.lru_cache(maxsize=None)
def problem():
    """(AD, DP) dense: every row length of the issue, each with all three depths and several rate kinds.
    Short rows live in 300 cells, the rows around and above the wave / workgroup threshold in 4 W + 3.
    A workgroup pass takes 256 lanes x 2 entries = 512 entries, a wave pass 128: 127 / 128 / 129 and
    2 x 512 -+ 1 sit on those boundaries (W - 1, W, W + 1 on the first workgroup boundary as well)."""
    W = wave_rows()
    short = [0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300]
    long_ = [W - 1, W, W + 1, 2 * W - 1, 2 * W, 2 * W + 1, 4 * W + 3]
    A1, D1 = VN.gen_rows(short * 5, seed=11)
    A2, D2 = VN.gen_rows(long_ * 3, seed=12, n_cell=4 * W + 3)
    n_cell = 4 * W + 3
    AD = np.zeros((A1.shape[0] + A2.shape[0], n_cell), dtype=np.int64)
    DP = np.zeros_like(AD)
    AD[:A1.shape[0], :A1.shape[1]], DP[:A1.shape[0], :A1.shape[1]] = A1, D1
    AD[A1.shape[0]:], DP[A1.shape[0]:] = A2, D2
    return AD, DP


@functools.lru_cache(maxsize=None)
def reference(K):
    """the restatement of every row of problem(), once per K"""
    AD, DP = problem()
    rows = []
    for v in range(AD.shape[0]):
        cols = np.flatnonzero(DP[v] > 0)
        n_cell = max(VN.N_CELL, cols.max() + 1 if cols.size else 0)          # uncovered cells add nothing
        r = VN.fit_row(AD[v, :n_cell], DP[v, :n_cell], K, **PARAMS)
        r["elbo_one"] = VN.elbo_one(AD[v], DP[v])
        rows.append(r)
    return rows


def worst(name, got, want, scale):
    err = np.max(np.abs(np.asarray(got) - np.asarray(want)) / scale) if np.size(want) else 0.0
    print("  %-10s worst error %.3g (bound %g)" % (name, err, TOL))
    return err


def compare(fit, ref, n_covered, check_iters=True):
    """the issue's checks of a device fit (with traces) against restatement rows"""
    n_it = np.array([r["n_iter"] for r in ref])
    warn = np.array([r["warn"] for r in ref])
    if check_iters:
        edges = [v for v, r in enumerate(ref) if VN.knife_edge(r["margins"], PARAMS["epsilon_conv"])]
        assert edges == [], "rows on a knife edge of the stop rule: change the seeds (%s)" % edges
        assert np.array_equal(fit["n_iter"], n_it), np.flatnonzero(fit["n_iter"] != n_it)
        assert np.array_equal(fit["warn"], warn)
    elbo = np.array([r["elbo"] for r in ref])
    one = np.array([r["elbo_one"] for r in ref])
    assert np.array_equal(fit["n_covered"], n_covered)
    errs = dict(
        elbo=worst("elbo", fit["elbo"], elbo, np.maximum(1.0, np.abs(elbo))),
        elbo_one=worst("elbo_one", fit["elbo_one"], one, np.maximum(1.0, np.abs(one))),
        gain=worst("gain", fit["gain"], elbo - one, np.maximum(1.0, np.abs(elbo))),
        beta_mu=worst("beta_mu", fit["beta_mu"], np.array([r["beta_mu"] for r in ref]), 1.0),
        beta_sum=worst("beta_sum", fit["beta_sum"], np.array([r["beta_sum"] for r in ref]),
                       np.maximum(1.0, np.array([r["beta_sum"] for r in ref]))),
        size=worst("size", fit["size"], np.array([r["size"] for r in ref]),
                   np.maximum(1, n_covered)[:, None].astype(float)))
    t_err = 0.0
    for v, r in enumerate(ref):
        assert fit["trace"][v].shape == r["trace"].shape, v
        t_err = max(t_err, np.max(np.abs(fit["trace"][v] - r["trace"]) / np.maximum(1.0, np.abs(r["trace"]))))
    print("  %-10s worst error %.3g (bound %g)" % ("trace", t_err, TOL))
    errs["trace"] = t_err
    for name, e in errs.items():
        assert e <= TOL, (name, e)
    return errs


@pytest.fixture(scope="module")
def mixtures(va):
    AD, DP = problem()
    return va.VariantMixtures(csr_matrix(AD), csr_matrix(DP))


@pytest.mark.parametrize("K", KS)
def test_parity(va, mixtures, K):
    AD, DP = problem()
    ref = reference(K)
    fit = mixtures.fit(n_clone=K, return_trace=True, **PARAMS)
    n_it = np.array([r["n_iter"] for r in ref])
    print("K = %d: %d rows, n_iter %d .. %d, kernel %.3f ms" % (K, len(ref), n_it.min(), n_it.max(),
                                                               mixtures.kernel_ms))
    compare(fit, ref, (DP > 0).sum(1))
    assert len(set(n_it.tolist())) > 3                                      # variants do stop at different iterations
    # empty rows: gain 0, the prior's beta_mu / beta_sum, nobody assigned
    for v in np.flatnonzero((DP > 0).sum(1) == 0):
        assert fit["gain"][v] == 0.0 and fit["elbo"][v] == 0.0 and fit["elbo_one"][v] == 0.0
        assert np.all(fit["beta_mu"][v] == 0.5) and np.all(fit["beta_sum"][v] == 2.0) and np.all(fit["size"][v] == 0.0)
        assert fit["n_iter"][v] == PARAMS["min_iter"] + 1


def test_golden(va):
    """the reference's own numbers (tests/golden/make_varmix_golden.py: BinomMixtureVB._fit_BV row by row)"""
    g = np.load(os.path.join(GOLD, "c1_varmix.npz"))
    AD, DP = g["AD"], g["DP"]
    kw = dict(max_iter=int(g["max_iter"]), min_iter=int(g["min_iter"]), epsilon_conv=float(g["epsilon_conv"]))
    vm = va.VariantMixtures(AD, DP)
    for K in g["Ks"]:
        K = int(K)
        fit = vm.fit(n_clone=K, return_trace=True, **kw)
        n_it = g["n_iter_K%d" % K]
        assert np.array_equal(fit["n_iter"], n_it)
        elbo = g["elbo_K%d" % K]
        scale = np.maximum(1.0, np.abs(elbo))
        assert worst("elbo", fit["elbo"], elbo, scale) <= TOL
        assert worst("elbo_one", fit["elbo_one"], g["elbo_one"], np.maximum(1.0, np.abs(g["elbo_one"]))) <= TOL
        assert worst("gain", fit["gain"], elbo - g["elbo_one"], scale) <= TOL
        assert worst("beta_mu", fit["beta_mu"], g["beta_mu_K%d" % K], 1.0) <= TOL
        assert worst("beta_sum", fit["beta_sum"], g["beta_sum_K%d" % K], np.maximum(1.0, g["beta_sum_K%d" % K])) <= TOL
        n_cov = (DP > 0).sum(1)
        unc = (DP.shape[1] - n_cov)[:, None] / K                            # ID_prob.sum(0) counts them as 1 / K
        assert worst("size", fit["size"], g["size_K%d" % K] - unc, np.maximum(1, n_cov)[:, None].astype(float)) <= TOL
        tr = g["trace_K%d" % K]
        for v in range(AD.shape[0]):
            want = tr[v, :n_it[v]]                                          # the reference keeps ELBO[:it]
            assert np.max(np.abs(fit["trace"][v][:-1] - want) / np.maximum(1.0, np.abs(want))) <= TOL


def test_special_rows(va):
    n = 120
    rng = np.random.default_rng(5)
    d = rng.poisson(20, n) + 1
    rows_a, rows_d = [], []
    rows_a.append(np.zeros(n, dtype=np.int64)); rows_d.append(d)            # noqa: E702  all reference
    rows_a.append(d.copy()); rows_d.append(d)                               # noqa: E702  all alternate
    one_a, one_d = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    one_a[17], one_d[17] = 3, 9
    rows_a.append(one_a); rows_d.append(one_d)                              # noqa: E702  one entry
    rows_a.append(np.zeros(n, dtype=np.int64)); rows_d.append(np.zeros(n, dtype=np.int64))   # noqa: E702  empty
    # one component empties: deep cells that are all reference or all alternate leave nothing to the middle
    # component of K = 3 -- its ID underflows to exactly 0 (the rel_entr(0, .) = 0 path) and its theta goes
    # back to the prior
    deep_d = rng.poisson(1500, n) + 1
    rows_a.append(np.where(np.arange(n) % 3 == 0, deep_d, 0)); rows_d.append(deep_d)   # noqa: E702
    p = np.where(rng.random(n) < 0.3, 0.4, 0.02)                            # still moving at max_iter = 4
    rows_a.append(rng.binomial(d, p)); rows_d.append(d)                     # noqa: E702
    AD, DP = np.array(rows_a), np.array(rows_d)
    vm = va.VariantMixtures(AD, DP)
    for K, kw in ((2, PARAMS), (3, PARAMS), (3, dict(max_iter=4, min_iter=0, epsilon_conv=1e-7)),
                  (2, dict(max_iter=4, min_iter=0, epsilon_conv=1e-7))):
        fit = vm.fit(n_clone=K, return_trace=True, **kw)
        ref = []
        for v in range(AD.shape[0]):
            r = VN.fit_row(AD[v], DP[v], K, **kw)
            r["elbo_one"] = VN.elbo_one(AD[v], DP[v])
            ref.append(r)
        n_it = np.array([r["n_iter"] for r in ref])
        assert not any(VN.knife_edge(r["margins"], kw["epsilon_conv"]) for r in ref)
        assert np.array_equal(fit["n_iter"], n_it) and np.array_equal(fit["warn"], [r["warn"] for r in ref])
        elbo = np.array([r["elbo"] for r in ref])
        assert worst("elbo", fit["elbo"], elbo, np.maximum(1.0, np.abs(elbo))) <= TOL
        assert worst("gain", fit["gain"], elbo - np.array([r["elbo_one"] for r in ref]),
                     np.maximum(1.0, np.abs(elbo))) <= TOL
        assert worst("beta_mu", fit["beta_mu"], np.array([r["beta_mu"] for r in ref]), 1.0) <= TOL
        assert worst("size", fit["size"], np.array([r["size"] for r in ref]),
                     np.maximum(1, (DP > 0).sum(1))[:, None].astype(float)) <= TOL
        if kw["max_iter"] == 4:
            assert fit["warn"][5] & 2 and fit["n_iter"][5] == 3
            assert fit["elbo"][5] == fit["trace"][5][2]                     # ELBO[it - 1] of it = max_iter - 1
        elif K == 3:
            assert ref[4]["size"][1] == 0.0 and np.all(ref[4]["ID_prob"][:, 1] == 0.0)     # (the input's property)
            assert fit["size"][4][1] == 0.0 and fit["beta_mu"][4][1] == 0.5 and fit["beta_sum"][4][1] == 2.0
        assert fit["gain"][3] == 0.0 and np.all(fit["size"][3] == 0.0)
        assert fit["gain"][0] < 0 and fit["gain"][1] < 0                    # pure rows: one component explains them


def fit_row_mp(ad, dp, K, max_iter, min_iter, epsilon_conv):
    """the protocol of varmix_np.fit_row on the covered cells at 40 digits -> (trace, it, elbo_one)"""
    import mpmath
    mpmath.mp.dps = 40
    mpf, psi = mpmath.mpf, mpmath.digamma
    cov = np.flatnonzero(dp > 0)
    a = [mpf(int(x)) for x in ad[cov]]
    d = [mpf(int(x)) for x in dp[cov]]
    b = [y - x for x, y in zip(a, d)]
    n = len(a)

    def beta_kl(s1, s2):
        d1, d2, ds = psi(s1), psi(s2), psi(s1 + s2)
        return -(mpmath.loggamma(s1) + mpmath.loggamma(s2) - mpmath.loggamma(s1 + s2)
                 - (s1 - 1) * d1 - (s2 - 1) * d2 + (s1 + s2 - 2) * ds)

    ID = []
    for x, y in zip(a, d):
        f = x / y
        w = [max(mpf(0), 1 - abs(f - mpf(k) / (K - 1)) * (K - 1)) + mpf(1) / 64 for k in range(K)]
        s = sum(w)
        ID.append([z / s for z in w])
    trace = []
    it = 0
    for it in range(max_iter):
        s1 = [1 + sum(a[i] * ID[i][k] for i in range(n)) for k in range(K)]
        s2 = [1 + sum(b[i] * ID[i][k] for i in range(n)) for k in range(K)]
        p1, p2, ps = [psi(x) for x in s1], [psi(x) for x in s2], [psi(x + y) for x, y in zip(s1, s2)]
        elbo = -sum(beta_kl(x, y) for x, y in zip(s1, s2))
        for i in range(n):
            L = [a[i] * p1[k] + b[i] * p2[k] - d[i] * ps[k] for k in range(K)]
            mx = max(L)
            e = [mpmath.exp(x - mx) for x in L]
            s = sum(e)
            ID[i] = [x / s for x in e]
            elbo += sum(x * y for x, y in zip(L, ID[i]))
            elbo -= sum(y * mpmath.log(y * K) for y in ID[i] if y > 0)
        trace.append(elbo)
        if it > min_iter:
            diff = trace[it] - trace[it - 1]
            if diff < -1e-6:
                pass
            elif it == max_iter - 1:
                pass
            elif diff < epsilon_conv:
                break
    ta, tb = sum(a), sum(b)
    s1, s2 = 1 + ta, 1 + tb
    one = ta * psi(s1) + tb * psi(s2) - (ta + tb) * psi(s1 + s2) - beta_kl(s1, s2)
    return trace, it, one


DEEP_HI = (0.02, 0.32, 0.31)          # a clear clone, and two whose levels overlap at depth 2000: slow fits


def test_deep_counts(va):
    """depth ~2000 (the class README "Known deviations" lists for clone mode): the arbiter is a 40-digit run of
    the same protocol; the device may be 1e-5 relative or twice as far from it as the float64 restatement"""
    import mpmath
    rng = np.random.default_rng(21)
    n, n_cell, K = 48, 64, 2
    AD = np.zeros((6, n_cell), dtype=np.int64)
    DP = np.zeros((6, n_cell), dtype=np.int64)
    for v in range(6):
        cells = np.sort(rng.choice(n_cell, n, replace=False))
        d = rng.poisson(2000, n) + 1
        p = np.where(rng.random(n) < 0.4, DEEP_HI[v // 2], 0.30) if v % 2 == 0 else np.full(n, (0.05, 0.5, 0.2)[v // 2])
        DP[v, cells] = d
        AD[v, cells] = rng.binomial(d, p)
    fit = va.variant_mixture_gain(AD, DP, n_clone=K, return_fit=True, **PARAMS)
    for v in range(6):
        r = VN.fit_row(AD[v], DP[v], K, **PARAMS)
        tr, it, one = fit_row_mp(AD[v], DP[v], K, **PARAMS)
        assert it == r["n_iter"], "row %d: float64 and 40 digits stop at %d / %d: replace the row" % (v, r["n_iter"], it)
        assert fit["n_iter"][v] == it
        exact = dict(elbo=tr[it - 1], elbo_one=one, gain=tr[it - 1] - one)
        np64 = dict(elbo=r["elbo"], elbo_one=VN.elbo_one(AD[v], DP[v]))
        np64["gain"] = np64["elbo"] - np64["elbo_one"]
        scale = float(max(1, abs(exact["elbo"])))
        for name in ("elbo", "elbo_one", "gain"):
            sc = scale if name != "elbo_one" else float(max(1, abs(one)))
            e_dev = float(abs(mpmath.mpf(float(fit[name][v])) - exact[name])) / sc
            e_np = float(abs(mpmath.mpf(float(np64[name])) - exact[name])) / sc
            print("  row %d %-8s = %.6f: device error %.3g, float64 restatement %.3g" % (v, name, float(exact[name]),
                                                                                     e_dev, e_np))
            assert e_dev <= max(TOL, 2.0 * e_np), (v, name, e_dev, e_np)


def _bits(fit, rows=None):
    keys = ("gain", "elbo", "elbo_one", "beta_mu", "beta_sum", "size", "n_iter", "warn")
    return {k: (fit[k] if rows is None else fit[k][rows]).tobytes() for k in keys}


def test_independence(va, mixtures):
    """a row's results are a function of the row: the call, the order and the run do not matter"""
    AD, DP = problem()
    K = 3
    full = mixtures.fit(n_clone=K, **PARAMS)
    assert _bits(mixtures.fit(n_clone=K, **PARAMS)) == _bits(full)          # two runs
    other = mixtures.fit(n_clone=2, **PARAMS)
    assert _bits(mixtures.fit(n_clone=K, **PARAMS)) == _bits(full)          # K = 3, 2, then 3 again
    assert _bits(other) == _bits(mixtures.fit(n_clone=2, **PARAMS))
    n = AD.shape[0]
    rev = va.VariantMixtures(AD[::-1], DP[::-1]).fit(n_clone=K, **PARAMS)
    assert _bits(rev, np.arange(n)[::-1]) == _bits(full)
    sub = np.arange(1, n, 3)
    part = va.VariantMixtures(AD[sub], DP[sub]).fit(n_clone=K, **PARAMS)
    assert _bits(part) == _bits(full, sub)
    A, D = csr_matrix(AD), csr_matrix(DP)
    for v in range(n):                                                      # every row alone
        single = va.VariantMixtures(A[v], D[v]).fit(n_clone=K, **PARAMS)
        assert _bits(single) == _bits(full, slice(v, v + 1)), v


def test_public_path(va):
    AD, DP = VN.gen_rows([5, 40, 0, 130, 299, 64] * 3, seed=31)
    kw = dict(n_clone=2, **PARAMS)
    base = va.variant_mixture_gain(csc_matrix(AD), csc_matrix(DP), return_fit=True, **kw)
    for conv in (csr_matrix, np.asarray, lambda X: np.asarray(X, dtype=np.float64),
                 lambda X: csc_matrix(X.astype(np.float64)), lambda X: csr_matrix(X).tocoo()):
        got = va.variant_mixture_gain(conv(AD), conv(DP), return_fit=True, **kw)
        assert _bits(got) == _bits(base)
    assert va.variant_mixture_gain(AD, DP, **kw).tobytes() == base["gain"].tobytes()
    shallow = DP < 5
    AD5, DP5 = np.where(shallow, 0, AD), np.where(shallow, 0, DP)
    a = va.variant_mixture_gain(AD, DP, min_DP=5, return_fit=True, **kw)
    b = va.variant_mixture_gain(AD5, DP5, return_fit=True, **kw)
    assert _bits(a) == _bits(b) and np.array_equal(a["n_covered"], (DP5 > 0).sum(1))
    # no variants, no entries
    empty = va.variant_mixture_gain(np.zeros((0, 7), dtype=int), np.zeros((0, 7), dtype=int), **kw)
    assert empty.shape == (0,)
    assert np.all(va.variant_mixture_gain(np.zeros((3, 7), dtype=int), np.zeros((3, 7), dtype=int), **kw) == 0.0)


def test_library_refuses_unsupported(va):
    """the library itself refuses what the Python layer checks first: VRX_ERR_UNSUPPORTED"""
    import ctypes as C
    from vireo_amd import _lib
    AD, DP = VN.gen_rows([5, 40], seed=32)
    vm = va.VariantMixtures(AD, DP)
    n = vm.n_var
    e, o = np.zeros(n), np.zeros(n)
    it, wn = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    i32 = C.POINTER(C.c_int32)
    for n_clone, max_iter in ((9, 10), (1, 10), (2, 1)):
        rc = _lib.lib().vrx_varmix_fit(vm._h, n_clone, max_iter, 0, 1e-2, _lib.dptr(e), _lib.dptr(o), None, None,
                                       None, it.ctypes.data_as(i32), wn.ctypes.data_as(i32), None, None)
        assert rc == -4 and b"vrx_varmix_fit" in _lib.lib().vrx_last_error()
    with pytest.raises(ValueError):
        vm.fit(n_clone=9)


def test_command(va, tmp_path):
    from vireo_amd.io_utils import read_cellSNP, read_mtx
    data = os.path.join(GOLD, "data", "cellSNP_mat")
    dat = read_cellSNP(data)
    AD, DP = csr_matrix(dat["AD"]), csr_matrix(dat["DP"])
    names = [str(x) for x in dat["variants"]]
    gain = va.variant_mixture_gain(AD, DP, n_clone=2)
    out = str(tmp_path / "o")
    r = subprocess.run([sys.executable, "-m", "vireo_amd.variant_gain", "-c", data, "-o", out, "-K", "2"],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "[variant_gain]" in r.stdout and "of %d variants" % len(names) in r.stdout
    lines = open(os.path.join(out, "variant_gain.tsv")).read().splitlines()
    assert lines[0].split("\t")[:6] == ["variant", "n_covered", "gain", "elbo_one", "elbo", "n_iter"]
    assert len(lines) == 1 + len(names)
    assert [l.split("\t")[0] for l in lines[1:]] == names
    assert np.array_equal(np.array([float(l.split("\t")[2]) for l in lines[1:]]), gain)
    rows = np.flatnonzero(gain > 0)
    assert 0 < rows.size < len(names)
    for name, X in (("passed_ad.mtx", AD), ("passed_dp.mtx", DP)):
        got = read_mtx(os.path.join(out, name)).tocsr()
        assert got.shape == (rows.size, X.shape[1]) and (got != X[rows]).nnz == 0
    assert open(os.path.join(out, "passed_variant_names.txt")).read().split("\n")[:-1] == [names[v] for v in rows]
    # a threshold above every gain: empty but valid files
    out2 = str(tmp_path / "none")
    r = subprocess.run([sys.executable, "-m", "vireo_amd.variant_gain", "-c", data, "-o", out2, "--minGain",
                        repr(float(gain.max()) + 1.0)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    for name in ("passed_ad.mtx", "passed_dp.mtx"):
        got = read_mtx(os.path.join(out2, name))
        assert got.shape == (0, AD.shape[1]) and got.nnz == 0
    assert open(os.path.join(out2, "passed_variant_names.txt")).read() == ""
    assert len(open(os.path.join(out2, "variant_gain.tsv")).read().splitlines()) == 1 + len(names)
