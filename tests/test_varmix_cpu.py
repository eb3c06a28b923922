"""CPU-only: the contract of variant_mixture_gain (tests/varmix_np.py) IS the reference's -- equal, bit for bit,
to oracle.vireo_oracle's BinomMixtureVB on one row and to the real reference's numbers in
tests/golden/c1_varmix.npz -- and the argument checks of the public path, which run before any launch."""
import os

import numpy as np
import pytest
from scipy.sparse import csc_matrix

import __graft_entry__ as entry
from oracle import vireo_oracle as O
from tests import varmix_np as VN

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KW = dict(max_iter=60, min_iter=2, epsilon_conv=1e-2)
LENGTHS = [300, 299, 257, 256, 129, 128, 127, 65, 64, 63, 2, 1, 0, 200, 150, 100, 80, 60, 40, 30,
           20, 10, 5, 3, 280, 240, 210, 170, 130, 110, 90, 70, 50, 35, 25, 15, 8, 4, 300, 1]


@pytest.fixture(scope="module", autouse=True)
def built():
    entry.build()


@pytest.fixture(scope="module")
def rows():
    return VN.gen_rows(LENGTHS, seed=7)


@pytest.mark.parametrize("K", [2, 3, 5])
def test_restatement_is_the_oracle(rows, K):
    AD, DP = rows
    n_cell = AD.shape[1]
    its = []
    for v in range(AD.shape[0]):
        a, d = AD[v:v + 1].astype(np.float64), DP[v:v + 1].astype(np.float64)
        st = O.bmm_new(n_cell, 1, K, ID_prob_init=VN.id_init(AD[v], DP[v], K))
        it = O.bmm_fit_vb(st, a, d, **KW)
        r = VN.fit_row(AD[v], DP[v], K, **KW)
        assert r["n_iter"] == it and it >= 1
        assert np.array_equal(r["trace"][:-1], st.ELBO_iters)                 # the reference keeps ELBO[:it]
        assert r["elbo"] == st.ELBO_iters[-1]
        assert np.array_equal(r["beta_mu"], st.beta_mu[0]) and np.array_equal(r["beta_sum"], st.beta_sum[0])
        assert np.array_equal(r["ID_prob"], st.ID_prob)
        # size counts covered cells only: ID_prob.sum(0) exceeds it by the uncovered cells' 1 / K each
        n_unc = int(np.sum(DP[v] == 0))
        assert np.all(st.ID_prob[DP[v] == 0] == 1.0 / K)
        np.testing.assert_allclose(st.ID_prob.sum(0) - r["size"], n_unc / K, rtol=0, atol=1e-10)
        assert r["warn"] == 0
        its.append(it)
    assert min(its) == 3 and max(its) > 10                                    # variants stop at different iterations


def test_uncovered_cells_add_nothing(rows):
    """the same row with its uncovered cells removed: identical trace up to the order of the sums"""
    AD, DP = rows
    for v in (0, 5, 13, 20):
        cov = DP[v] > 0
        full = VN.fit_row(AD[v], DP[v], 3, **KW)
        only = VN.fit_row(AD[v][cov], DP[v][cov], 3, **KW)
        assert full["n_iter"] == only["n_iter"]
        np.testing.assert_allclose(full["trace"], only["trace"], rtol=1e-12, atol=1e-9)
        np.testing.assert_allclose(full["size"], only["size"], rtol=0, atol=1e-9)


def test_one_component_is_the_closed_form(rows):
    AD, DP = rows
    n_cell = AD.shape[1]
    for v in range(AD.shape[0]):
        a, d = AD[v:v + 1].astype(np.float64), DP[v:v + 1].astype(np.float64)
        st = O.bmm_new(n_cell, 1, 1)
        it = O.bmm_fit_vb(st, a, d, **KW)
        assert it == KW["min_iter"] + 1 and np.all(st.ID_prob == 1.0)
        assert np.all(st.ELBO_iters == VN.elbo_one(AD[v], DP[v]))             # at every iteration
    assert VN.elbo_one(AD[12], DP[12]) == 0.0 and not np.any(DP[12])          # the empty row


def test_golden_is_reproduced():
    """the real reference's BinomMixtureVB._fit_BV, row by row (tests/golden/make_varmix_golden.py)"""
    g = np.load(os.path.join(GOLD, "c1_varmix.npz"))
    assert all(g[k].dtype.kind in "if" for k in g.files)                      # numeric arrays only
    AD, DP = g["AD"].astype(np.int64), g["DP"].astype(np.int64)
    kw = dict(max_iter=int(g["max_iter"]), min_iter=int(g["min_iter"]), epsilon_conv=float(g["epsilon_conv"]))
    for K in g["Ks"]:
        K = int(K)
        for v in range(AD.shape[0]):
            r = VN.fit_row(AD[v], DP[v], K, **kw)
            n = g["n_iter_K%d" % K][v]
            assert r["n_iter"] == n
            assert np.array_equal(r["trace"][:-1], g["trace_K%d" % K][v, :n]) and r["elbo"] == g["elbo_K%d" % K][v]
            assert np.array_equal(r["beta_mu"], g["beta_mu_K%d" % K][v])
            assert np.array_equal(r["beta_sum"], g["beta_sum_K%d" % K][v])
            assert np.array_equal(r["ID_prob"].sum(0), g["size_K%d" % K][v])
    for v in range(AD.shape[0]):
        assert VN.elbo_one(AD[v], DP[v]) == g["elbo_one"][v]


def test_probe_of_the_score():
    """what the score is for: a planted clone gains, noise and pure rows do not, an empty row gives 0"""
    rng = np.random.default_rng(3)
    n = 300
    d = rng.poisson(20, n) + 1
    planted = rng.binomial(d, np.where(rng.random(n) < 0.3, 0.30, 0.02))
    kw = dict(max_iter=200, min_iter=20, epsilon_conv=1e-2)

    def gain(a, dd):
        return VN.fit_row(a, dd, 2, **kw)["elbo"] - VN.elbo_one(a, dd)
    assert gain(planted, d) > 50
    assert gain(rng.binomial(d, 0.05), d) < 0 and gain(rng.binomial(d, 0.5), d) < 0
    assert gain(np.zeros(n, dtype=np.int64), d) < 0 and gain(d, d) < 0
    assert gain(np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)) == 0.0


def test_covered_csr_and_argument_checks(rows):
    import vireo_amd
    from vireo_amd.variant_mixture import covered_csr
    AD, DP = rows
    (n_var, n_cell), rowptr, cell, ad, dp = covered_csr(csc_matrix(AD), csc_matrix(DP))
    assert (n_var, n_cell) == AD.shape and np.array_equal(np.diff(rowptr), (DP > 0).sum(1))
    r, c = np.nonzero(DP)
    assert np.array_equal(cell, c) and np.array_equal(ad, AD[r, c]) and np.array_equal(dp, DP[r, c])
    got5 = covered_csr(AD.astype(np.float64), DP.astype(np.float64), min_DP=5)
    r, c = np.nonzero(DP >= 5)
    assert np.array_equal(np.diff(got5[1]), (DP >= 5).sum(1)) and np.array_equal(got5[4], DP[r, c])
    # all of these fail before any launch (there is no GPU here)
    bad = AD.copy()
    bad[3, np.flatnonzero(DP[3])[0]] = DP[3].max() + 1
    with pytest.raises(ValueError, match="AD > DP"):
        vireo_amd.variant_mixture_gain(bad, DP)
    bad = AD.copy()
    bad[0, 0] = -1
    with pytest.raises(ValueError):
        vireo_amd.variant_mixture_gain(bad, DP)
    with pytest.raises(ValueError):
        vireo_amd.variant_mixture_gain(AD, -DP)
    with pytest.raises(ValueError):
        vireo_amd.variant_mixture_gain(AD + 0.5, DP.astype(np.float64))
    for kw in (dict(n_clone=1), dict(n_clone=9), dict(max_iter=1), dict(min_iter=-1)):
        with pytest.raises(ValueError):
            vireo_amd.variant_mixture_gain(AD, DP, **kw)
    with pytest.raises(ValueError):
        vireo_amd.variant_mixture_gain(AD, DP[:, :-1])


def test_library_validates_the_csr():
    """vrx_varmix_create checks its operand before it touches a device"""
    import ctypes as C
    from vireo_amd import _lib
    L = _lib.lib()
    i32, i64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64)

    def create(rowptr, ad, dp):
        rowptr, ad, dp = np.array(rowptr, np.int64), np.array(ad, np.int32), np.array(dp, np.int32)
        h = C.c_void_p()
        rc = L.vrx_varmix_create(0, rowptr.size - 1, ad.size, rowptr.ctypes.data_as(i64), ad.ctypes.data_as(i32),
                                 dp.ctypes.data_as(i32), C.byref(h))
        return rc, L.vrx_last_error().decode()
    for rowptr, ad, dp, what in (([0, 2, 1, 3], [1, 1, 1], [2, 2, 2], "rowptr"), ([0, 1, 2], [1, 1, 1], [2, 2, 2], "rowptr"),
                                 ([1, 2, 3], [1, 1, 1], [2, 2, 2], "rowptr"), ([0, 1, 3], [1, 3, 1], [2, 2, 2], "ad ="),
                                 ([0, 1, 3], [1, -1, 1], [2, 2, 2], "ad ="), ([0, 1, 3], [0, 0, 0], [2, 0, 2], "dp =")):
        rc, msg = create(rowptr, ad, dp)
        assert rc == -1 and what in msg, (rc, msg)
    assert int(L.vrx_varmix_wave_rows()) >= 128
    assert L.vrx_varmix_fit(None, 2, 10, 0, 1e-2, None, None, None, None, None, None, None, None, None) == -1
