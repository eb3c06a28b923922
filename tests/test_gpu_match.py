"""Donor matching on the GPU: match_VCF_samples against the reference's fixture, and the device
genotype-distance pass (vrx_geno_dist) against the NumPy formula np.mean(np.abs(X[:, i] - Z[:, j])).

Tolerance (derived, tests/match_np.py): both sides add the same correctly rounded non-negative terms
|x - z| in different orders; any order of n = n_var * n_gt such terms is within (n - 1) u of the exact
sum, u = 2^-53, so |D_gpu - D_ref| <= 2 n u D_ref, with no absolute slack: where D_ref is 0 the result
is exactly 0."""
import contextlib
import io

import numpy as np
import pytest

from tests import gold
from tests import match_np as M

pytestmark = pytest.mark.gpu

PAIRS = [(1, 1), (1, 5), (4, 4), (3, 17), (16, 16), (15, 33), (17, 64), (65, 130)]
N_GTS = [1, 2, 3, 5]
N_VARS = [1, 2, 3, 255, 257, 4097]


def dirichlet(seed, n_var, k, n_gt):
    return np.random.RandomState(seed).dirichlet(np.ones(n_gt), size=(n_var, k))


@pytest.fixture(scope="module")
def fixture():
    return gold.load("c1_donor_match")


@pytest.fixture(scope="module")
def pool16():
    """3 783 variants x 16 donors on each side and the formula's matrix"""
    X, Z = dirichlet(1, 3783, 16, 3), dirichlet(2, 3783, 16, 3)
    return X, Z, M.distance_np(X, Z)


@pytest.mark.parametrize("k", range(1, len(M.CASES) + 1))
def test_golden_match_VCF_samples(fixture, k):
    import vireo_amd
    c = M.fixture_case(fixture, k)
    vcf1, vcf2, tag1, tag2 = M.case_paths(k)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        rv = vireo_amd.vcf.match_VCF_samples(vcf1, vcf2, tag1, tag2)
    n = M.N_MATCHED[k - 1] * M.N_GT
    M.assert_within_bound(rv["full_GPb_diff"], c["full_GPb_diff"], n)
    M.assert_within_bound(rv["matched_GPb_diff"], c["matched_GPb_diff"], n)
    for key in ("matched_donors1", "matched_donors2", "full_donors1", "full_donors2"):
        assert np.array_equal(np.asarray(rv[key], dtype=str), c[key]), key
    assert rv["matched_n_var"] == int(c["matched_n_var"])
    assert out.getvalue().splitlines() == str(c["stdout"]).splitlines()


@pytest.mark.parametrize("n_gt", N_GTS)
@pytest.mark.parametrize("k1,k2", PAIRS)
def test_shape_sweep(k1, k2, n_gt):
    from vireo_amd import genotype_distance
    for n_var in N_VARS:
        X, Z = dirichlet(10 + n_var, n_var, k1, n_gt), dirichlet(20 + n_var, n_var, k2, n_gt)
        D = genotype_distance(X, Z)
        M.assert_within_bound(D, M.distance_np(X, Z), n_var * n_gt)      # every cell


@pytest.mark.parametrize("block_vars", [1, 2, 1000, 3783, 10**9])
def test_slabs(pool16, block_vars):
    from vireo_amd import genotype_distance
    X, Z, ref = pool16
    M.assert_within_bound(genotype_distance(X, Z, block_vars=block_vars), ref, 3783 * 3)


@pytest.mark.parametrize("block_vars", [None, 4096])
def test_slabs_many_variants(block_vars):
    from vireo_amd import genotype_distance
    n_var = 160001
    X, Z = dirichlet(3, n_var, 4, 3), dirichlet(4, n_var, 7, 3)
    M.assert_within_bound(genotype_distance(X, Z, block_vars=block_vars), M.distance_np(X, Z), n_var * 3)


def test_determinism(pool16):
    from vireo_amd import genotype_distance
    X, Z, _ = pool16
    assert np.array_equal(genotype_distance(X, Z), genotype_distance(X, Z))
    assert np.array_equal(genotype_distance(X, Z, block_vars=500), genotype_distance(X, Z, block_vars=500))


def test_self_distance(pool16):
    from vireo_amd import genotype_distance
    X = pool16[0]
    D = genotype_distance(X)
    assert np.array_equal(np.diag(D), np.zeros(16))
    assert np.array_equal(D, genotype_distance(X, X.copy()))
    ref = M.distance_np(X, X)
    M.assert_within_bound(D, ref, 3783 * 3)
    assert np.all(np.abs(D - D.T) <= M.bound(ref, 3783 * 3))


def test_nan_stays_in_its_row_or_column(pool16):
    from vireo_amd import genotype_distance
    X, Z, ref = pool16
    Xn = X.copy()
    Xn[1234, 5, 2] = np.nan
    want = ref.copy()
    want[5, :] = np.nan
    M.assert_within_bound(genotype_distance(Xn, Z), want, 3783 * 3)
    Zn = Z.copy()
    Zn[77, 11, 0] = np.nan
    want = ref.copy()
    want[:, 11] = np.nan
    M.assert_within_bound(genotype_distance(X, Zn), want, 3783 * 3)


def test_layouts():
    from vireo_amd import genotype_distance
    X, Z = dirichlet(5, 301, 6, 3), dirichlet(6, 301, 9, 3)
    D = genotype_distance(X, Z)
    M.assert_within_bound(D, M.distance_np(X, Z), 301 * 3)
    # donors along axis 0 / axis 2 of a 3-D input
    for axis in (0, 2):
        Xa, Za = np.ascontiguousarray(np.moveaxis(X, 1, axis)), np.ascontiguousarray(np.moveaxis(Z, 1, axis))
        Da = genotype_distance(Xa, Za, axis=axis)
        assert np.array_equal(Da, genotype_distance(np.moveaxis(Xa, axis, 1), np.moveaxis(Za, axis, 1)))
        assert np.array_equal(Da, D)                      # (D is held to the formula above)
    assert np.array_equal(genotype_distance(np.moveaxis(X, 1, 0), np.moveaxis(Z, 1, 0), axis=0), D)
    # 2-D: one genotype class
    X2, Z2 = X[:, :, 0], Z[:, :, 0]
    D2 = genotype_distance(X2, Z2)
    assert np.array_equal(D2, genotype_distance(X2[:, :, None], Z2[:, :, None]))
    M.assert_within_bound(D2, M.distance_np(X2[:, :, None], Z2[:, :, None]), 301)
    assert np.array_equal(genotype_distance(X2.T, Z2.T, axis=0), D2)
    # float32 and Fortran order are converted
    X32, Z32 = X.astype(np.float32), Z.astype(np.float32)
    assert np.array_equal(genotype_distance(X32, Z32), genotype_distance(X32.astype(np.float64), Z32.astype(np.float64)))
    assert np.array_equal(genotype_distance(np.asfortranarray(X), np.asfortranarray(Z)), D)
    # no variants; mismatched shapes
    E = genotype_distance(X[:0], Z[:0])
    assert E.shape == (6, 9) and np.isnan(E).all()
    with pytest.raises(ValueError):
        genotype_distance(X, Z[:300])
    with pytest.raises(ValueError):
        genotype_distance(X, Z[:, :, :2])


@pytest.mark.parametrize("k", range(1, len(M.CASES) + 1))
def test_donor_match_equals_optimal_match(k):
    from vireo_amd import donor_match, optimal_match
    X, Z = M.matched_tensors(k)
    assert X.shape[0] == M.N_MATCHED[k - 1]
    i0, i1, d = donor_match(X, Z, return_delta=True)
    j0, j1, e = optimal_match(X, Z, return_delta=True)
    assert np.array_equal(i0, j0) and np.array_equal(i1, j1)
    M.assert_within_bound(d, e, X.shape[0] * X.shape[2])
    a0, a1 = donor_match(X, Z)
    assert np.array_equal(a0, j0) and np.array_equal(a1, j1)
