"""Donor matching without a GPU: the fixture's own conditions, the host logic of match_VCF_samples with
the distance matrix from the NumPy formula, the argument checks that run before any device call, and
the error a compute call gives when there is no GPU."""
import contextlib
import io

import numpy as np
import pytest

from tests import gold
from tests import match_np as M

CASE_IDS = range(1, len(M.CASES) + 1)


@pytest.fixture(scope="module")
def fixture():
    return gold.load("c1_donor_match")


def numpy_distance(X, Z=None, axis=1, block_vars=None):
    from vireo_amd.vireo_base import _canonical_genotypes
    Xc = _canonical_genotypes(X, axis, "X")
    return M.distance_np(Xc, Xc if Z is None else _canonical_genotypes(Z, axis, "Z"))


@pytest.mark.parametrize("k", CASE_IDS)
def test_fixture_sizes_and_margin(fixture, k):
    c = M.fixture_case(fixture, k)
    assert c["full_GPb_diff"].shape == M.SHAPES[k - 1]
    assert int(c["matched_n_var"]) == M.N_MATCHED[k - 1]
    n = min(M.SHAPES[k - 1])
    assert c["matched_GPb_diff"].shape == (n, n)
    assert len(c["matched_donors1"]) == len(c["matched_donors2"]) == n
    assert (len(c["full_donors1"]), len(c["full_donors2"])) == M.SHAPES[k - 1]
    margin = M.assignment_margin(c["full_GPb_diff"])
    assert margin == float(c["margin"]) and margin >= 1e-6


def test_fixture_case1_is_the_notebook(fixture):
    c = M.fixture_case(fixture, 1)
    assert np.array_equal(np.round(c["full_GPb_diff"], 8), M.NOTEBOOK_DIFF)
    assert list(c["matched_donors1"]) == ["MantonCB1", "MantonCB2", "MantonCB3", "MantonCB4"]
    assert list(c["matched_donors2"]) == ["donor2", "donor1", "donor3", "donor0"]


@pytest.mark.parametrize("k", CASE_IDS)
def test_match_VCF_samples_host_logic(fixture, k, monkeypatch):
    """prints, keys, variant matching (case 1, 2, 4: one id differs by more than the chr prefix) and the
    rectangular cases equal the reference's, with the distance from the NumPy formula"""
    import vireo_amd
    from vireo_amd import vireo_base
    monkeypatch.setattr(vireo_base, "genotype_distance", numpy_distance)
    c = M.fixture_case(fixture, k)
    vcf1, vcf2, tag1, tag2 = M.case_paths(k)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        rv = vireo_amd.vcf.match_VCF_samples(vcf1, vcf2, tag1, tag2)
    assert out.getvalue().splitlines() == str(c["stdout"]).splitlines()
    assert len(out.getvalue().splitlines()) == 6
    assert sorted(rv) == sorted(M.KEYS)
    assert rv["matched_n_var"] == int(c["matched_n_var"])
    for key in ("matched_donors1", "matched_donors2", "full_donors1", "full_donors2"):
        assert list(rv[key]) == list(c[key]), key
    n = M.N_MATCHED[k - 1] * M.N_GT
    M.assert_within_bound(rv["full_GPb_diff"], c["full_GPb_diff"], n)
    M.assert_within_bound(rv["matched_GPb_diff"], c["matched_GPb_diff"], n)


def test_package_surface():
    import vireo_amd
    for name in ("genotype_distance", "donor_match", "match_VCF_samples"):
        assert hasattr(vireo_amd, name) and name in vireo_amd.__all__
    assert vireo_amd.vcf.match_VCF_samples is vireo_amd.match_VCF_samples
    assert vireo_amd.base.genotype_distance is vireo_amd.genotype_distance
    from vireo_amd import _lib
    assert "vrx_geno_dist" in _lib.SIGNATURES


def test_donor_match_is_optimal_match_on_the_same_matrix(monkeypatch):
    from vireo_amd import vireo_base
    monkeypatch.setattr(vireo_base, "genotype_distance", numpy_distance)
    X, Z = M.matched_tensors(3)
    i0, i1, d = vireo_base.donor_match(X, Z, return_delta=True)
    j0, j1, e = vireo_base.optimal_match(X, Z, return_delta=True)
    assert np.array_equal(i0, j0) and np.array_equal(i1, j1) and np.array_equal(d, e)
    assert len(vireo_base.donor_match(X, Z)) == 2


def test_argument_errors_and_empty_input_before_any_device_call(monkeypatch):
    from vireo_amd import _lib, genotype_distance

    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(_lib, "lib", no_device)
    monkeypatch.setattr(_lib, "require_gpu", no_device)
    X = np.random.RandomState(0).rand(6, 3, 3)
    bad = [
        dict(X=X, Z=X[:5]),                       # n_var differs
        dict(X=X, Z=X[:, :, :2]),                 # n_gt differs
        dict(X=X, Z=X[:, :, 0]),                  # 2-D against 3-D
        dict(X=X[0, 0]),                          # 1-D
        dict(X=X[None]),                          # 4-D
        dict(X=X, axis=3),
        dict(X=X.astype(str)),
        dict(X=X.astype(complex)),
        dict(X=X[:, :0]),                         # no donor
        dict(X=np.zeros((2, 2, 65))),             # too many genotype classes
        dict(X=X, block_vars=-1),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            genotype_distance(**kw)
    D = genotype_distance(np.zeros((0, 2, 3)), np.zeros((0, 5, 3)))
    assert D.shape == (2, 5) and np.isnan(D).all()
    assert genotype_distance(np.zeros((0, 4))).shape == (4, 4)


def test_no_gpu_no_fallback():
    """where no GPU is visible a compute call raises; it never computes on the host"""
    from vireo_amd import _lib, genotype_distance, donor_match
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible here")
    X = np.random.RandomState(0).rand(6, 3, 3)
    with pytest.raises(_lib.VrxError):
        genotype_distance(X)
    with pytest.raises(_lib.VrxError):
        donor_match(X, X)
