"""What the donor-matching tests share: the fixture's cases, the NumPy formula of the genotype distance,
the derived tolerance and the assignment margin."""
import contextlib
import io
import itertools
import os

import numpy as np

from tests import gold

# (VCF1, VCF2, GT_tag1, GT_tag2), paths under tests/golden/
CASES = [
    ("data/donors.cellSNP.vcf.gz", "cli/mode1_noGT/GT_donors.vireo.vcf.gz", "PL", "PL"),
    ("data/donors.cellSNP.vcf.gz", "cli/mode1_noGT/GT_donors.vireo.vcf.gz", "GT", "GT"),
    ("data/donors.two.cellSNP.vcf.gz", "cli/mode1_noGT/GT_donors.vireo.vcf.gz", "GT", "PL"),
    ("cli/extraDonor/GT_donors.vireo.vcf.gz", "data/donors.cellSNP.vcf.gz", "PL", "GT"),
    ("cli/mode1_noGT/GT_donors.vireo.vcf.gz", "cli/cellRange/GT_donors.vireo.vcf.gz", "PL", "PL"),
]
SHAPES = [(4, 4), (4, 4), (2, 4), (3, 4), (4, 4)]
N_MATCHED = [3783, 3783, 3784, 3783, 3784]
KEYS = ("matched_GPb_diff", "matched_donors1", "matched_donors2", "full_GPb_diff", "full_donors1",
        "full_donors2", "matched_n_var")
N_GT = 3
# the matrix the reference's examples/donor_match.ipynb prints for case 1
NOTEBOOK_DIFF = np.array([[0.43964819, 0.44643109, 0.14587468, 0.43192166],
                          [0.41247473, 0.18310327, 0.43770159, 0.42725593],
                          [0.42989822, 0.41561379, 0.42926244, 0.21593441],
                          [0.22427656, 0.40927258, 0.43158556, 0.42760225]])


def case_paths(k):
    vcf1, vcf2, tag1, tag2 = CASES[k - 1]
    return os.path.join(gold.GOLD, vcf1), os.path.join(gold.GOLD, vcf2), tag1, tag2


def fixture_case(g, k):
    return {key: g["c%d_%s" % (k, key)] for key in KEYS + ("stdout", "margin")}


def distance_np(X, Z):
    """the reference's double loop (vireo_base.py:197-201) on canonical (n_var, K, n_gt) operands"""
    D = np.zeros((X.shape[1], Z.shape[1]))
    for i in range(X.shape[1]):
        for j in range(Z.shape[1]):
            D[i, j] = np.mean(np.abs(X[:, i] - Z[:, j]))
    return D


def bound(D_ref, n):
    """|D - D_ref| allowed for sums of n = n_var * n_gt correctly rounded non-negative terms in two
    different orders: each is within (n - 1) u of the exact sum, relatively"""
    return 2 * n * 2.0 ** -53 * D_ref


def assert_within_bound(D, D_ref, n):
    """every cell: NaN where the reference is NaN, exactly 0 where it is 0, else within the bound (no
    absolute slack)"""
    D, D_ref = np.asarray(D), np.asarray(D_ref)
    assert D.shape == D_ref.shape, (D.shape, D_ref.shape)
    nan = np.isnan(D_ref)
    assert np.array_equal(np.isnan(D), nan)
    err = np.abs(np.where(nan, 0.0, D) - np.where(nan, 0.0, D_ref))
    lim = np.where(nan, 0.0, bound(D_ref, n))
    worst = float(np.max(err / np.where(lim > 0, lim, 1.0))) if err.size else 0.0
    assert np.all(err <= lim), "worst error is %.3g of the bound (n = %d)" % (worst, n)


def assignment_margin(D):
    """cost of the second-best assignment minus the cost of the best one, by brute force: every way to
    give each slice of the shorter side a different slice of the longer one"""
    D = np.asarray(D)
    if D.shape[0] > D.shape[1]:
        D = D.T
    rows = np.arange(D.shape[0])
    costs = sorted(D[rows, list(p)].sum() for p in itertools.permutations(range(D.shape[1]), D.shape[0]))
    return costs[1] - costs[0]


def matched_tensors(k):
    """the two genotype tensors of case k restricted to their common variants, through this package's
    loaders (what match_VCF_samples hands to donor_match)"""
    from vireo_amd.vcf_utils import load_VCF, match_SNPs, parse_donor_GPb
    vcf1, vcf2, tag1, tag2 = case_paths(k)
    with contextlib.redirect_stdout(io.StringIO()):
        d1 = load_VCF(vcf1, biallelic_only=True, sparse=False, format_list=[tag1])
        d2 = load_VCF(vcf2, biallelic_only=True, sparse=False, format_list=[tag2])
    P1 = parse_donor_GPb(d1["GenoINFO"][tag1], tag1)
    P2 = parse_donor_GPb(d2["GenoINFO"][tag2], tag2)
    found = match_SNPs(np.array(d2["variants"]), np.array(d1["variants"]))
    use2 = np.where(found != None)[0]                              # noqa: E711
    return P1[found[use2].astype(int)], P2[use2]
