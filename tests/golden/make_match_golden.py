"""Donor-matching fixture from the REAL reference (build container only, /root/reference):

    python tests/golden/make_match_golden.py

  c1_donor_match.npz   vireoSNP.vcf.match_VCF_samples on five pairs of VCFs already committed under
                       tests/golden/ (tests/match_np.py lists them): per case `c<k>_` + the seven keys of
                       the returned dict (donor names as unicode arrays), the captured stdout, and
                       margin = cost of the second-best assignment - cost of the best one

Every case must have margin >= 1e-6 (checked here by brute force over the assignments and again by
tests/test_match_cpu.py): an assignment that rounding alone could flip is replaced by another case,
not loosened.  Case 1 is the pair of examples/donor_match.ipynb and must print its matrix.  Pure data:
numbers, names and printed lines only.  Follows make_bulk_golden.py (which it does not change)."""
import contextlib
import io
import os
import sys

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import vireoSNP                                                  # noqa: E402
from tests import match_np as M                                  # noqa: E402

MIN_MARGIN = 1e-6


def main():
    assert vireoSNP.__version__ == "0.5.9", vireoSNP.__version__
    rec = {}
    for k, (vcf1, vcf2, tag1, tag2) in enumerate(M.CASES, start=1):
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            rv = vireoSNP.vcf.match_VCF_samples(os.path.join(HERE, vcf1), os.path.join(HERE, vcf2), tag1, tag2)
        assert sorted(rv) == sorted(M.KEYS), sorted(rv)
        margin = M.assignment_margin(rv["full_GPb_diff"])
        assert margin >= MIN_MARGIN, (k, margin)
        assert rv["full_GPb_diff"].shape == M.SHAPES[k - 1] and rv["matched_n_var"] == M.N_MATCHED[k - 1]
        for key in M.KEYS:
            v = rv[key]
            rec["c%d_%s" % (k, key)] = np.asarray(v, dtype=str) if "donors" in key else np.asarray(v)
        rec["c%d_stdout" % k] = np.array(out.getvalue())
        rec["c%d_margin" % k] = np.float64(margin)
        print("case %d  %s x %s  matched %d  margin %.4f" % (k, tag1, tag2, rv["matched_n_var"], margin))
        print(out.getvalue(), end="")
    assert np.array_equal(np.round(rec["c1_full_GPb_diff"], 8), M.NOTEBOOK_DIFF)
    assert list(rec["c1_matched_donors2"]) == ["donor2", "donor1", "donor3", "donor0"]
    path = os.path.join(HERE, "c1_donor_match.npz")
    np.savez_compressed(path, **rec)
    print("c1_donor_match.npz %.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
