"""SNP-to-gene matching fixture from the REAL reference (build container only, /root/reference, needs pandas):

    python tests/golden/make_genematch_golden.py

  c1_genematch.npz   the generated case of tests/genematch_np.fixture_case (chromosome codes, start, stop, pos)
                     and, for multi_gene in {True, False} x gaps in {default, [1000, 0, 50], [0]}, what
                     vireoSNP.utils.vcf_utils.snp_gene_match returns: the flags and the ragged lists as
                     (ptr, gene row index).  Names are "G%d" of the row, chromosomes "chr%d" of the code.

Asserts on the way that the restatement (tests/genematch_np.match_rows) equals the reference.
Pure data: numeric arrays only.  Follows make_varmix_golden.py."""
import os
import sys

import numpy as np
import pandas as pd

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import vireoSNP                                                   # noqa: E402
from vireoSNP.utils.vcf_utils import snp_gene_match               # noqa: E402
from tests import genematch_np as GN                              # noqa: E402


def main():
    assert vireoSNP.__version__ == "0.5.9", vireoSNP.__version__
    case = GN.fixture_case()
    n_gene = case["start"].size
    names = GN.gene_names(n_gene)
    gene_df = pd.DataFrame(dict(chrom=GN.chrom_names(case["gchrom"]), start=case["start"], stop=case["stop"],
                                gene=names))
    var = dict(CHROM=list(GN.chrom_names(case["schrom"])), POS=[str(p) for p in case["pos"]])
    out = dict(case)
    for i, (multi_gene, gaps) in enumerate(GN.SETTINGS):
        gene_list, flag_list = snp_gene_match(var, gene_df, multi_gene=multi_gene, gaps=gaps)
        rows = [np.array([int(x[1:]) for x in g], dtype=np.int64) for g in gene_list]
        flags, want = GN.match_rows(var["CHROM"], case["pos"], gene_df["chrom"].values, case["start"],
                                    case["stop"], multi_gene=multi_gene, gaps=gaps)
        assert flags == [int(f) for f in flag_list]
        assert all(np.array_equal(a, b) for a, b in zip(rows, want))
        ptr, flat = GN.ragged(rows)
        key = GN.setting_key(i)
        out[key + "_flag"] = np.array(flag_list, dtype=np.int32)
        out[key + "_ptr"], out[key + "_rows"] = ptr, flat
        print("multi_gene=%s gaps=%s: flags %s, longest list %d" % (
            multi_gene, gaps, np.bincount(flag_list, minlength=len(gaps) + 1).tolist(), int(np.diff(ptr).max())))
    path = os.path.join(HERE, "c1_genematch.npz")
    np.savez_compressed(path, **out)
    print("c1_genematch %.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
