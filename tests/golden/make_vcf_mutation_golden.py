"""What the REAL reference does with the mutation corpus of tests/vcf_mutate.py (build container only,
/root/reference):

    python tests/golden/make_vcf_mutation_golden.py

  vcf_mutation.npz   per corpus ('donor', 'cell') and file: the SHA-256 of its decompressed text; per donor file and
                     tag in GT / PL / GP what vireoSNP's load_VCF(biallelic_only=True, sparse=False, format_list=[tag])
                     -> match_SNPs(cells, variants) -> parse_donor_GPb do with it; per cell file and biallelic_only
                     what load_VCF(path, biallelic_only) -> read_sparse_GeneINFO(GenoINFO, ['AD', 'DP']) do with it.
                     An outcome is the class name of the exception (SystemExit: the reference's exit()), or one SHA-256
                     over everything returned (vcf_mutate.donor_digest: keep, the matched lines, GPb's shape and bytes,
                     the samples, the kept and the tagged lines; vcf_mutate.cell_digest: the shape, indptr / indices /
                     data of AD and DP with their dtypes, the variant ids, the samples, n_SNP_tagged).

Pure data: digests and class names.  The script prints how many files return and how many raise, by class, and the
shares the CPU test asserts.  Follows make_cell_vcf_golden.py and make_donor_vcf_golden.py."""
import collections
import contextlib
import io
import os
import sys
import tempfile

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, REF)

import vireoSNP                                                   # noqa: E402
from vireoSNP.utils import vcf_utils                               # noqa: E402

from tests import vcf_mutate as M                                  # noqa: E402


def donor(path, tag, cells):
    v = vcf_utils.load_VCF(path, biallelic_only=True, sparse=False, format_list=[tag])
    rows = v["GenoINFO"][tag]
    mm = vcf_utils.match_SNPs(cells, v["variants"])
    keep = np.where(mm != None)[0]                                 # noqa: E711
    line = mm[keep].astype(np.int64)
    GPb = vcf_utils.parse_donor_GPb([rows[x] for x in line], tag)
    return M.donor_digest(keep, line, GPb, v["samples"], len(rows), v["n_SNP_tagged"][0])


def cell(path, biallelic_only):
    v = vcf_utils.load_VCF(path, biallelic_only=biallelic_only)
    m = vcf_utils.read_sparse_GeneINFO(v["GenoINFO"], keys=["AD", "DP"])
    return M.cell_digest(m["AD"], m["DP"], v["variants"], v["samples"], v["n_SNP_tagged"])


def main():
    assert vireoSNP.__version__ == "0.5.9", vireoSNP.__version__
    out, classes = {}, [""]
    with tempfile.TemporaryDirectory() as tmp:
        for kind, cases in (("donor", M.TAGS), ("cell", (True, False))):
            files = M.corpus(kind)
            text = np.zeros((len(files), 32), np.uint8)
            digest = np.zeros((len(files), len(cases), 32), np.uint8)
            raised = np.zeros((len(files), len(cases)), np.uint8)
            tally = collections.Counter()
            for k, f in enumerate(files):
                path = f.write(tmp)
                text[k] = np.frombuffer(bytes.fromhex(f.sha256), np.uint8)
                for c, case in enumerate(cases):
                    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all="ignore"):
                        got = M.outcome((lambda: donor(path, case, f.cells)) if kind == "donor"
                                        else (lambda: cell(path, case)))
                    if got[0] == "ok":
                        digest[k, c] = np.frombuffer(bytes.fromhex(got[1]), np.uint8)
                    else:
                        if got[1] not in classes:
                            classes.append(got[1])
                        raised[k, c] = classes.index(got[1])
                    tally["returns" if got[0] == "ok" else got[1]] += 1
            out[kind + "_text"], out[kind + "_digest"], out[kind + "_raised"] = text, digest, raised
            n = len(files) * len(cases)
            everywhere = int((raised == 0).all(axis=1).sum())
            print("%s: %d files x %d cases: %s" % (kind, len(files), len(cases), ", ".join(
                "%s %d (%.0f %%)" % (name, count, 100.0 * count / n) for name, count in tally.most_common())))
            print("  the reference returns in every case on %d files (%.0f %%), field-only files %d (%.0f %%), "
                  "mutations in the sample region %.0f %%"
                  % (everywhere, 100.0 * everywhere / len(files), sum(f.field_only for f in files),
                     100.0 * sum(f.field_only for f in files) / len(files),
                     100.0 * np.mean([m[2] == "sample" for f in files for m in f.mutations])))
    out["classes"] = np.array(classes)
    path = os.path.join(HERE, "vcf_mutation.npz")
    np.savez_compressed(path, **out)
    print("%.1f KB npz" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
