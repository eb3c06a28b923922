"""Cell VCF fixtures from the REAL reference (build container only, /root/reference):

    python tests/golden/make_cell_vcf_golden.py

  cell_vcf/<name>.vcf.gz   small cell VCFs written here, in cellSNP's layout (FORMAT GT:AD:DP:OTH:PL:ALL)
  c1_cell_vcf.npz          per file, and for the demo file data/cells.cellSNP.vcf.gz, what vireoSNP's
                           load_VCF(path, biallelic_only) -> read_sparse_GeneINFO(GenoINFO, ['AD', 'DP']) return:
                           indptr, indices and data of AD and DP (with their dtypes), the variant ids, the samples,
                           n_SNP_tagged, contigs, comments and FixedINFO (the lists for the small files, a SHA-256 of
                           them for the demo file)

Cases: both missing forms, one dot more than the missing form, AD '.' beside DP digits, values behind commas,
leading zeros, 9 and 10 digits, '+5', '1e3', ' 7', multi-allelic lines (kept with biallelic_only=False), a permuted
FORMAT, trailing blanks, DOS line ends, no final line end.  Pure data: text the script writes and the arrays the
reference returns.  Follows make_donor_vcf_golden.py."""
import contextlib
import gzip
import hashlib
import io
import os
import sys

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "cell_vcf")
sys.path.insert(0, REF)

import vireoSNP                                                   # noqa: E402
from vireoSNP.utils import vcf_utils                               # noqa: E402

FORMAT = ["GT", "AD", "DP", "OTH", "PL", "ALL"]
HEAD = ["##fileformat=VCFv4.2", "##contig=<ID=1>", "##contig=<ID=2>",
        '##FORMAT=<ID=AD,Number=1,Type=Integer,Description="alt depth">']
COLS = ["CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO", "FORMAT"]


def entry(rng, ad=None, dp=None, fmt=FORMAT):
    a = int(rng.integers(0, 30))
    code = dict(GT=["0/0", "1/0", "1/1"][rng.integers(3)], AD=str(a) if ad is None else ad,
                DP=str(a + int(rng.integers(0, 40))) if dp is None else dp, OTH=str(int(rng.integers(3))),
                PL="%d,%d,%d" % tuple(rng.integers(0, 300, 3)), ALL="%d,%d,%d,%d,%d" % tuple(rng.integers(0, 9, 5)))
    return ":".join(code[k] for k in fmt)


def make_lines(seed, n_cell, n_line, odd=False, permute_at=None):
    rng = np.random.default_rng(seed)
    special = [("3,0,12", "15"), (".", "7"), ("007", "0012"), ("123456789", "999999999"), (".", "."), ("0,3,45", "48")]
    if odd:
        special += [("1234567890", "1"), ("+5", "6"), ("1e3", "2000"), (" 7", "8"), ("2", "10000000000")]
    lines = []
    for i in range(n_line):
        ref, alt = "ACGT"[rng.integers(4)], "ACGT"[rng.integers(4)]
        if i % 9 == 4:
            alt += ",G"
        if i % 13 == 6:
            ref += "T"
        fmt = FORMAT if i != permute_at else ["AD", "GT", "ALL", "DP", "PL", "OTH"]
        fields = []
        for j in range(n_cell):
            kind = int(rng.integers(10))
            if kind < 4:
                fields.append(".:.:.:.:.:.")
            elif kind < 7:
                fields.append(".")
            elif kind == 7 and i % 3 == 0:
                fields.append(".:.:.:.:.:.:.")                     # one dot more: an entry
            elif kind == 8:
                ad, dp = special[(i + j) % len(special)]
                fields.append(entry(rng, ad, dp, fmt))
            else:
                fields.append(entry(rng, fmt=fmt))
        info = "AD=%d;DP=%d;OTH=0" % (rng.integers(50), rng.integers(50, 99))
        lines.append("\t".join([str(1 + i // 20), str(500 + 11 * i), ".", ref, alt, ".", "PASS", info, ":".join(fmt)]
                               + fields))
    return lines


def write(name, samples, lines, eol="\n", last=True, tails=None):
    text = eol.join(HEAD + ["#" + "\t".join(COLS + samples)]) + eol
    for i, line in enumerate(lines):
        text += line + (tails[i % len(tails)] if tails else "") + (eol if last or i + 1 < len(lines) else "")
    path = os.path.join(OUT, name + ".vcf.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as fh:
        fh.write(text.encode())
    return path


def reference(path, biallelic_only, digest):
    with contextlib.redirect_stdout(io.StringIO()):
        v = vcf_utils.load_VCF(path, biallelic_only=biallelic_only)
        m = vcf_utils.read_sparse_GeneINFO(v["GenoINFO"], keys=["AD", "DP"])
    out = dict(variants=np.array(v["variants"]), samples=np.array(v["samples"]), n_SNP_tagged=v["n_SNP_tagged"],
               contigs=np.array(v["contigs"]), comments=np.array(v["comments"]), shape=np.array(m["AD"].shape),
               fixed_keys=np.array(list(v["FixedINFO"])))
    for key in ("AD", "DP"):
        out[key + "_indptr"], out[key + "_indices"], out[key + "_data"] = m[key].indptr, m[key].indices, m[key].data
    if digest:
        h = hashlib.sha256()
        for k in v["FixedINFO"]:
            h.update(("\n".join([k] + v["FixedINFO"][k]) + "\n").encode())
        out["fixed_sha256"] = np.array(h.hexdigest())
    else:
        for k in v["FixedINFO"]:
            out["fixed_" + k] = np.array(v["FixedINFO"][k])
    return out


def main():
    assert vireoSNP.__version__ == "0.5.9", vireoSNP.__version__
    os.makedirs(OUT, exist_ok=True)
    cells7 = ["cell%d" % k for k in range(7)]
    cells70 = ["AAAC%04d-1" % k for k in range(70)]
    files = {
        "plain": write("plain", cells7, make_lines(1, 7, 40)),
        "wide": write("wide", cells70, make_lines(2, 70, 25)),
        "odd": write("odd", cells7, make_lines(3, 7, 40, odd=True)),
        "permuted": write("permuted", cells7, make_lines(4, 7, 30, permute_at=11)),
        "dos": write("dos", cells7, make_lines(5, 7, 30), eol="\r\n", last=False),
        "blanks": write("blanks", cells7, make_lines(6, 7, 30), tails=["", " ", "  \t", "\t "]),
    }
    out = {}
    for name, path in files.items():
        for bi in (True, False):
            for k, val in reference(path, bi, digest=False).items():
                out["%s__%d__%s" % (name, bi, k)] = val
        print(name, "kept", len(out[name + "__1__variants"]), "of", len(out[name + "__0__variants"]), "entries",
              len(out[name + "__1__AD_data"]))
    demo = os.path.join(HERE, "data", "cells.cellSNP.vcf.gz")
    for k, val in reference(demo, True, digest=True).items():
        out["demo__1__" + k] = val
    print("demo", len(out["demo__1__variants"]), "variants", len(out["demo__1__AD_data"]), "entries",
          int((out["demo__1__AD_data"] == 0).sum()), "explicit AD zeros")
    path = os.path.join(HERE, "c1_cell_vcf.npz")
    np.savez_compressed(path, **out)
    print("%.1f KB npz" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
