"""Donor VCF fixtures from the REAL reference (build container only, /root/reference):

    python tests/golden/make_donor_vcf_golden.py

  donor_vcf/<name>.vcf.gz   small donor VCFs generated here (5 samples, about 60 lines each)
  donor_vcf/<name>.npz      per tag and cell-id list what vireoSNP's load_VCF(biallelic_only=True, sparse=False,
                            format_list=[tag]) -> io_utils.match_donor_VCF -> parse_donor_GPb return: GPb, the kept
                            cell indices, the samples, the lines and the lines whose FORMAT names the tag; the
                            cell-id lists themselves

Cases: GT phased / unphased / haploid / missing, PL with ties for the minimum and values up to 4095, GP with 1-15
digits, FORMAT without the tag on some lines, multi-allelic lines, "chr" on either side, a shuffled cell list, no
match.  Pure data: text the script writes and the arrays the reference returns.  Follows make_varmix_golden.py."""
import contextlib
import gzip
import io
import os
import sys

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "donor_vcf")
sys.path.insert(0, REF)

import vireoSNP                                                   # noqa: E402
from vireoSNP.utils import io_utils, vcf_utils                     # noqa: E402

SAMPLES = ["donorA", "donorB", "d3", "sample_4", "E"]
HEAD = ["##fileformat=VCFv4.2", "##contig=<ID=1>", '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">']


def gt_code(rng):
    return ["0/0", "0/1", "1/0", "1/1", "0|0", "0|1", "1|0", "1|1", "0", "1", ".", "./.", ".|."][rng.integers(13)]


def pl_code(rng):
    kind = rng.integers(5)
    if kind == 0:
        v = [0, 0, int(rng.integers(4096))]                        # a tie for the minimum
    elif kind == 1:
        v = [4095, int(rng.integers(4096)), 4095]
    elif kind == 2:
        v = [7, 7, 7]
    else:
        v = [int(x) for x in rng.integers(0, 4096, 3)]
    rng.shuffle(v)
    return ",".join(str(x) for x in v)


def gp_number(rng):
    n = int(rng.integers(1, 16))                                    # significant digits
    digits = "".join(str(x) for x in rng.integers(0, 10, n))
    cut = int(rng.integers(0, n))                                   # digits after the point
    if cut == 0:
        return str(int(digits))
    whole = digits[:n - cut].lstrip("0") or "0"
    return whole + "." + digits[n - cut:]


def gp_code(rng):
    if rng.integers(4) == 0:
        return ["1,0,0", "0.5,0.5,0", "0.001,0.998,0.001", "0,0,1"][rng.integers(4)]
    return ",".join(gp_number(rng) for _ in range(3))


def make_file(name, seed, chrom_prefix, n_lines=60):
    rng = np.random.default_rng(seed)
    lines = list(HEAD) + ["#" + "\t".join(["CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO", "FORMAT"]
                                           + SAMPLES)]
    ids = []
    for i in range(n_lines):
        chrom = chrom_prefix + str(1 + i // 25) if i % 17 else chrom_prefix + "X"
        pos = str(1000 + 37 * i)
        ref, alt = "ACGT"[rng.integers(4)], "ACGT"[rng.integers(4)]
        if i % 11 == 5:
            alt = alt + ",T"                                        # multi-allelic: dropped
        if i % 13 == 7:
            ref = ref + "GG"                                        # a deletion: dropped
        fmt = [["GT", "PL", "GP"], ["GT", "GP", "PL"], ["PL", "GP"], ["GT"], ["GT", "DP", "PL", "GP"]][i % 5]
        fields = []
        for _s in SAMPLES:
            code = dict(GT=gt_code(rng), PL=pl_code(rng), GP=gp_code(rng), DP=str(int(rng.integers(100))))
            if rng.integers(9) == 0:
                code["PL"] = code["GP"] = "."
            fields.append(":".join(code[k] for k in fmt))
        info = "AD=%d;DP=%d" % (rng.integers(50), rng.integers(50, 99)) if i % 3 else "."
        lines.append("\t".join([chrom, pos, ".", ref, alt, ".", "PASS", info, ":".join(fmt)] + fields))
        ids.append("_".join((chrom, pos, ref, alt)))
    path = os.path.join(OUT, name + ".vcf.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as fh:
        fh.write(("\n".join(lines) + "\n").encode())
    return path, ids


def reference(path, tag, cell_ids):
    with contextlib.redirect_stdout(io.StringIO()):
        v = vcf_utils.load_VCF(path, biallelic_only=True, sparse=False, format_list=[tag])
        n_lines, n_tagged = len(v['GenoINFO'][tag]), int(v['n_SNP_tagged'][0])
        cell = dict(AD=np.zeros((len(cell_ids), 1)), DP=np.zeros((len(cell_ids), 1)), variants=list(cell_ids),
                    FixedINFO={})
        kept_before = list(cell_ids)
        cell, v = io_utils.match_donor_VCF(cell, v)
        keep = np.array([kept_before.index(x) for x in cell['variants']], dtype=np.int64)
        if len(keep):
            GPb = vcf_utils.parse_donor_GPb(v['GenoINFO'][tag], tag)
        else:
            GPb = np.zeros((0, len(v['samples']), 3))
    return dict(GPb=GPb, keep=keep, samples=np.array(v['samples']), n_lines=np.int64(n_lines),
                n_tagged=np.int64(n_tagged))


def main():
    assert vireoSNP.__version__ == "0.5.9", vireoSNP.__version__
    os.makedirs(OUT, exist_ok=True)
    for name, seed, prefix in (("plain", 11, ""), ("chr", 12, "chr")):
        path, ids = make_file(name, seed, prefix)
        rng = np.random.default_rng(seed + 100)
        bare = [x[len(prefix):] for x in ids]
        absent = ["%s9_%d_A_C" % (prefix, 5 + k) for k in range(7)]
        every_other = [x for k, x in enumerate(ids) if k % 2 == 0]
        lists = {
            "inorder": every_other[:10] + absent[:3] + every_other[10:] + absent[3:],
            "shuffled": [str(x) for x in rng.permutation(ids + absent)],
            "nomatch": absent,
            # the "chr" retries of match_SNPs: cells without the prefix against a donor file with it, and the reverse
            "other_side": [str(x) for x in rng.permutation(bare if prefix else ["chr" + x for x in ids])][:40],
        }
        out = {}
        for lname, cell_ids in lists.items():
            out["list_" + lname] = np.array(cell_ids)
            for tag in ("GT", "PL", "GP"):
                for k, val in reference(path, tag, cell_ids).items():
                    out["%s_%s_%s" % (tag, lname, k)] = val
                print(name, lname, tag, "kept", len(out["%s_%s_keep" % (tag, lname)]), "of", len(cell_ids),
                      "lines", int(out["%s_%s_n_lines" % (tag, lname)]), "tagged", int(out["%s_%s_n_tagged" % (tag, lname)]))
        np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
        print("%s: %.1f KB text, %.1f KB npz" % (name, os.path.getsize(path) / 1024,
                                                 os.path.getsize(os.path.join(OUT, name + ".npz")) / 1024))


if __name__ == "__main__":
    main()
