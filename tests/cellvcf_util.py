"""Shared by tests/test_cell_vcf_cpu.py and tests/test_gpu_cell_vcf.py: the golden file of the real reference
(tests/golden/c1_cell_vcf.npz, made by tests/golden/make_cell_vcf_golden.py), exact comparison of two read_cellVCF
results, and a writer of tiny cell VCFs in cellSNP's layout."""
import gzip
import hashlib
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "c1_cell_vcf.npz")
FILES = os.path.join(HERE, "golden", "cell_vcf")
DEMO = os.path.join(HERE, "golden", "data", "cells.cellSNP.vcf.gz")
SMALL = ("plain", "wide", "odd", "permuted", "dos", "blanks")
FORMAT = "GT:AD:DP:OTH:PL:ALL"
BLANK = ".:.:.:.:.:."
HEAD = "##fileformat=VCFv4.2\n##contig=<ID=1>\n##source=test\n"
COLS = "CHROM POS ID REF ALT QUAL FILTER INFO FORMAT".split()
_gold = None


def gold():
    global _gold
    if _gold is None:
        _gold = dict(np.load(GOLD))
    return _gold


def small_path(name):
    return os.path.join(FILES, name + ".vcf.gz")


def check_golden(got, prefix):
    """every array with its dtype and every list of a read_cellVCF result against the reference's"""
    g = {k[len(prefix) + 2:]: v for k, v in gold().items() if k.startswith(prefix + "__")}
    assert g, prefix
    for key in ("AD", "DP"):
        m = got[key]
        assert m.shape == tuple(g["shape"]) and m.dtype == np.float64
        for part in ("indptr", "indices", "data"):
            have, want = getattr(m, part), g["%s_%s" % (key, part)]
            assert have.dtype == want.dtype, (key, part, have.dtype, want.dtype)
            assert np.array_equal(have, want), (key, part)
    assert got["variants"] == list(g["variants"]) and got["samples"] == list(g["samples"])
    assert got["contigs"] == list(g["contigs"]) and got["comments"] == list(g["comments"])
    assert got["n_SNP_tagged"].dtype == g["n_SNP_tagged"].dtype and np.array_equal(got["n_SNP_tagged"], g["n_SNP_tagged"])
    assert list(got["FixedINFO"]) == list(g["fixed_keys"])
    if "fixed_sha256" in g:
        h = hashlib.sha256()
        for k in got["FixedINFO"]:
            h.update(("\n".join([k] + got["FixedINFO"][k]) + "\n").encode())
        assert h.hexdigest() == str(g["fixed_sha256"])
    else:
        for k in got["FixedINFO"]:
            assert got["FixedINFO"][k] == list(g["fixed_" + k]), k
    assert got["n_lines"] == len(g["variants"])
    assert set(got["seconds"]) == {"inflate", "upload", "kernels", "download", "host"}


def same(a, b):
    """two read_cellVCF results: the same bits, dtypes and lists"""
    for key in ("AD", "DP"):
        assert a[key].shape == b[key].shape
        for part in ("indptr", "indices", "data"):
            x, y = getattr(a[key], part), getattr(b[key], part)
            assert x.dtype == y.dtype and np.array_equal(x, y), (key, part)
    for k in ("variants", "samples", "contigs", "comments", "FixedINFO", "n_lines"):
        assert a[k] == b[k], k
    assert a["n_SNP_tagged"].dtype == b["n_SNP_tagged"].dtype and np.array_equal(a["n_SNP_tagged"], b["n_SNP_tagged"])


def entry(ad, dp, gt="1/0"):
    return "%s:%s:%s:0:10,0,30:0,1,2,3,4" % (gt, ad, dp)


def make_line(i, fields, ref="A", alt="C", fmt=FORMAT, info="."):
    return "\t".join(["1", str(100 + 7 * i), ".", ref, alt, ".", "PASS", info, fmt] + list(fields))


def random_fields(rng, n_cell, rate=0.1):
    """about `rate` entries among both missing forms"""
    out = []
    for _ in range(n_cell):
        u = rng.random()
        if u < rate:
            a = int(rng.integers(0, 50))
            out.append(entry(a if rng.integers(4) else "0,%d" % a, a + int(rng.integers(0, 200))))
        else:
            out.append(BLANK if u < 0.6 else ".")
    return out


def write_vcf(path, n_cell, lines, eol="\n", last=True, head=HEAD):
    text = head.replace("\n", eol) + "#" + "\t".join(COLS + ["c%d" % k for k in range(n_cell)]) + eol
    text += eol.join(lines) + (eol if last and lines else "")
    with gzip.open(str(path), "wb") as fh:
        fh.write(text.encode("latin-1"))
    return str(path)
