"""snp_gene_match / gene_counts on the GPU (vrx_genematch.h) against the restatement (tests/genematch_np.py, proven
equal to the real reference when the fixture was made) and against the fixture itself.  Everything is integers:
flags and lists are compared with ==, the gene-level matrices with (got != want).nnz == 0 -- no tolerance.

Matching: genes per chromosome 0, 1, T - 1, T, T + 1, 2 T + 1 (T = vrx_genematch_tile()), SNP counts 0, 1, 63, 64,
65, B - 1, B, B + 1 (B = vrx_genematch_block()), interleaved chromosomes, chromosomes on one side only,
boundary / degenerate / reversed genes, coordinates 0 and 2^31 - 1, ties, duplicates, a list longer than a wave
and a tile, every setting of the issue, int labels, dict against DataFrame, the verbose lines.
Aggregation: the listed special cases, the 2^31 error, and the command as a child process."""
import functools
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest
from scipy.sparse import csc_matrix, csr_matrix

from tests import genematch_np as GN

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
IMAX = GN.IMAX


@pytest.fixture(scope="module")
def va():
    import __graft_entry__ as entry
    entry.build()
    import vireo_amd
    from vireo_amd import _lib, gene_counts, snp_gene_match     # noqa: F401  (the names this file is about)
    _lib.require_gpu()
    return vireo_amd


def tile():
    from vireo_amd import _lib
    return int(_lib.lib().vrx_genematch_tile())


def block():
    from vireo_amd import _lib
    return int(_lib.lib().vrx_genematch_block())


def genes_of(chrom, start, stop):
    n = len(start)
    return dict(chrom=np.asarray(chrom), start=np.asarray(start, dtype=np.int64), stop=np.asarray(stop, dtype=np.int64),
                gene=GN.gene_names(n))


def check(va, chrom, pos, genes, **kw):
    """device == restatement on flags and lists; -> (flags, rows)"""
    gene_list, flag_list = va.snp_gene_match(dict(CHROM=chrom, POS=pos), genes, **kw)
    rest = {k: v for k, v in kw.items() if k in ("multi_gene", "gaps")}
    flags, rows = GN.match_rows(chrom, pos, genes["chrom"], genes["start"], genes["stop"], **rest)
    assert isinstance(flag_list, list) and all(type(f) is int for f in flag_list)
    assert flag_list == flags
    assert len(gene_list) == len(rows)
    for i, (got, want) in enumerate(zip(gene_list, rows)):
        assert got.dtype == genes["gene"].dtype
        assert got.tolist() == genes["gene"][want].tolist(), (i, flags[i])
    return flags, rows


@functools.lru_cache(maxsize=None)
def gold():
    with np.load(os.path.join(GOLD, "c1_genematch.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("i", range(len(GN.SETTINGS)))
def test_reference_fixture(va, i):
    z = gold()
    multi_gene, gaps = GN.SETTINGS[i]
    genes = genes_of(GN.chrom_names(z["gchrom"]), z["start"], z["stop"])
    var = dict(CHROM=list(GN.chrom_names(z["schrom"])), POS=[str(p) for p in z["pos"]])
    gene_list, flag_list = va.snp_gene_match(var, genes, multi_gene=multi_gene, gaps=gaps)
    key = GN.setting_key(i)
    assert flag_list == z[key + "_flag"].tolist()
    ptr, rows = z[key + "_ptr"], z[key + "_rows"]
    assert [len(g) for g in gene_list] == np.diff(ptr).tolist()
    assert np.concatenate(gene_list).tolist() == genes["gene"][rows].tolist()


@functools.lru_cache(maxsize=None)
def tile_case():
    """six chromosomes with 0, 1, T - 1, T, T + 1, 2 T + 1 genes in interleaved gene_df rows; 70 SNPs each,
    interleaved too.  Most genes are short against the chromosome, so every flag occurs; a few are long, so lists
    of several genes occur."""
    T = tile()
    rng = np.random.default_rng(5)
    sizes = [0, 1, T - 1, T, T + 1, 2 * T + 1]
    L = 40_000_000
    gchrom = rng.permutation(np.repeat(np.arange(6), sizes))
    n = gchrom.size
    start = rng.integers(0, L, n)
    stop = start + rng.choice([0, 30, 3000, 500_000], n, p=[0.05, 0.25, 0.68, 0.02])
    schrom = rng.permutation(np.repeat(np.arange(6), 70))
    pos = rng.integers(0, L, schrom.size)
    near = rng.random(schrom.size) < 0.5                            # half of the SNPs sit at or near a gene of theirs
    for i in np.flatnonzero(near):
        own = np.flatnonzero(gchrom == schrom[i])
        if own.size:
            g = rng.choice(own)
            pos[i] = max(0, start[g] + rng.choice([-20000, -5000, -500, -1, 0, 1, 10]))
    return genes_of(GN.chrom_names(gchrom), start, stop), GN.chrom_names(schrom), pos


@pytest.mark.parametrize("kw", [dict(), dict(gaps=[0]), dict(multi_gene=False), dict(gaps=[1000, 0, 50])],
                         ids=["default", "gaps0", "single", "unordered"])
def test_genes_per_chromosome_around_the_tile(va, kw):
    genes, chrom, pos = tile_case()
    flags, rows = check(va, chrom, pos, genes, **kw)
    if not kw:
        assert set(flags) == {0, 1, 2, 3, 4}
        assert max(len(r) for r in rows) > 1


def test_snp_counts_around_wave_and_block(va):
    rng = np.random.default_rng(6)
    B = block()
    start = rng.integers(0, 100000, 90)
    genes = genes_of(np.array(["1", "2", "3"])[rng.integers(0, 3, 90)], start, start + rng.integers(0, 5000, 90))
    for n in (0, 1, 63, 64, 65, B - 1, B, B + 1, 2 * B + 1):
        chrom = np.array(["1", "2", "3"])[rng.integers(0, 3, n)] if n else np.zeros(0, dtype=str)
        flags, rows = check(va, chrom, rng.integers(0, 110000, n), genes)
        assert len(flags) == n
    one = check(va, np.array(["2"]), np.array([int(genes["start"][genes["chrom"] == "2"][0])]), genes)
    assert one[0] == [0]
    gene_list, flag_list = va.snp_gene_match(dict(CHROM=[], POS=[]), genes)
    assert gene_list == [] and flag_list == []


def test_layout_interleaved_and_one_sided_chromosomes(va):
    genes = genes_of(["A", "B", "A", "G", "B"], [100, 100, 300, 100, 90], [200, 200, 400, 200, 250])
    chrom = ["A", "B", "A", "S", "B", "A", "S"]
    pos = [150, 150, 350, 150, 95, 250, 0]
    flags, rows = check(va, chrom, pos, genes)
    assert flags == [0, 0, 0, 4, 0, 1, 4]
    assert [r.tolist() for r in rows] == [[0], [1, 4], [2], [], [4], [0], []]
    # the same SNPs grouped by chromosome give the same answers: results do not depend on the order
    order = np.argsort(chrom, kind="stable")
    flags2, rows2 = check(va, [chrom[i] for i in order], [pos[i] for i in order], genes)
    assert flags2 == [flags[i] for i in order]
    assert all(np.array_equal(rows2[j], rows[i]) for j, i in enumerate(order))
    # no gene at all, and genes but on other chromosomes only
    empty = genes_of(np.zeros(0, dtype=str), [], [])
    assert check(va, chrom, pos, empty)[0] == [4] * 7
    assert check(va, ["S", "S"], [1, 2], genes)[0] == [4, 4]


def test_boundaries_degenerate_reversed_and_extreme_coordinates(va):
    #                 0     1     2     3      4     5       6        7            8
    start = np.array([100, 500, 700, 900, 0, IMAX, 0, IMAX, IMAX - 10])
    stop = np.array([200, 500, 650, 905, 0, IMAX, IMAX, 0, IMAX - 10])
    genes = genes_of(["1"] * 6 + ["2"] * 2 + ["3"], start, stop)
    chrom = ["1"] * 12 + ["2"] * 4 + ["3"] * 2
    pos = [100, 200, 150, 500, 499, 675, 650, 700, 0, IMAX, 902, 1_000_000, 0, IMAX, 5, IMAX - 1, 0, IMAX]
    for kw in (dict(), dict(multi_gene=False), dict(gaps=[0]), dict(gaps=[1, 2 ** 31 - 1, 2 ** 31]),
               dict(gaps=[-2 ** 31 + 2, -2 ** 31 + 1, 0])):
        check(va, chrom, pos, genes, **kw)
    flags, rows = check(va, chrom, pos, genes)
    # pos == start and pos == stop are distance 0: not "< 0", found by the 1000 gap as the nearest gene
    assert flags[:4] == [1, 1, 0, 1] and [r.tolist() for r in rows[:4]] == [[0], [0], [0], [1]]
    # a reversed interval: "inside" is between its ends as well
    assert flags[5] == 0 and rows[5].tolist() == [2]
    # chromosome 2: every position is inside or on the boundary of [0, IMAX] in either orientation
    assert [r.tolist() for r in rows[12:16]] == [[6], [6], [6, 7], [6, 7]]
    # the largest differences: a gene at IMAX - 10 seen from 0 needs a gap above IMAX - 10
    f, r = check(va, ["3", "3"], [0, IMAX], genes, gaps=[IMAX - 10, IMAX - 9])
    assert f == [1, 0] and [x.tolist() for x in r] == [[8], [8]]
    f, r = check(va, ["1"], [0], genes_of(["1"], [IMAX], [IMAX]), gaps=[IMAX, 2 ** 31])
    assert f == [1] and r[0].tolist() == [0]


def test_ties_duplicates_and_a_list_longer_than_a_tile(va):
    T = tile()
    # two genes at equal distance (the first row wins), identical duplicates (overlap: both; nearest: the first)
    genes = genes_of(["1"] * 6, [300, 100, 100, 300, 500, 500], [310, 110, 110, 310, 510, 510])
    flags, rows = check(va, ["1"] * 4, [205, 105, 400, 505], genes)
    assert flags == [1, 0, 1, 0] and [r.tolist() for r in rows] == [[0], [1, 2], [0], [4, 5]]
    flags, rows = check(va, ["1"] * 4, [205, 105, 400, 505], genes, multi_gene=False)
    assert [r.tolist() for r in rows] == [[0], [1], [0], [4]]
    # one SNP inside T + 70 genes of a chromosome of 2 T + 5, the rest of them elsewhere, other rows between
    rng = np.random.default_rng(8)
    n = 2 * T + 5
    inside = np.zeros(n, dtype=bool)
    inside[rng.choice(n, T + 70, replace=False)] = True
    start = np.where(inside, rng.integers(0, 1000, n), rng.integers(5000, 9000, n))
    stop = np.where(inside, rng.integers(1002, 2000, n), start + 10)
    gchrom = np.array(["7"] * n + ["8"] * 40)
    st2, sp2 = rng.integers(0, 3000, 40), rng.integers(0, 3000, 40)
    order = rng.permutation(n + 40)
    genes = genes_of(gchrom[order], np.concatenate([start, st2])[order], np.concatenate([stop, sp2])[order])
    chrom = ["8"] * 3 + ["7"] + ["8"] * 70 + ["7"] * 3
    pos = [5, 1500, 2999, 1001] + list(rng.integers(0, 3000, 70)) + [1001, 4000, 5005]
    flags, rows = check(va, chrom, pos, genes)
    assert len(rows[3]) == T + 70 and np.all(np.diff(rows[3]) > 0) and np.array_equal(rows[3], rows[74])
    check(va, chrom, pos, genes, gaps=[-1, 0])
    check(va, chrom, pos, genes, multi_gene=False)


def test_settings_and_labels(va):
    genes, chrom, pos = tile_case()
    sub = slice(0, None, 3)
    for kw in (dict(gaps=[-5, 0]), dict(gaps=[10 ** 15]), dict(gaps=[-10 ** 15, 10 ** 15]), dict(gaps=[0, 0, 5, 5]),
               dict(gaps=[0], multi_gene=False), dict(gaps=[100000, 10000, 1000, 0], multi_gene=0)):
        check(va, chrom[sub], pos[sub], genes, **kw)
    flags, rows = check(va, chrom[sub], pos[sub], genes, gaps=[10 ** 15])
    has = np.isin(chrom[sub], genes["chrom"])
    assert flags == [0 if h else 1 for h in has] and all(len(r) == int(h) for r, h in zip(rows, has))
    # int labels on both sides, and a gene key of another name and dtype
    g = dict(chrom=np.array([int(c[3:]) for c in genes["chrom"]]), start=genes["start"], stop=genes["stop"],
             id=np.arange(genes["start"].size) * 3)
    ichrom = np.array([int(c[3:]) for c in chrom])
    gene_list, flag_list = va.snp_gene_match(dict(CHROM=ichrom, POS=pos), g, gene_key="id")
    flags, rows = GN.match_rows(chrom, pos, genes["chrom"], genes["start"], genes["stop"])
    assert flag_list == flags and all(a.dtype == g["id"].dtype and a.tolist() == (r * 3).tolist()
                                      for a, r in zip(gene_list, rows))
    # labels of different kinds never match ('1' != 1), as with pandas
    gene_list, flag_list = va.snp_gene_match(dict(CHROM=[str(c) for c in ichrom[:50]], POS=pos[:50]), g, gene_key="id")
    assert flag_list == [4] * 50 and all(len(a) == 0 for a in gene_list)


def test_dataframe_equals_dict_and_verbose_lines(va, capsys):
    genes, chrom, pos = tile_case()
    var = dict(CHROM=list(chrom[:120]), POS=[str(p) for p in pos[:120]])
    df = pd.DataFrame(genes)
    a_list, a_flag = va.snp_gene_match(var, genes)
    capsys.readouterr()
    b_list, b_flag = va.vcf.snp_gene_match(var, df, verbose=True)
    out = capsys.readouterr().out.splitlines()
    assert a_flag == b_flag and all(x.tolist() == y.tolist() for x, y in zip(a_list, b_list))
    assert b_list[0].dtype == df["gene"].values.dtype
    want = [c for i, c in enumerate(var["CHROM"]) if i == 0 or var["CHROM"][i - 1] != c]
    assert out == ["processing: %s" % c for c in want] and len(want) > 6


# ---- gene counts ------------------------------------------------------------------------------------

def check_counts(va, AD, DP, lists, **kw):
    A, D, names = va.gene_counts(AD, DP, lists, **kw)
    wA, wD, wnames = GN.gene_counts(AD, DP, lists, **kw)
    assert np.asarray(names).tolist() == np.asarray(wnames).tolist()
    for got, want in ((A, wA), (D, wD)):
        assert isinstance(got, csc_matrix) and got.dtype == np.int64 and got.shape == want.shape
        assert (got != want).nnz == 0
        assert got.has_sorted_indices and not np.any(got.data == 0) and got.nnz == want.nnz
        chk = got.copy()
        chk.has_canonical_format = False
        chk.sum_duplicates()
        assert chk.nnz == got.nnz and np.array_equal(chk.indices, got.indices)
    return A, D, names


@functools.lru_cache(maxsize=None)
def count_case():
    rng = np.random.default_rng(9)
    n_var, n_cell, n_gene = 400, 60, 50
    DP = rng.poisson(0.4, (n_var, n_cell))
    DP[:, [3, 17, 59]] = 0                                           # empty columns
    DP[:, 5] = rng.integers(1, 9, n_var)                             # a full column
    AD = rng.binomial(DP, 0.3)
    names = GN.gene_names(n_gene)
    lists = []
    for v in range(n_var):
        k = rng.choice([0, 1, 1, 1, 2, 5])
        lists.append(names[np.sort(rng.choice(n_gene, k, replace=False))])
    lists[7] = names[:0]                                             # no gene
    lists[8] = names                                                 # every gene
    lists[9] = names[[4, 4, 11, 4]]                                  # a name several times in one list
    flags = rng.integers(0, 5, n_var)
    return AD, DP, lists, flags


def test_gene_counts_general_case_and_formats(va):
    AD, DP, lists, flags = count_case()
    A, D, names = check_counts(va, AD, DP, lists)
    assert A.shape == (50, 60) and D.nnz > A.nnz > 0
    check_counts(va, csr_matrix(AD), csc_matrix(DP).astype(np.float64), lists)
    check_counts(va, AD, DP, lists, flag_list=list(flags), max_flag=1)
    check_counts(va, AD, DP, lists, flag_list=flags, max_flag=-1)     # nobody contributes
    order = list(GN.gene_names(50)[::-1]) + ["absent"]
    A, D, names = check_counts(va, AD, DP, lists, gene_names=order)
    assert names.tolist() == order and A.shape[0] == 51 and A[50].nnz == 0


def test_gene_counts_special_cases(va):
    AD, DP, lists, _flags = count_case()
    zero = np.zeros_like(DP)
    A, D, _ = check_counts(va, zero, zero, lists)                     # nnz = 0
    assert A.nnz == 0 and D.nnz == 0 and A.shape == (50, 60)
    none = [np.zeros(0, dtype=str)] * len(lists)
    A, D, names = check_counts(va, AD, DP, none)                      # no SNP has a gene
    assert A.shape == (0, 60) and names.size == 0
    one = [np.array(["only"])] * len(lists)
    A, D, _ = check_counts(va, AD, DP, one)                           # n_gene == 1, every SNP in it
    assert np.array_equal(A.toarray()[0], AD.sum(0)) and np.array_equal(D.toarray()[0], DP.sum(0))
    # a column of 70 000 entries, each in two genes: far beyond anything a workgroup's LDS could hold
    rng = np.random.default_rng(10)
    n_var = 70_000
    col = rng.integers(1, 4, (n_var, 1))
    DPl = csc_matrix(np.hstack([col, np.zeros((n_var, 1), dtype=np.int64), (np.arange(n_var)[:, None] % 97 == 0) * 2]))
    names = GN.gene_names(30)
    long_lists = [names[[v % 30, (v * 7 + 1) % 30]] for v in range(n_var)]
    check_counts(va, DPl, DPl, long_lists)
    check_counts(va, np.zeros((0, 4), dtype=np.int64), np.zeros((0, 4), dtype=np.int64), [])   # no variant at all


def test_gene_counts_overflow_is_an_error_naming_gene_and_cell(va):
    big = 2 ** 30
    DP = np.zeros((4, 3), dtype=np.int64)
    DP[0, 2] = DP[2, 2] = big
    DP[1, 1] = DP[3, 1] = big
    lists = [np.array(["a", "b"]), np.array(["c"]), np.array(["b"]), np.array(["d"])]
    with pytest.raises(OverflowError, match="gene 'b', cell 2"):
        va.gene_counts(DP // 2, DP, lists)
    AD = DP.copy()
    AD[2, 2] -= 1                                                    # 2^31 - 1 still fits
    lists[3] = np.array(["c"])
    with pytest.raises(OverflowError, match="gene 'c', cell 1"):
        va.gene_counts(AD, DP, lists)
    DP[2, 2] -= 1
    DP[3, 1] -= 1
    AD = np.minimum(AD, DP)
    A, D, names = check_counts(va, AD, DP, lists)
    assert D.max() == 2 ** 31 - 1 and D.dtype == np.int64


def test_command_round_trip(va, tmp_path):
    from vireo_amd.io_utils import read_cellSNP, read_mtx
    data = os.path.join(GOLD, "data", "cellSNP_mat")
    dat = read_cellSNP(data)
    chrom, pos = np.array(dat["FixedINFO"]["CHROM"]), np.array(dat["FixedINFO"]["POS"]).astype(np.int64)
    rng = np.random.default_rng(11)
    pick = rng.choice(chrom.size, min(300, chrom.size), replace=False)
    start = np.maximum(0, pos[pick] + rng.integers(-30000, 2000, pick.size))
    stop = start + rng.choice([100, 5000, 60000], pick.size)
    gchrom = chrom[pick]
    names = np.array(["gene-%d" % i for i in range(pick.size)])
    table = tmp_path / "genes.tsv"
    with open(table, "w") as f:
        f.write("id\tchrom\tstart\tstop\tnote\n")
        f.write("".join("%s\t%s\t%d\t%d\tx\n" % t for t in zip(names, gchrom, start, stop)))
    out = str(tmp_path / "o")
    r = subprocess.run([sys.executable, "-m", "vireo_amd.gene_counts", "-c", data, "-g", str(table), "-o", out,
                        "--gaps", "0,1000,10000", "--maxFlag", "1", "--geneKey", "id"],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "[gene_counts]" in r.stdout and "RuntimeWarning" not in r.stderr
    flags, rows = GN.match_rows(chrom, pos, gchrom, start, stop, gaps=[0, 1000, 10000])
    lists = [names[x] for x in rows]
    assert 0 < sum(f <= 1 for f in flags) < len(flags)
    wA, wD, wnames = GN.gene_counts(dat["AD"], dat["DP"], lists, flag_list=flags, max_flag=1)
    assert open(os.path.join(out, "genes.tsv")).read().split("\n")[:-1] == wnames.tolist()
    for name, want in (("cellSNP.tag.AD.mtx", wA), ("cellSNP.tag.DP.mtx", wD)):
        got = read_mtx(os.path.join(out, name)).tocsc()
        assert got.shape == want.shape and (got != want).nnz == 0 and got.nnz == want.nnz
    assert open(os.path.join(out, "cellSNP.samples.tsv")).read() == open(os.path.join(data, "cellSNP.samples.tsv")).read()
    lines = open(os.path.join(out, "snp_gene.tsv")).read().split("\n")
    assert lines[0] == "chrom\tpos\tflag\tgenes" and lines[-1] == "" and len(lines) == chrom.size + 2
    want = ["%s\t%d\t%d\t%s" % (c, p, f, ",".join(g)) for c, p, f, g in zip(chrom, pos, flags, lists)]
    assert lines[1:-1] == want
    # the package attribute stays the function after the module has been imported by name
    import importlib
    importlib.import_module("vireo_amd.gene_counts")
    assert va.gene_counts(np.zeros((1, 1)), np.zeros((1, 1)), [np.array(["g"])])[2].tolist() == ["g"]
