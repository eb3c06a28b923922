"""SNP-to-gene matching and gene counts without a GPU: the restatement (tests/genematch_np.py) against the fixture
captured from the real reference (tests/golden/c1_genematch.npz, six settings), the host half of the device path
(``prepare``: codes, grouping, sorting, clamped gaps) walked in NumPy the way the kernel walks it, the argument
errors, the gene table parser of the command, and the build with its new symbols."""
import functools
import os

import numpy as np
import pytest

from tests import genematch_np as GN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "c1_genematch.npz")


@functools.lru_cache(maxsize=None)
def gold():
    with np.load(GOLD) as z:
        return {k: z[k] for k in z.files}


def walk(p):
    """The kernel's two passes on a ``prepare`` result, lane by lane: minimum and first row, the winning gap,
    then the set -- with the int32 arithmetic of vrx_gm_dist"""
    n = p["n_snp"]
    flags, rows = [0] * n, [None] * n
    for j in range(n):
        c, pos = p["code"][j], p["pos"][j]
        g0, g1 = p["chrom_ptr"][c], p["chrom_ptr"][c + 1]
        d1, d2 = p["start"][g0:g1] - pos, p["stop"][g0:g1] - pos
        assert d1.dtype == np.int32
        m = np.minimum(np.abs(d1), np.abs(d2))
        dist = np.where((d1 < 0) != (d2 < 0), -m, m)
        k, out = p["gap_m1"].size, np.zeros(0, dtype=np.int64)
        if dist.size:
            hit = np.flatnonzero(dist.min() <= p["gap_m1"])
            if hit.size:
                k = int(hit[0])
                at = [int(np.argmin(dist))] if p["single"][k] else np.flatnonzero(dist <= p["gap_m1"][k])
                out = p["row"][g0:g1][at].astype(np.int64)
        flags[p["perm"][j]], rows[p["perm"][j]] = k, out
    return flags, rows


@pytest.mark.parametrize("i", range(len(GN.SETTINGS)))
def test_restatement_and_host_half_equal_the_reference_fixture(i):
    from vireo_amd import gene_match as GM
    z = gold()
    multi_gene, gaps = GN.SETTINGS[i]
    key = GN.setting_key(i)
    chrom, gchrom = GN.chrom_names(z["schrom"]), GN.chrom_names(z["gchrom"])
    flags, rows = GN.match_rows(chrom, z["pos"], gchrom, z["start"], z["stop"], multi_gene=multi_gene, gaps=gaps)
    ptr, flat = GN.ragged(rows)
    assert np.array_equal(flags, z[key + "_flag"])
    assert np.array_equal(ptr, z[key + "_ptr"]) and np.array_equal(flat, z[key + "_rows"])
    p = GM.prepare(chrom, [str(x) for x in z["pos"]], gchrom, z["start"], z["stop"], multi_gene=multi_gene, gaps=gaps)
    flags2, rows2 = walk(p)
    ptr2, flat2 = GN.ragged(rows2)
    assert np.array_equal(flags2, z[key + "_flag"])
    assert np.array_equal(ptr2, z[key + "_ptr"]) and np.array_equal(flat2, z[key + "_rows"])


def test_fixture_is_the_generated_case_and_covers_the_planted_kinds():
    z, case = gold(), GN.fixture_case()
    for k, v in case.items():
        assert np.array_equal(z[k], v), k
    assert set(np.unique(z["s0_flag"])) == {0, 1, 2, 3, 4}
    assert np.diff(z["s0_ptr"]).max() > 1 and np.diff(z["s3_ptr"]).max() == 1
    assert np.any(z["start"] > z["stop"]) and np.any(z["start"] == z["stop"])
    assert z["pos"].max() == GN.IMAX and z["pos"].min() == 0


def test_prepare_clamps_gaps_without_changing_a_comparison():
    from vireo_amd import gene_match as GM
    gap_m1, single = GM._gaps([0, 1, -5, 10 ** 15, -10 ** 15, 2 ** 31, 2 ** 31 - 1, -2 ** 31 + 1], True)
    assert gap_m1.tolist() == [-1, 0, -6, 2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1, 2 ** 31 - 2, -2 ** 31]
    assert single.tolist() == [0, 1, 0, 1, 0, 1, 1, 0]
    assert GM._gaps([0, -3], False)[1].tolist() == [1, 1]
    assert GM._gaps([0], 0)[1].tolist() == [0]            # `multi_gene is False`: 0 is not False


def _genes(**over):
    g = dict(chrom=np.array(["1", "1"]), start=np.array([10, 50]), stop=np.array([20, 60]),
             gene=np.array(["A", "B"]))
    g.update(over)
    return g


def test_argument_errors_need_no_gpu(monkeypatch):
    from vireo_amd import _lib, gene_match as GM

    def no_gpu():
        raise AssertionError("the GPU was asked for before the arguments were checked")
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    var = dict(CHROM=["1", "1"], POS=["15", "70"])
    with pytest.raises(ValueError, match="gaps"):
        GM.snp_gene_match(var, _genes(), gaps=[])
    for bad in ([15.5, 70], [float("nan"), 70], [-1, 70], [2 ** 31, 70], ["15.5", "70"], ["x", "70"]):
        with pytest.raises(ValueError, match="POS"):
            GM.snp_gene_match(dict(CHROM=["1", "1"], POS=bad), _genes())
    for col in ("start", "stop"):
        for bad in ([10.5, 50], [np.nan, 50], [-10, 50], [2 ** 31, 50]):
            with pytest.raises(ValueError, match=col):
                GM.snp_gene_match(var, _genes(**{col: np.array(bad)}))
    # the largest legal coordinate passes the checks and reaches the device call
    with pytest.raises(AssertionError, match="GPU"):
        GM.snp_gene_match(dict(CHROM=["1"], POS=[2 ** 31 - 1]), _genes(stop=np.array([20, 2 ** 31 - 1])))


def test_gene_index_and_missing_name(monkeypatch):
    from vireo_amd import _lib, gene_match as GM
    monkeypatch.setattr(_lib, "require_gpu", lambda: (_ for _ in ()).throw(AssertionError("GPU")))
    lists = [np.array(["B", "A"]), np.array([], dtype=str), np.array(["B", "B"]), np.array(["C"])]
    names, gptr, gid = GM.gene_index(lists)
    assert names.tolist() == ["A", "B", "C"] and gptr.tolist() == [0, 2, 2, 4, 5] and gid.tolist() == [1, 0, 1, 1, 2]
    names, gptr, gid = GM.gene_index(lists, gene_names=["C", "B", "Z", "A"])
    assert names.tolist() == ["C", "B", "Z", "A"] and gid.tolist() == [1, 3, 1, 1, 0]
    names, gptr, gid = GM.gene_index(lists, flag_list=[0, 4, 1, 0], max_flag=0)
    assert names.tolist() == ["A", "B", "C"] and gptr.tolist() == [0, 2, 2, 2, 3] and gid.tolist() == [1, 0, 2]
    with pytest.raises(ValueError, match="'C' is not in gene_names"):
        GM.gene_index(lists, gene_names=["A", "B"])
    with pytest.raises(ValueError, match="twice"):
        GM.gene_index(lists, gene_names=["A", "B", "C", "A"])
    import __graft_entry__ as entry
    entry.build()                                       # merge_counts is host code of the library
    AD = np.array([[1, 0], [0, 2], [1, 1], [0, 3]])
    with pytest.raises(ValueError, match="not in gene_names"):
        GM.gene_counts(AD, AD + 1, lists, gene_names=["A", "B"])
    with pytest.raises(ValueError, match="gene_list has 3"):
        GM.gene_counts(AD, AD + 1, lists[:3])


def test_restatement_of_gene_counts_on_a_hand_case():
    AD = np.array([[1, 0, 2], [0, 2, 0], [1, 1, 0], [0, 3, 0]])
    DP = AD + np.array([[0, 0, 1], [1, 0, 0], [0, 0, 0], [0, 0, 0]])
    lists = [np.array(["B", "A"]), np.array([], dtype=str), np.array(["B", "B"]), np.array(["C"])]
    A, D, names = GN.gene_counts(AD, DP, lists)
    assert names.tolist() == ["A", "B", "C"]
    assert A.toarray().tolist() == [[1, 0, 2], [3, 2, 2], [0, 3, 0]]
    assert D.toarray().tolist() == [[1, 0, 3], [3, 2, 3], [0, 3, 0]]
    assert A.has_canonical_format and not np.any(A.data == 0)


def test_gene_table_parser(tmp_path):
    from vireo_amd.gene_match import parse_genes
    path = tmp_path / "genes.tsv"
    path.write_text("#name\tchrom\tstrand\tstart\tstop\n"
                    "TP53\tchr17\t-\t7661779\t7687550\n"
                    "\n"
                    "X Y\t17\t+\t0\t2147483647\r\n")
    g = parse_genes(str(path), gene_key="name")
    assert g["chrom"].tolist() == ["chr17", "17"] and g["name"].tolist() == ["TP53", "X Y"]
    assert g["start"].tolist() == [7661779, 0] and g["stop"].tolist() == [7687550, 2147483647]
    assert g["start"].dtype == np.int64
    with pytest.raises(ValueError, match="no column 'gene'"):
        parse_genes(str(path))
    path.write_text("chrom\tstart\tstop\tgene\n1\t5\t9.5\tA\n")
    with pytest.raises(ValueError, match="integers"):
        parse_genes(str(path))
    path.write_text("chrom\tstart\tstop\tgene\n1\t5\n")
    with pytest.raises(ValueError, match="line 2"):
        parse_genes(str(path))
    path.write_text("chrom\tstart\tstop\tgene\n")
    g = parse_genes(str(path))
    assert all(g[k].size == 0 for k in ("chrom", "start", "stop", "gene"))


def test_build_resolves_the_new_symbols_and_exports():
    import __graft_entry__ as entry
    entry.build()
    import vireo_amd
    from vireo_amd import _lib
    L = _lib.lib()
    for name in ("vrx_genematch_create", "vrx_genematch_destroy", "vrx_genematch_match", "vrx_genematch_lists",
                 "vrx_genematch_tile", "vrx_genematch_block", "vrx_genecount_create", "vrx_genecount_read",
                 "vrx_genecount_destroy"):
        assert name in _lib.SIGNATURES and getattr(L, name) is not None
    assert L.vrx_genematch_tile() >= 64 and L.vrx_genematch_block() % 64 == 0
    assert vireo_amd.vcf.snp_gene_match is vireo_amd.snp_gene_match is vireo_amd.vcf_utils.snp_gene_match
    assert callable(vireo_amd.gene_counts)
    for mod in ("gene_match.py", "gene_counts.py"):
        assert "import pandas" not in open(os.path.join(ROOT, "vireo_amd", mod)).read()


def test_library_rejects_malformed_tables_before_any_device_call():
    import ctypes as C
    import __graft_entry__ as entry
    entry.build()
    from vireo_amd import _lib
    L = _lib.lib()
    i32, i64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    h = C.c_void_p()
    ok = np.array([5, 9], dtype=np.int32)

    def create(ptr, start=ok, stop=ok, row=np.array([0, 1], dtype=np.int32), n_gene=2):
        ptr = np.array(ptr, dtype=np.int64)
        return L.vrx_genematch_create(0, ptr.size - 1, n_gene, ptr.ctypes.data_as(i64), start.ctypes.data_as(i32),
                                      stop.ctypes.data_as(i32), row.ctypes.data_as(i32), C.byref(h))
    for ptr in ([0, 1], [1, 2], [0, 3, 2]):                          # not 0 .. n_gene, not monotone
        with pytest.raises(_lib.VrxError, match="chrom_ptr"):
            _lib.check(create(ptr))
    with pytest.raises(_lib.VrxError, match="negative"):
        _lib.check(create([0, 2], start=np.array([5, -1], dtype=np.int32)))
    assert not h.value
    n_out = C.c_int64(0)
    colptr, gptr = np.array([0, 1], dtype=np.int64), np.array([0, 1], dtype=np.int64)
    one = np.array([0], dtype=np.int32)
    for gid, row in ((np.array([3], dtype=np.int32), one), (one, np.array([1], dtype=np.int32))):
        with pytest.raises(_lib.VrxError, match="vrx_genecount_create"):
            _lib.check(L.vrx_genecount_create(0, 1, 1, 2, colptr.ctypes.data_as(i64), row.ctypes.data_as(i32),
                                              one.ctypes.data_as(i32), one.ctypes.data_as(i32), gptr.ctypes.data_as(i64),
                                              gid.ctypes.data_as(i32), C.byref(h), C.byref(n_out), None))
    assert not h.value
