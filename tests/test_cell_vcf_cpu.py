"""CPU-only: read_cellVCF's host path (force_host=True) against what the real reference makes of the demo file and of
the small crafted files (tests/golden/c1_cell_vcf.npz, made by tests/golden/make_cell_vcf_golden.py), the export, and
the host halves of the device path that need no GPU: the one line that is split for its FORMAT, and the repair of
flagged lines by the host functions."""
import numpy as np
import pytest

import __graft_entry__ as entry
from tests import cellvcf_util as U


@pytest.fixture(scope="module", autouse=True)
def built():
    entry.build()


def test_export_and_abi():
    import vireo_amd
    from vireo_amd import _lib, io_utils
    assert vireo_amd.read_cellVCF is io_utils.read_cellVCF and "read_cellVCF" in vireo_amd.__all__
    for name in ("create", "destroy", "segment", "format", "slab", "rows"):
        assert "vrx_cellvcf_" + name in _lib.SIGNATURES and getattr(_lib.lib(), "vrx_cellvcf_" + name) is not None
    seg = _lib.lib().vrx_cellvcf_segment()
    assert seg > 0 and seg % _lib.lib().vrx_vcf_chunk() == 0


def test_host_path_equals_the_reference_on_the_demo_file(capsys):
    import vireo_amd
    got = vireo_amd.read_cellVCF(U.DEMO, force_host=True)
    assert got["path"] == "host" and got["reason"] == "forced" and got["n_repaired"] == 0
    U.check_golden(got, "demo__1")
    assert got["AD"].nnz == 73046 and int((got["AD"].data == 0).sum()) == 40602      # the explicit zeros stay
    assert capsys.readouterr().out == ""


@pytest.mark.parametrize("biallelic_only", (True, False))
@pytest.mark.parametrize("name", U.SMALL)
def test_host_path_equals_the_reference_on_the_crafted_files(name, biallelic_only):
    import vireo_amd
    got = vireo_amd.read_cellVCF(U.small_path(name), biallelic_only=biallelic_only, force_host=True)
    U.check_golden(got, "%s__%d" % (name, biallelic_only))


def test_host_path_is_the_composition(monkeypatch):
    """VIREO_CELL_VCF=host forces the path like force_host; other keys and axes are the host's; a missing GPU is no
    reason for it"""
    import vireo_amd
    from vireo_amd import _lib, vcf_utils
    path = U.small_path("plain")
    v = vcf_utils.load_VCF(path, biallelic_only=True)
    want = vcf_utils.read_sparse_GeneINFO(v["GenoINFO"], keys=["AD", "DP"])
    monkeypatch.setenv("VIREO_CELL_VCF", "host")
    got = vireo_amd.read_cellVCF(path)
    assert got["path"] == "host" and got["reason"] == "forced"
    for key in ("AD", "DP"):
        assert (got[key] != want[key]).nnz == 0 and np.array_equal(got[key].indptr, want[key].indptr)
    monkeypatch.delenv("VIREO_CELL_VCF")
    three = vireo_amd.read_cellVCF(path, keys=("AD", "DP", "OTH"), axes=(-1, -1, -1))
    assert three["path"] == "host" and "two keys" in three["reason"] and three["OTH"].shape == want["AD"].shape
    first = vireo_amd.read_cellVCF(path, keys=("PL", "ALL"), axes=(0, -1))
    assert first["path"] == "host" and np.array_equal(first["PL"].indptr, want["AD"].indptr)
    if _lib.device_count() == 0:
        with pytest.raises(_lib.VrxError):
            vireo_amd.read_cellVCF(path)


def test_command_loader_keeps_the_load(capsys):
    from vireo_amd import _lib, vireo
    opts = vireo.build_parser().parse_args(["-c", U.small_path("wide")])[0]
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible here: tests/test_gpu_cell_vcf.py runs the command")
    dat = vireo.load_cells(opts)
    assert capsys.readouterr().out == "[vireo] Loading cell VCF file ...\n"
    assert sorted(dat) == ["AD", "DP", "FixedINFO", "comments", "contigs", "samples", "variants"]
    assert vireo.CELL_LOAD["path"] == "host" and "no HIP device" in vireo.CELL_LOAD["reason"]
    assert set(vireo.CELL_LOAD) == {"path", "reason", "seconds", "n_lines", "n_repaired"}
    want = U.gold()
    assert np.array_equal(dat["AD"].data, want["wide__1__AD_data"]) and dat["variants"] == list(want["wide__1__variants"])


def test_first_kept_format():
    from vireo_amd.io_utils import _first_kept_format
    multi = U.make_line(0, ["."], alt="C,G")
    kept = U.make_line(1, [".", U.entry(1, 2)], fmt="AD:DP") + " \x1c"
    assert _first_kept_format(bytearray((multi + "\n" + kept + "\n").encode()), True) == (b"AD:DP", None)
    assert _first_kept_format(bytearray((multi + "\n" + kept).encode()), False) == (U.FORMAT.encode(), None)
    assert _first_kept_format(bytearray((multi + "\n").encode()), True) == (None, None)
    assert _first_kept_format(bytearray(b""), True) == (None, None)
    nine = "\t".join(kept.split("\t")[:9])                        # FORMAT ends the line: rstrip() takes its blanks
    assert _first_kept_format(bytearray((nine + "\n").encode()), True) == (b"AD:DP", None)
    fmt, why = _first_kept_format(bytearray(b"1\t5\t.\tA\tC\t.\t.\t.\n"), True)
    assert fmt is None and "fewer than 9" in why
    fmt, why = _first_kept_format(bytearray(("##late\n" + kept + "\n").encode()), True)
    assert fmt is None and "'#' line" in why


def test_repair_is_the_host_functions(tmp_path):
    """the values of a flagged line as the device path overwrites them: the same numbers and the same exceptions as
    load_VCF + read_sparse_GeneINFO on a file that holds that line alone"""
    import vireo_amd
    from vireo_amd.io_utils import _cell_repair
    from vireo_amd.vcf_utils import read_sparse_GeneINFO
    fmt = U.FORMAT.split(":")
    odd = [U.entry("1234567890", "+5"), ".", U.entry("1e3", " 7"), U.BLANK, U.entry("0,3,45", "."), U.BLANK + ":."]
    for fields, error in ((odd, None), ([U.entry("abc", 3)], ValueError), ([U.entry("3,", 3)], ValueError),
                          ([".", "1/0:3"], IndexError)):
        line = U.make_line(0, fields)
        path = U.write_vcf(tmp_path / "one.vcf.gz", len(fields), [line])
        if error is IndexError:
            for fn in (lambda: vireo_amd.read_cellVCF(path, force_host=True),
                       lambda: _cell_repair([(line + "\r\n").encode()], fmt)):
                with pytest.raises(IndexError):
                    fn()
            continue
        geno = _cell_repair([(line + " \r\n").encode()], fmt)[0]
        if error is not None:
            with pytest.raises(error) as want:
                vireo_amd.read_cellVCF(path, force_host=True)
            with pytest.raises(error) as got:
                read_sparse_GeneINFO(geno, keys=["AD"], axes=[-1])
            assert str(got.value) == str(want.value)
            continue
        whole = vireo_amd.read_cellVCF(path, force_host=True)
        assert geno["indices"] == whole["AD"].indices.tolist() == [0, 2, 4, 5]
        for key in ("AD", "DP"):
            assert np.array_equal(read_sparse_GeneINFO(geno, keys=[key], axes=[-1])[key].data, whole[key].data)
        assert whole["AD"].data.tolist() == [1234567890.0, 1000.0, 45.0, 0.0]
        assert whole["DP"].data.tolist() == [5.0, 7.0, 0.0, 0.0]
