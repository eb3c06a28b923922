"""CPU-only: load_donor_GPb's host path (force_host=True) against the real reference's numbers in
tests/golden/donor_vcf/ (made by tests/golden/make_donor_vcf_golden.py), and the two arithmetic rules the device
parser rests on -- the GP digit rule and the PL table -- restated in NumPy against float() and the reference
expression.  These fixtures are well-formed; what the host path does with malformed text -- ragged rows, control bytes,
truncated lines, a missing #CHROM line -- is held to the reference's result or exception class, file by file, in
tests/test_vcf_mutation_cpu.py."""
import os

import numpy as np
import pytest

import __graft_entry__ as entry

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "donor_vcf")
FILES = ("plain", "chr")
LISTS = ("inorder", "shuffled", "nomatch", "other_side")
TAGS = ("GT", "PL", "GP")


@pytest.fixture(scope="module", autouse=True)
def built():
    entry.build()


def check_fixture(got, gold, tag, lname):
    want = {k: gold["%s_%s_%s" % (tag, lname, k)] for k in ("GPb", "keep", "samples", "n_lines", "n_tagged")}
    assert got["samples"] == list(want["samples"])
    assert np.array_equal(got["keep"], want["keep"])
    assert got["GPb"].dtype == np.float64 and got["GPb"].shape == want["GPb"].shape
    assert got["GPb"].tobytes() == want["GPb"].tobytes()
    assert (got["n_lines"], got["n_tagged"]) == (int(want["n_lines"]), int(want["n_tagged"]))
    assert got["keep"].dtype == np.int64 and got["line"].dtype == np.int64 and len(got["line"]) == len(got["keep"])
    assert set(got["seconds"]) == {"inflate", "upload", "kernels", "download", "host"}


@pytest.mark.parametrize("lname", LISTS)
@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("name", FILES)
def test_host_path_equals_the_reference(name, tag, lname, capsys):
    from vireo_amd import vcf
    gold = np.load(os.path.join(GOLD, name + ".npz"))
    with np.errstate(invalid="ignore"):
        got = vcf.load_donor_GPb(os.path.join(GOLD, name + ".vcf.gz"), tag, [str(x) for x in gold["list_" + lname]],
                                 force_host=True)
    assert got["path"] == "host" and got["reason"] == "forced" and got["n_repaired"] == 0
    check_fixture(got, gold, tag, lname)
    assert capsys.readouterr().out == ""


def test_host_path_is_the_composition(monkeypatch):
    """keep / line are match_SNPs', min_prob reaches parse_donor_GPb, variants=None is the whole file, and
    VIREO_DONOR_VCF=host forces the path like force_host"""
    from vireo_amd import vcf
    path = os.path.join(GOLD, "plain.vcf.gz")
    ids = [str(x) for x in np.load(os.path.join(GOLD, "plain.npz"))["list_shuffled"]]
    v = vcf.load_VCF(path, biallelic_only=True, sparse=False, format_list=["PL"])
    mm = vcf.match_SNPs(ids, v["variants"])
    keep = np.where(mm != None)[0]                                   # noqa: E711
    monkeypatch.setenv("VIREO_DONOR_VCF", "host")
    got = vcf.load_donor_GPb(path, "PL", ids, min_prob=0.01)
    assert got["path"] == "host"
    assert np.array_equal(got["keep"], keep) and np.array_equal(got["line"], mm[keep].astype(int))
    want = vcf.parse_donor_GPb([v["GenoINFO"]["PL"][x] for x in mm[keep]], "PL", 0.01)
    assert got["GPb"].tobytes() == want.tobytes()
    whole = vcf.load_donor_GPb(path, "PL", None)
    assert whole["GPb"].tobytes() == vcf.parse_donor_GPb(v["GenoINFO"]["PL"], "PL").tobytes()
    assert np.array_equal(whole["keep"], np.arange(len(v["variants"]))) and whole["n_lines"] == len(v["variants"])
    import vireo_amd
    assert vireo_amd.vcf.load_donor_GPb is vireo_amd.vcf_utils.load_donor_GPb
    from vireo_amd import _lib
    for name in ("create", "destroy", "chunk", "begin", "slab", "rows"):
        assert "vrx_vcf_" + name in _lib.SIGNATURES and getattr(_lib.lib(), "vrx_vcf_" + name) is not None
    assert _lib.lib().vrx_vcf_chunk() == 64


def test_gp_digit_rule_equals_float():
    """digits[.digits] with at most 15 significant and 22 fractional digits: the digits as an integer over an exact
    power of ten, one correctly rounded division, is Python's float()"""
    rng = np.random.default_rng(5)
    p10 = np.array([float(10 ** k) for k in range(23)])
    assert all(int(p10[k]) == 10 ** k for k in range(23))          # exactly representable
    texts, ints, fracs = [], [], []
    for _ in range(20000):
        n = int(rng.integers(1, 16))
        digits = "".join(str(x) for x in rng.integers(0, 10, n))
        n_frac = int(rng.integers(0, 23))
        if n_frac == 0:
            text = digits
        elif n_frac >= n:
            text = "0." + "0" * (n_frac - n) + digits
        else:
            text = digits[:n - n_frac] + "." + digits[n - n_frac:]
        texts.append(text)
        ints.append(int(digits))
        fracs.append(n_frac)
    assert max(ints) < 10 ** 15
    got = np.array(ints, dtype=np.float64) / p10[np.array(fracs)]
    want = np.array([float(t) for t in texts])
    assert got.tobytes() == want.tobytes()
    assert np.array(texts, dtype=float).tobytes() == want.tobytes()  # what the vectorised host parser does


def test_pl_table_equals_the_reference_expression():
    """table[v - min] with table = 10 ** (-0.1 * arange(4096) - 0.025) is the reference's per-code expression,
    wherever the element stands in NumPy's array power"""
    rng = np.random.default_rng(6)
    table = 10 ** (-0.1 * np.arange(4096.) - 0.025)
    for d in range(4096):                                            # every entry as the reference forms it
        phred = np.array([str(d + 3), "3", str(4095 if d % 2 else 3)], float)
        if d + 3 > 4095:
            phred = np.array([str(d), "0", "0"], float)
        want = 10 ** (-0.1 * (phred - min(phred)) - 0.025)
        lo = int(min(phred))
        assert table[[int(x) - lo for x in phred]].tobytes() == want.tobytes()
    vals = rng.integers(0, 4096, (3003, 3)).astype(float)          # and in one long array, as parse_donor_GPb's
    big = 10 ** (-0.1 * (vals - vals.min(axis=1, keepdims=True)) - 0.025)   # vectorised path forms them
    assert table[(vals - vals.min(axis=1, keepdims=True)).astype(int)].tobytes() == big.tobytes()
    assert np.float64(1 / 3).tobytes() == np.array([0x3FD5555555555555], dtype=np.uint64).tobytes()


def test_resolve_donors_uses_the_reader(tmp_path, monkeypatch, capsys):
    """the command's donor step: the same lines, the filtered cell data and where the path is kept"""
    from scipy.sparse import csc_matrix
    from vireo_amd import vireo
    gold = np.load(os.path.join(GOLD, "chr.npz"))
    ids = [str(x) for x in gold["list_other_side"]]
    monkeypatch.setenv("VIREO_DONOR_VCF", "host")
    opts = vireo.build_parser().parse_args(["-c", "x", "-d", os.path.join(GOLD, "chr.vcf.gz"), "-t", "GP"])[0]
    cell = dict(AD=csc_matrix(np.arange(len(ids) * 2).reshape(len(ids), 2)), variants=list(ids),
                FixedINFO=dict(POS=[x.split("_")[1] for x in ids]))
    cell["DP"] = cell["AD"] * 2
    with np.errstate(invalid="ignore"):
        out, donors = vireo.resolve_donors(opts, cell)
    keep = gold["GP_other_side_keep"]
    assert capsys.readouterr().out == ("[vireo] Loading donor VCF file ...\n[vireo] %d out %d variants matched to donor "
                                       "VCF\n" % (len(keep), len(ids)))
    assert out["variants"] == [ids[x] for x in keep] and out["FixedINFO"]["POS"] == [ids[x].split("_")[1] for x in keep]
    assert np.array_equal(out["AD"].toarray(), np.arange(len(ids) * 2).reshape(len(ids), 2)[keep])
    assert donors["GPb"].tobytes() == gold["GP_other_side_GPb"].tobytes()
    assert donors["names"] == list(gold["GP_other_side_samples"]) and donors["learn_GT"] is False
    assert vireo.DONOR_LOAD["path"] == "host" and vireo.DONOR_LOAD["reason"] == "forced"
    # no match at all: the warning, then the failure
    cell = dict(AD=csc_matrix(np.ones((7, 2))), DP=csc_matrix(np.ones((7, 2))),
                variants=[str(x) for x in gold["list_nomatch"]], FixedINFO={})
    with pytest.raises(SystemExit):
        vireo.resolve_donors(opts, cell)
    assert capsys.readouterr().out == ("[vireo] Loading donor VCF file ...\n[vireo] warning: no variants matched to donor "
                                       "VCF, please check chr format!\nError: No matching variants found between cell "
                                       "data and donor VCF.\n")
