"""CPU-only: the host paths of both VCF readers (load_donor_GPb and read_cellVCF with force_host=True) against what
the real reference does with the mutation corpus of tests/vcf_mutate.py, recorded in tests/golden/vcf_mutation.npz by
tests/golden/make_vcf_mutation_golden.py.  Every comparison is on the class of the exception or on a SHA-256 over
everything returned: there is no tolerance.  The corpus is regenerated here and its text digests are checked first; the
golden record must show that the reference returns on at least half of each corpus, and seven defects planted into the
host parser must each be caught by a file the test names."""
import contextlib
import inspect
import io
import os

import numpy as np
import pytest

import __graft_entry__ as entry
from tests import vcf_mutate as M

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vcf_mutation.npz")
CASES = {"donor": M.TAGS, "cell": (True, False)}


@pytest.fixture(scope="module", autouse=True)
def built():
    entry.build()


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    """every corpus file written once: {kind: [path]}"""
    tmp = tmp_path_factory.mktemp("vcf_mutation")
    return {kind: [f.write(tmp) for f in M.corpus(kind)] for kind in CASES}


def want(gold, kind, k, c):
    """the reference's record of case c of file k: an exception's class name or the digest"""
    raised = int(gold[kind + "_raised"][k, c])
    return str(gold["classes"][raised]) if raised else gold[kind + "_digest"][k, c].tobytes().hex()


def host(kind, path, f, case):
    """the host path's record of one case, formed like the reference's"""
    from vireo_amd import read_cellVCF, vcf

    def run():
        if kind == "donor":
            r = vcf.load_donor_GPb(path, case, f.cells, force_host=True)
            return M.donor_digest(r["keep"], r["line"], r["GPb"], r["samples"], r["n_lines"], r["n_tagged"])
        r = read_cellVCF(path, biallelic_only=case, force_host=True)
        return M.cell_digest(r["AD"], r["DP"], r["variants"], r["samples"], r["n_SNP_tagged"])
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all="ignore"):
        got = M.outcome(run)
    return got[1]


def misses(gold, paths, kind, first_only=False):
    """[(file name, case, reference, host)] wherever the host path's record is not the reference's"""
    out = []
    for k, f in enumerate(M.corpus(kind)):
        for c, case in enumerate(CASES[kind]):
            ref, got = want(gold, kind, k, c), host(kind, paths[kind][k], f, case)
            if ref != got:
                out.append((f.name, case, ref, got, f.mutations))
                if first_only:
                    return out
    return out


@pytest.mark.parametrize("kind", ("donor", "cell"))
def test_the_corpus_is_the_recorded_one(gold, kind):
    from vireo_amd import _lib
    assert _lib.lib().vrx_vcf_chunk() == M.CHUNK and _lib.lib().vrx_cellvcf_segment() == M.SEGMENT
    files = M.corpus(kind)
    assert len(files) == M.N_FILES == len(gold[kind + "_text"])
    for k, f in enumerate(files):                                   # a NumPy stream that drifted fails here
        assert f.sha256 == gold[kind + "_text"][k].tobytes().hex(), f.name
    again = M.make_file(kind, 7)
    assert again.text == files[7].text and again is not files[7]
    # the generator's guarantees: half of the files field-only, two thirds of the mutations in the sample region,
    # one to three mutations each, every S and the padded lines present, the wide base across one segment boundary
    assert 2 * sum(f.field_only for f in files) >= len(files)
    mutations = [m for f in files for m in f.mutations]
    assert 3 * sum(m[2] == "sample" for m in mutations) >= 2 * len(mutations)
    assert {len(f.mutations) for f in files} == {1, 2, 3}
    assert {f.S for f in files if f.field_only} == set(M.DONOR_S if kind == "donor" else M.CELL_S)
    assert {m[0] for m in mutations} == set(M.BYTE_OPS + M.STRUCT_OPS)
    for f in files:
        assert 12 <= len(f.base_ids) <= 40
        if f.field_only:
            assert all(m[2] == "sample" and M.printable(m[3].encode("latin-1")) and "\t" not in m[3] and
                       m[1] in f.eligible for m in f.mutations)
            assert len(f.lines) == len(f.base_ids) and all(x.count(b"\t") == 8 + f.S for x in f.lines)
    # what the GPU test asks of the field-only files: some stay inside the device's grammar, some leave it
    if kind == "donor":
        for tag in M.TAGS:
            repairs = [M.donor_repairs(f, tag) for f in files if f.field_only]
            assert sum(x > 0 for x in repairs) >= 10 and sum(x == 0 for x in repairs) >= 10, (tag, repairs)
    else:
        repairs = [M.cell_repairs(f) for f in files if f.field_only]
        assert min(sum(x is None for x in repairs), sum(x == 0 for x in repairs)) >= 10, repairs
        assert sum(x is not None and x > 0 for x in repairs) >= 5, repairs
    if kind == "cell":
        wide = [f for f in files if f.S == max(M.CELL_S)]
        regions = [len(x) - len(b"\t".join(x.split(b"\t")[:9])) for f in wide if f.field_only for x in f.lines]
        assert min(regions) > M.SEGMENT and max(regions) <= 2 * M.SEGMENT


@pytest.mark.parametrize("kind", ("donor", "cell"))
def test_the_reference_returns_on_half_of_the_corpus(gold, kind):
    """a comparison of exceptions proves little: on at least half of the files the reference returns in every case"""
    raised = gold[kind + "_raised"]
    assert raised.shape == (M.N_FILES, len(CASES[kind]))
    assert 2 * int((raised == 0).all(axis=1).sum()) >= M.N_FILES
    assert {"IndexError", "ValueError", "UnicodeDecodeError", "UnboundLocalError"} <= set(gold["classes"].tolist())
    if kind == "cell":
        assert "SystemExit" in gold["classes"].tolist()


@pytest.mark.parametrize("kind", ("donor", "cell"))
def test_host_path_is_the_reference_on_every_file(gold, paths, kind):
    bad = misses(gold, paths, kind)
    assert not bad, "%d of %d cases differ, the first: %r" % (len(bad), M.N_FILES * len(CASES[kind]), bad[:3])


# (kind that catches it, [(function, old text, new text)]): each planted into the host parser's own source
DEFECTS = {
    "the blank form accepted with one dot too many": ("cell", [
        ("_sparse_geno", 'if call == blank or call == ".":',
         'if call == blank or call == blank + ":." or call == ".":')]),
    "the value taken after the first comma": ("cell", [
        ("read_sparse_GeneINFO", 'x.split(",")[ax]', 'x.split(",")[min(1, x.count(","))]')]),
    "'.' as a value not read as 0": ("cell", [
        ("read_sparse_GeneINFO", "[v if v != '.' else '0' for v in vals]", "list(vals)")]),
    "the PL minimum taken over the first two values": ("donor", [
        ("_parse_codes_vectorised", "vals.min(axis=1, keepdims=True)", "vals[:, :2].min(axis=1, keepdims=True)"),
        ("_parse_codes_one_by_one", "min(phred)", "min(phred[:2])")]),
    "rstrip() left out": ("cell", [
        ("load_VCF", 'f = line.rstrip().split("\\t")', 'f = line.split("\\t")')]),
    "the biallelic filter looking at REF only": ("cell", [
        ("load_VCF", "(len(f[3]) > 1 or len(f[4]) > 1)", "len(f[3]) > 1")]),
    "GT from code[0] + code[1]": ("donor", [
        ("_parse_codes_vectorised", "code[-1] for code in good", "code[1] for code in good"),
        ("_parse_codes_one_by_one", "float(code[-1])", "float(code[1])")]),
}


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_planted_defects_are_caught(gold, paths, monkeypatch, defect):
    """the corpus has teeth: with the defect in the host parser some file's record is no longer the reference's"""
    import vireo_amd
    from vireo_amd import io_utils, vcf_utils
    kind, edits = DEFECTS[defect]
    assert not misses(gold, paths, kind, first_only=True)
    for name, old, new in edits:
        src = inspect.getsource(getattr(vcf_utils, name))
        assert src.count(old) == 1, (name, old)
        scope = {}
        exec(compile(src.replace(old, new), "<planted: %s>" % defect, "exec"), vcf_utils.__dict__, scope)
        original = getattr(vcf_utils, name)
        for mod in (vcf_utils, io_utils, vireo_amd.vcf):            # wherever the name is bound
            if getattr(mod, name, None) is original:
                monkeypatch.setattr(mod, name, scope[name])
    caught = misses(gold, paths, kind, first_only=True)
    assert caught, defect
    print("%s: caught by %s, case %s (%s instead of %s)" % ((defect,) + caught[0][:2] + (caught[0][3][:16], caught[0][2][:16])))
