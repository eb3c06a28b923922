"""BGZF inflation on the GPU (csrc/vrx_bgzf.h, vireo_amd/bgzf.py): the bytes of ``gzip.decompress``, byte for byte, with
every member's status 0 on everything zlib accepts (tests/test_bgzf_cpu.py shows that it accepts all of it), the named
status for every crafted invalid member and for that member alone, and both VCF readers equal under
VIREO_INFLATE=device and VIREO_INFLATE=host.  Nothing here has a tolerance."""
import gzip
import os
import zlib

import numpy as np
import pytest

from tests import bgzf_util as U
from tests import cellvcf_util

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "data")
CELLS = os.path.join(DATA, "cells.cellSNP.vcf.gz")
DONORS = os.path.join(DATA, "donors.cellSNP.vcf.gz")
FIXTURES = (CELLS, DONORS, os.path.join(DATA, "donors.two.cellSNP.vcf.gz"),
            os.path.join(DATA, "cellSNP_mat", "cellSNP.base.vcf.gz"))


@pytest.fixture(scope="module")
def bgzf():
    import __graft_entry__ as entry
    entry.build()
    from vireo_amd import _lib, bgzf
    _lib.require_gpu()
    return bgzf


def _read(path):
    with open(path, "rb") as fh:
        return fh.read()


def clean(bgzf, image, **kw):
    """inflate() equals gzip, every member's status is 0 and the record says 'device'"""
    with bgzf.BgzfReader(image, **kw) as r:
        text = r.read()
        status = r.statuses
    rec = bgzf.last()
    assert rec["path"] == "device" and rec["reason"] is None
    assert len(status) == rec["members"] == len(U.split_members(image)) and not status.any()
    assert text == gzip.decompress(image)
    return rec


@pytest.mark.parametrize("mode", sorted(U.MODES))
def test_every_writer_mode_at_every_member_length(bgzf, mode):
    texts = [U.vcf_like(n, n + 3) for n in U.MEMBER_TEXT_LENGTHS]
    clean(bgzf, U.bgzf(texts, mode))
    clean(bgzf, U.bgzf(texts[::-1], mode, eof=False))


def test_a_member_of_random_bytes_just_under_the_limit(bgzf):
    rnd = bytes(np.random.RandomState(1).randint(0, 256, 65280).astype(np.uint8))
    clean(bgzf, U.bgzf([rnd, rnd[:100]]))


@pytest.mark.parametrize("members", (1, 2, 63, 64, 65, 300))
def test_member_counts(bgzf, members):
    text = U.vcf_like(members * 211, members)
    image = U.bgzf([text[i * 211:(i + 1) * 211] for i in range(members)], eof=False)
    assert clean(bgzf, image)["members"] == members
    assert bgzf.inflate(image) == text


def test_a_batch_limit_forces_several_batches(bgzf):
    texts = [U.vcf_like(65280, k) for k in range(5)]
    image = U.bgzf(texts, eof=False)
    with bgzf.BgzfReader(image, batch_bytes=2 * 65536) as r:       # batches of 2, 2 and 1 members
        parts = []
        while True:
            part = r.read(100000)
            if not part:
                break
            parts.append(part)
        assert len(r.statuses) == 5 and not r.statuses.any()
    assert b"".join(parts) == b"".join(texts)
    clean(bgzf, image, batch_bytes=65536)                           # one member per batch
    with pytest.raises(Exception):
        bgzf.BgzfReader(image, batch_bytes=1000)


def test_every_crafted_valid_stream(bgzf):
    valid, _ = U.crafted()
    for name, (image, text) in valid.items():
        assert bgzf.inflate(image) == text, name
    clean(bgzf, b"".join(image for image, _ in valid.values()) + U.EOF_MEMBER)


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p) for p in FIXTURES])
def test_committed_fixtures(bgzf, path):
    clean(bgzf, _read(path))
    with gzip.open(path, "rb") as fh:
        assert bgzf.inflate(path) == fh.read()
    assert bgzf.last()["file"] == path and bgzf.is_bgzf(path)


def test_every_crafted_invalid_stream_is_named_and_alone(bgzf):
    _, invalid = U.crafted()
    left, right = U.vcf_like(3000, 1), U.vcf_like(70, 2)
    for name, (image, bit, _) in invalid.items():
        whole = U.member(U.deflate(left), left) + image + U.member(U.deflate(right, "fixed"), right) + U.EOF_MEMBER
        with bgzf.BgzfReader(whole, strict=False) as r:
            text = r.read()
            status = r.statuses.tolist()
        assert status[0] == 0 and status[2] == 0 and status[3] == 0 and status[1] & bit, (name, status, bit)
        assert text[:len(left)] == left and text[-len(right):] == right, name
        with pytest.raises(bgzf.BgzfStatus) as e:
            bgzf.inflate(whole)
        assert "member 1" in e.value.reason, e.value.reason
        rec = bgzf.last()
        assert rec["path"] == "host" and rec["reason"] == e.value.reason


def test_what_is_not_bgzf_is_a_status(bgzf):
    plain = os.path.join(ROOT, "tests", "golden", "donor_vcf", "plain.vcf.gz")
    assert not bgzf.is_bgzf(plain)
    image = _read(DONORS)
    for bad in (_read(plain), image[:len(image) // 2], image + b"\x00" * 30, b""):
        with pytest.raises(bgzf.BgzfStatus):
            bgzf.inflate(bad)
        assert bgzf.last()["path"] == "host"


def test_mutated_payloads_the_host_build_has_passed(bgzf):
    """U.DEVICE_MUTATIONS: the list tests/test_bgzf_cpu.py runs through the sanitizer build of the same source.  A parity
    check of the two builds, one launch: a status, or zlib's bytes."""
    bases = U.mutation_bases()
    images = []
    for name, offset, mask in U.DEVICE_MUTATIONS:
        m = U.mutate(bases[name], offset, mask)
        want = U.zlib_verdict(m)
        images.append(m if want is None else U.refoot(m, want))
    assert 24 <= len(images) <= 60
    with bgzf.BgzfReader(b"".join(images), strict=False) as r:
        text = r.read()
        status = r.statuses.tolist()
    at = 0
    for key, image, st in zip(U.DEVICE_MUTATIONS, images, status):
        n = int.from_bytes(image[-4:], "little")
        if st == 0:
            assert text[at:at + n] == U.zlib_verdict(image), key
        at += n
    assert at == len(text)


# ---- the readers -----------------------------------------------------------------------------------------------------
def same_donor(a, b):
    for k in ("GPb", "keep", "line"):
        assert np.array_equal(a[k], b[k]) and a[k].dtype == b[k].dtype, k
    for k in ("samples", "n_lines", "n_tagged", "n_repaired", "path", "reason"):
        assert a[k] == b[k], k


def outcome(fn):
    try:
        return "ok", fn()
    except (Exception, SystemExit) as e:                              # noqa: BLE001
        return "raise", type(e), str(e)


def test_read_cellVCF_is_the_same_with_either_inflater(bgzf, monkeypatch):
    import vireo_amd
    got = {}
    for mode in ("device", "host"):
        monkeypatch.setenv("VIREO_INFLATE", mode)
        got[mode] = vireo_amd.read_cellVCF(CELLS)
        rec = bgzf.last()
        assert rec["path"] == mode and rec["file"] == CELLS
        assert got[mode]["path"] == "device"                          # (the parser's path, not the inflater's)
    assert bgzf.last()["reason"] == "VIREO_INFLATE=host"
    cellvcf_util.same(got["device"], got["host"])
    assert set(got["device"]) == set(got["host"]) and set(got["device"]["seconds"]) == set(got["host"]["seconds"])


def test_load_donor_GPb_is_the_same_with_either_inflater(bgzf, monkeypatch):
    import vireo_amd
    from vireo_amd.vcf_utils import load_donor_GPb
    cells = vireo_amd.read_cellVCF(CELLS)["variants"]
    for variants in (None, cells):
        got = {}
        for mode in ("device", "host"):
            monkeypatch.setenv("VIREO_INFLATE", mode)
            got[mode] = load_donor_GPb(DONORS, "GT", variants)
            assert bgzf.last()["path"] == mode and bgzf.last()["file"] == DONORS
            assert got[mode]["path"] == "device"
        same_donor(got["device"], got["host"])
        assert set(got["device"]) == set(got["host"])
        assert len(got["device"]["GPb"]) > 0


def test_plain_gzip_stays_on_the_host(bgzf, monkeypatch):
    from vireo_amd.vcf_utils import load_donor_GPb
    plain = os.path.join(ROOT, "tests", "golden", "donor_vcf", "plain.vcf.gz")
    monkeypatch.setenv("VIREO_INFLATE", "device")
    a = load_donor_GPb(plain, "GT", None)
    assert bgzf.last()["path"] == "host" and bgzf.last()["reason"] == "not a BGZF file"
    monkeypatch.setenv("VIREO_INFLATE", "host")
    same_donor(a, load_donor_GPb(plain, "GT", None))


def corrupt(path, out, member=3):
    """a copy with one payload byte of one member flipped, the footers left alone"""
    image = bytearray(_read(path))
    _, a, b, _ = U.split_members(image)[member]
    image[(a + b) // 2] ^= 0x5a
    with open(out, "wb") as fh:
        fh.write(image)
    return out


@pytest.mark.parametrize("which", ("cells", "donors"))
def test_a_corrupt_file_takes_the_host_path_and_raises_as_before(bgzf, monkeypatch, tmp_path, which):
    import vireo_amd
    from vireo_amd.vcf_utils import load_donor_GPb
    if which == "cells":
        bad = corrupt(CELLS, str(tmp_path / "cells.vcf.gz"))
        call = lambda: vireo_amd.read_cellVCF(bad)                    # noqa: E731
    else:
        bad = corrupt(DONORS, str(tmp_path / "donors.vcf.gz"))
        call = lambda: load_donor_GPb(bad, "GT", None)                # noqa: E731
    monkeypatch.setenv("VIREO_INFLATE", "host")
    before = outcome(call)                                            # what the file raises without this feature
    assert before[0] == "raise" and issubclass(before[1], (OSError, EOFError, zlib.error)), before
    monkeypatch.setenv("VIREO_INFLATE", "device")
    after = outcome(call)
    rec = bgzf.last()
    assert rec["path"] == "host" and "member 3" in rec["reason"], rec
    assert after == before, (after, before)


def test_reader_lifecycle(bgzf):
    r = bgzf.BgzfReader(_read(DONORS))
    assert r.read(10) == gzip.decompress(_read(DONORS))[:10] and r.read(0) == b""
    r.close()
    r.close()
    with pytest.raises(ValueError):
        r.read(1)


def test_the_setting_is_checked(bgzf, monkeypatch):
    from vireo_amd.vcf_utils import load_donor_GPb
    monkeypatch.delenv("VIREO_INFLATE", raising=False)
    assert bgzf.wanted() == "device"                                  # the default (profiles/bgzf_bench.json)
    assert load_donor_GPb(DONORS, "GT", None)["path"] == "device" and bgzf.last()["path"] == "device"
    monkeypatch.setenv("VIREO_INFLATE", "gpu")
    with pytest.raises(ValueError):
        load_donor_GPb(DONORS, "GT", None)
