"""The BGZF decoder on the CPU, before it runs on a GPU: zlib judges the helper's crafted streams, vrx_bgzf_scan is held
to the committed fixtures, and the host build of csrc/vrx_bgzf.h (one lane, the same source text as the kernel) runs
as a stand-alone program under AddressSanitizer and UBSan against zlib: on every writer mode, every crafted stream,
the small fixtures whole and a few thousand seeded mutations.  No GPU, nothing loaded into Python but the library's
host-only scan."""
import gzip
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

import __graft_entry__ as entry
from tests import bgzf_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "data")
BGZF_FIXTURES = {                                   # file -> BGZF members (the end-of-file member included)
    os.path.join(DATA, "cells.cellSNP.vcf.gz"): 684,
    os.path.join(DATA, "donors.cellSNP.vcf.gz"): 14,
    os.path.join(DATA, "donors.two.cellSNP.vcf.gz"): 10,
    os.path.join(DATA, "cellSNP_mat", "cellSNP.base.vcf.gz"): 4,
}
SMALL_FIXTURES = [p for p, n in BGZF_FIXTURES.items() if n < 100]
PLAIN_GZIP = os.path.join(ROOT, "tests", "golden", "donor_vcf", "plain.vcf.gz")
N_MUTATIONS_PER_BASE = 300                          # x 11 bases = 3 300


def _read(path):
    with open(path, "rb") as fh:
        return fh.read()


# ---- zlib judges the helper ------------------------------------------------------------------------------------------
def test_zlib_accepts_every_crafted_valid_stream():
    valid, _ = U.crafted()
    assert len(valid) >= 8
    for name, (image, text) in valid.items():
        assert zlib.decompress(image[18:-8], -15) == text, name
        assert gzip.decompress(image) == text, name


def test_zlib_rejects_every_crafted_invalid_stream():
    _, invalid = U.crafted()
    assert len(invalid) >= 16
    for name, (image, bit, deflate_level) in invalid.items():
        assert U.gzip_raises(image), name
        if deflate_level:
            with pytest.raises(zlib.error):
                zlib.decompress(image[18:-8], -15)
        else:                                                    # the stream is sound: the footer or the framing is not
            d = zlib.decompressobj(-15)
            d.decompress(image[18:-8])
            assert d.eof, name


def test_writer_modes_are_what_they_claim():
    text = U.vcf_like(5000, 1)
    first = {mode: U.deflate(text, mode)[0] for mode in U.MODES}
    assert (first["stored"] >> 1) & 3 == 0 and (first["fixed"] >> 1) & 3 == 1 and (first["level6"] >> 1) & 3 == 2
    for mode in U.MODES:
        for n in U.MEMBER_TEXT_LENGTHS:
            t = U.vcf_like(n, n)
            assert gzip.decompress(U.bgzf([t, t[:7]], mode)) == t + t[:7]
    rnd = bytes(np.random.RandomState(1).randint(0, 256, 65280).astype(np.uint8))
    image = U.bgzf([rnd], eof=False)
    assert len(image) > 65300 and gzip.decompress(image) == rnd   # a member just under the format's limit


# ---- vrx_bgzf_scan ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scan():
    entry.build()
    from vireo_amd import bgzf
    return bgzf.scan


def test_scan_counts_the_members_of_the_fixtures(scan):
    for path, members in BGZF_FIXTURES.items():
        s = scan(_read(path))
        with gzip.open(path, "rb") as fh:
            n_text = len(fh.read())
        assert s["status"] == 0 and s["members"] == members, path
        assert int(s["isize"].sum()) == n_text == int(s["out_off"][-1]), path
        assert np.array_equal(np.cumsum(s["isize"]), s["out_off"][1:])
        spans = U.split_members(_read(path))
        assert [a for _, a, _, _ in spans] == s["payload_off"].tolist()
        assert [b - a for _, a, b, _ in spans] == s["payload_len"].tolist()


def test_scan_names_what_is_not_bgzf(scan, tmp_path):
    from vireo_amd import bgzf
    image = _read(os.path.join(DATA, "donors.cellSNP.vcf.gz"))
    spans = U.split_members(image)
    assert scan(_read(PLAIN_GZIP))["status"] == 1 and not bgzf.is_bgzf(PLAIN_GZIP)
    plain = gzip.compress(b"##fileformat=VCFv4.2\n")
    assert scan(plain)["status"] == 1
    cut = scan(image[:spans[3][2] - 5])                              # cut in the middle of the fourth member
    assert cut["status"] == 2 and cut["members"] == 3
    assert scan(image[:spans[3][0] + 7])["status"] == 2              # cut inside a header
    assert scan(image + b"\x00" * 4)["status"] == 2                  # trailing zeros, fewer than a header
    assert scan(image + b"\x00" * 40)["status"] == 1                 # trailing zeros, more than a header
    named = bytearray(image)                                         # FNAME set in the second member
    named[spans[1][0] + 3] |= 8
    bad = scan(bytes(named))
    assert bad["status"] == 1 and bad["members"] == 1
    extra = bytearray(image)                                         # XLEN says there are further subfields
    extra[spans[0][0] + 10] = 12
    assert scan(bytes(extra))["status"] == 1
    no_eof = scan(image[:spans[-1][0]])                              # a missing end-of-file member is fine
    assert no_eof["status"] == 0 and no_eof["members"] == len(spans) - 1
    assert scan(b"")["status"] == 0 and scan(b"")["members"] == 0
    p = tmp_path / "x.vcf.gz"
    p.write_bytes(image)
    assert bgzf.is_bgzf(str(p))


# ---- the host build of the decoder under sanitizers ------------------------------------------------------------------
def _compilers():
    out = []
    if shutil.which("g++"):
        out.append(shutil.which("g++"))
    for clang in ("/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++"):
        if os.path.exists(clang):
            out.append(clang)
            break
    return out


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """the sanitizer builds of tests/san/bgzf_host.cpp, one per host compiler found"""
    compilers = _compilers()
    assert compilers, "no host compiler"
    d = tmp_path_factory.mktemp("bgzf_san")
    out = []
    for k, cxx in enumerate(compilers):
        exe = str(d / ("bgzf_host_%d" % k))
        # the sanitizer runtimes linked into the program itself (clang's default), so that it runs as it is
        static = ["-static-libasan", "-static-libubsan"] if cxx.endswith("g++") and "clang" not in cxx else []
        subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
                       + static + [os.path.join(ROOT, "tests", "san", "bgzf_host.cpp"), "-o", exe], check=True)
        out.append(exe)
    return out


def run_host(exe, images, workdir):
    """-> per image (scan status, [(member status, text)])"""
    cases, results = os.path.join(workdir, "cases.bin"), os.path.join(workdir, "results.bin")
    with open(cases, "wb") as fh:
        for image in images:
            fh.write(struct.pack("<I", len(image)))
            fh.write(image)
    r = subprocess.run([exe, cases, results], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", "sanitizer log:\n" + r.stderr[-4000:]
    data, at, out = _read(results), 0, []
    for _ in images:
        rc, members = struct.unpack_from("<iI", data, at)
        at += 8
        got = []
        for _ in range(members):
            st, n = struct.unpack_from("<II", data, at)
            at += 8
            got.append((st, data[at:at + n]))
            at += n
        out.append((rc, got))
    assert at == len(data)
    return out


def test_host_decoder_equals_zlib_on_valid_input(programs, tmp_path):
    valid, _ = U.crafted()
    images = [image for image, _ in valid.values()]
    images += [U.bgzf([U.vcf_like(n, n + 1)], mode) for mode in U.MODES for n in U.MEMBER_TEXT_LENGTHS]
    images.append(U.bgzf([bytes(np.random.RandomState(1).randint(0, 256, 65280).astype(np.uint8))]))
    images += [_read(p) for p in SMALL_FIXTURES]
    for exe in programs:
        for image, (rc, got) in zip(images, run_host(exe, images, str(tmp_path))):
            assert rc == 0 and all(st == 0 for st, _ in got), [st for st, _ in got]
            assert b"".join(text for _, text in got) == gzip.decompress(image)


def test_host_decoder_names_every_invalid_stream(programs, tmp_path):
    _, invalid = U.crafted()
    good = U.member(U.deflate(b"neighbour\n"), b"neighbour\n")
    images = [good + image + good for image, _, _ in invalid.values()]
    for exe in programs:
        for (name, (_, bit, _)), (rc, got) in zip(invalid.items(), run_host(exe, images, str(tmp_path))):
            assert rc == 0 and len(got) == 3, name
            assert got[1][0] & bit, (name, got[1][0], bit)
            assert got[0] == got[2] == (0, b"neighbour\n"), name


def check_mutation(mutated, st, text):
    """the rule for a mutated member: a status, or the bytes zlib gives for the same payload (footer recomputed)"""
    if st != 0:
        return
    want = U.zlib_verdict(mutated)
    assert want is not None and text == want, "the decoder accepts what zlib does not, or differs from it"


def mutated_images():
    """(name, offset, mask) -> the mutated member; the footer is zlib's for the mutated payload where zlib accepts it"""
    bases = U.mutation_bases()
    out = {}
    for key in U.seeded_mutations(N_MUTATIONS_PER_BASE) + list(U.DEVICE_MUTATIONS):
        m = U.mutate(bases[key[0]], key[1], key[2])
        want = U.zlib_verdict(m)
        out[key] = m if want is None else U.refoot(m, want)
    return out


def test_host_decoder_on_mutated_payloads(programs, tmp_path):
    images = mutated_images()
    assert len(images) >= 3000
    accepted = 0
    for exe in programs:
        got = run_host(exe, list(images.values()), str(tmp_path))
        for (key, image), (rc, members) in zip(images.items(), got):
            assert rc == 0 and len(members) == 1, key              # (the header and BSIZE are not touched)
            st, text = members[0]
            check_mutation(image, st, text)
            accepted += st == 0
    assert accepted > 0                                            # some mutations leave a stream zlib accepts
    assert all(key in images for key in U.DEVICE_MUTATIONS)


# ---- the CRC scheme --------------------------------------------------------------------------------------------------
def test_crc_scheme_in_numpy_equals_zlib():
    rng = np.random.RandomState(9)
    c = U.CRC_CHUNK
    for n in (0, 1, c - 1, c, c + 1, 65279, 65280, 65536):
        text = bytes(rng.randint(0, 256, n).astype(np.uint8))
        assert U.crc_by_lanes(text) == zlib.crc32(text), n
