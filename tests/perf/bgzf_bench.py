"""Inflating BGZF: the device path (vireo_amd/bgzf.py, csrc/vrx_bgzf.h) against Python's gzip on the same file and
machine, which is what both VCF readers did before and the yardstick of whether the device path is their default.

Inputs: the generators of donor_vcf_bench.py (100000x16 and 1000000x16 donors) and cell_vcf_bench.py (5000x10000 and
50000x10000 cells), their output written as BGZF: members of 65 280 bytes of text, zlib level 6, and the end-of-file
member.  Per case, after one warm-up, medians over the repeats (and the spread, max - min) of

  gzip_s      gzip.open(path).read(8 MiB) to the end: the parent's inflation
  threads_s   zlib.decompressobj per member on a pool of 16 threads (in this script only, for the record)
  device_s    bgzf.BgzfReader(path).read(8 MiB) to the end, with the median of its scan / upload / kernels / download
              split and the kernels' GB/s of text
  readers     load_donor_GPb (tag GT, every second variant matched) or read_cellVCF end to end under
              VIREO_INFLATE=host (before) and VIREO_INFLATE=device (after), with their seconds['inflate']

The text of all three inflaters is compared once per case.  ``device_faster``: device_s + its spread < gzip_s - its
spread; ``default_rule`` at the end: true iff that holds for every case measured.  One JSON line; --out FILE writes it
too (profiles/bgzf_bench.json).

    python tests/perf/bgzf_bench.py [--reps 3] [--cases d100000x16,d1000000x16,c5000x10000,c50000x10000] [--out FILE]
"""
import gzip
import json
import os
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vireo_amd                                                     # noqa: E402
from vireo_amd import _lib, bgzf, vcf                                # noqa: E402
from tests import bgzf_util                                          # noqa: E402
import cell_vcf_bench                                                # noqa: E402
import donor_vcf_bench                                               # noqa: E402

THREADS = 16
MEMBER_TEXT = 65280
READ = 8 << 20


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


class BgzfWriter:
    """what the generators take for gzip.open(path, "wb"): the bytes written come out as BGZF members"""

    def __init__(self, path, level):
        self.fh, self.level, self.buf = open(path, "wb"), level, bytearray()
        self.pool = ThreadPoolExecutor(THREADS)

    def _member(self, text):
        c = zlib.compressobj(self.level, zlib.DEFLATED, -15, 9)
        return bgzf_util.member(c.compress(text) + c.flush(), text)

    def _drain(self, everything):
        n = len(self.buf) if everything else len(self.buf) // MEMBER_TEXT * MEMBER_TEXT
        texts = [bytes(self.buf[i:i + MEMBER_TEXT]) for i in range(0, n, MEMBER_TEXT)]
        del self.buf[:n]
        for m in self.pool.map(self._member, texts):
            self.fh.write(m)

    def write(self, data):
        self.buf += data
        if len(self.buf) >= 256 * MEMBER_TEXT:
            self._drain(False)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self._drain(True)
        self.fh.write(bgzf_util.EOF_MEMBER)
        self.fh.close()
        self.pool.shutdown()


class _AsBgzf:
    @staticmethod
    def open(path, mode, compresslevel=6):
        assert mode == "wb"
        return BgzfWriter(path, compresslevel)


def read_all(fh):
    parts = []
    while True:
        part = fh.read(READ)
        if not part:
            return parts
        parts.append(part)


def by_gzip(path):
    with gzip.open(path, "rb") as fh:
        return read_all(fh)


def by_threads(path, pool):
    with open(path, "rb") as fh:
        image = fh.read()
    spans = bgzf_util.split_members(image)

    def one(span):
        return zlib.decompressobj(-15).decompress(image[span[1]:span[2]])
    return list(pool.map(one, spans))


def by_device(path):
    with bgzf.BgzfReader(path) as r:
        return read_all(r)


def timed(fn, reps):
    walls, extra, got = [], [], None
    for rep in range(reps + 1):                                      # the first call is the warm-up
        got = None
        t0 = time.perf_counter()
        got = fn()
        wall = time.perf_counter() - t0
        if rep:
            walls.append(wall)
            extra.append(bgzf.last())
    return float(np.median(walls)), float(max(walls) - min(walls)), extra, got


def main():
    reps = int(arg("--reps", "3"))
    cases = arg("--cases", "d100000x16,d1000000x16,c5000x10000,c50000x10000").split(",")
    out = arg("--out", None)
    _lib.require_gpu()
    result = dict(device=_lib.device_info(0)["name"], host_cpus=THREADS, reps=reps, member_text=MEMBER_TEXT, level=6,
                  default_in_tree=bgzf.DEFAULT, cases={})
    donor_vcf_bench.gzip = cell_vcf_bench.gzip = _AsBgzf               # the generators write BGZF
    pool = ThreadPoolExecutor(THREADS)
    with tempfile.TemporaryDirectory() as tmp:
        for case in cases:
            a, b = (int(x) for x in case[1:].split("x"))
            path = os.path.join(tmp, case + ".vcf.gz")
            if case[0] == "d":
                cells, raw = donor_vcf_bench.make_file(path, a, b)
                reader = lambda: vcf.load_donor_GPb(path, "GT", cells)          # noqa: E731
            else:
                raw, _ = cell_vcf_bench.make_files(path, os.path.join(tmp, "head.vcf.gz"), a, b, 1)
                reader = lambda: vireo_amd.read_cellVCF(path)                   # noqa: E731
            assert bgzf.is_bgzf(path)
            print("%s: written" % case, file=sys.stderr, flush=True)
            gzip_s, gzip_spread, _, text = timed(lambda: by_gzip(path), reps)
            crc, n_text = 0, 0
            for part in text:
                crc, n_text = zlib.crc32(part, crc), n_text + len(part)
            del text
            threads_s, threads_spread, _, text = timed(lambda: by_threads(path, pool), reps)
            check = 0
            for part in text:
                check = zlib.crc32(part, check)
            assert check == crc
            del text
            device_s, device_spread, recs, text = timed(lambda: by_device(path), reps)
            check = 0
            for part in text:
                check = zlib.crc32(part, check)
            assert check == crc and all(r["path"] == "device" for r in recs)
            del text
            split = {k: float(np.median([r["seconds"][k] for r in recs])) for k in recs[0]["seconds"]}
            entry = dict(text_bytes=n_text, gz_bytes=os.path.getsize(path), members=recs[0]["members"],
                         gzip_s=gzip_s, gzip_spread_s=gzip_spread, threads_s=threads_s, threads_spread_s=threads_spread,
                         device_s=device_s, device_spread_s=device_spread, device_seconds=split,
                         kernel_gb_per_s=n_text / split["kernels"] / 1e9,
                         device_faster=bool(device_s + device_spread < gzip_s - gzip_spread), readers={})
            assert n_text >= raw
            for mode in ("host", "device"):
                os.environ["VIREO_INFLATE"] = mode
                wall, spread, recs, got = timed(reader, reps)
                assert got["path"] == "device" and all(r["path"] == mode for r in recs), (got["reason"], recs[-1])
                entry["readers"][mode] = dict(wall_s=wall, spread_s=spread, seconds=got["seconds"])
                del got
            del os.environ["VIREO_INFLATE"]
            result["cases"][case] = entry
            print("%s: %.0f MB of text; gzip %.3f s, %d threads %.3f s, device %.3f s (kernels %.3f s, %.2f GB/s); "
                  "reader %.3f s -> %.3f s" % (case, n_text / 1e6, gzip_s, THREADS, threads_s, device_s, split["kernels"],
                                               entry["kernel_gb_per_s"], entry["readers"]["host"]["wall_s"],
                                               entry["readers"]["device"]["wall_s"]), file=sys.stderr, flush=True)
            os.remove(path)
            result["default_rule"] = all(c["device_faster"] for c in result["cases"].values())
            if out:                                                  # (after every case: a long run leaves what it has)
                with open(out, "w") as fh:
                    fh.write(json.dumps(result) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
