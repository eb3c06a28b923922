"""Reading a donor VCF: load_donor_GPb on the GPU (vrx_vcf.h) against the host composition it replaces
(force_host=True: load_VCF -> match_SNPs -> parse_donor_GPb).

Cases, variants x samples: 100000x16, 1000000x16, 100000x256, each for GT and PL.  The file is generated here:
FORMAT GT:PL, one biallelic SNP per line, gzip level 6; the cell list holds every second variant, shuffled, so half
of the lines match.  Per case and tag, after one warm-up call of each path, the median over the repeats of the
host clock around the call, and for the device path the median of every entry of its ``seconds`` split (inflate,
upload, kernels, download, host).  The two results must be equal bit for bit.  One JSON line; --out FILE writes it
too (profiles/donor_vcf_bench.json).

    python tests/perf/donor_vcf_bench.py [--reps 3] [--cases 100000x16,1000000x16,100000x256] [--tags GT,PL]
                                         [--out FILE]
"""
import gzip
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from vireo_amd import _lib, vcf                                      # noqa: E402

GT = np.array(["0/0", "0/1", "1/1", "./."])


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def make_file(path, n_var, n_sample, seed=1):
    rng = np.random.default_rng(seed)
    head = "##fileformat=VCFv4.2\n#" + "\t".join("CHROM POS ID REF ALT QUAL FILTER INFO FORMAT".split()
                                                  + ["donor%d" % k for k in range(n_sample)]) + "\n"
    ids = []
    raw = 0
    with gzip.open(path, "wb", compresslevel=6) as fh:
        fh.write(head.encode())
        for lo in range(0, n_var, 20000):
            n = min(20000, n_var - lo)
            gt = rng.integers(0, 4, (n, n_sample))
            pl = rng.integers(0, 256, (n, n_sample, 3))
            pl[np.arange(n)[:, None], np.arange(n_sample)[None, :], np.minimum(gt, 2)] = 0
            bases = rng.integers(0, 4, (n, 2))
            out = []
            for i in range(n):
                v = lo + i
                chrom, pos = str(1 + v * 22 // n_var), str(1000 + 10 * v)
                ref, alt = "ACGT"[bases[i, 0]], "ACGT"[bases[i, 1]]
                ids.append("_".join((chrom, pos, ref, alt)))
                fields = ["%s:%d,%d,%d" % (GT[g], a, b, c) for g, (a, b, c) in zip(gt[i], pl[i])]
                out.append("\t".join([chrom, pos, ".", ref, alt, ".", "PASS", "AD=%d;DP=%d" % (bases[i, 0], 40),
                                      "GT:PL"] + fields))
            text = ("\n".join(out) + "\n").encode()
            raw += len(text)
            fh.write(text)
    cells = [ids[k] for k in rng.permutation(np.arange(0, n_var, 2))]
    return cells, raw


def main():
    reps = int(arg("--reps", "3"))
    cases = arg("--cases", "100000x16,1000000x16,100000x256").split(",")
    tags = arg("--tags", "GT,PL").split(",")
    _lib.require_gpu()
    result = dict(device=_lib.device_info(0)["name"], reps=reps, cases={})
    with tempfile.TemporaryDirectory() as tmp:
        for case in cases:
            n_var, n_sample = (int(x) for x in case.split("x"))
            path = os.path.join(tmp, case + ".vcf.gz")
            cells, raw = make_file(path, n_var, n_sample)
            entry = dict(text_bytes=raw, gz_bytes=os.path.getsize(path), matched=len(cells))
            for tag in tags:
                runs = {"device": [], "host": []}
                split = []
                for how in ("device", "host"):
                    for rep in range(reps + 1):                      # the first call is the warm-up
                        t0 = time.perf_counter()
                        got = vcf.load_donor_GPb(path, tag, cells, force_host=how == "host")
                        wall = time.perf_counter() - t0
                        assert got["path"] == how, (got["path"], got["reason"])
                        if rep:
                            runs[how].append(wall)
                            if how == "device":
                                split.append(got["seconds"])
                    if how == "device":
                        dev = got
                assert dev["GPb"].tobytes() == got["GPb"].tobytes() and np.array_equal(dev["keep"], got["keep"])
                assert np.array_equal(dev["line"], got["line"]) and dev["n_repaired"] == 0
                entry[tag] = dict(device_s=float(np.median(runs["device"])), host_s=float(np.median(runs["host"])),
                                  seconds={k: float(np.median([s[k] for s in split])) for k in split[0]},
                                  rows=int(len(dev["keep"])))
                print("%s %s: device %.3f s, host %.3f s" % (case, tag, entry[tag]["device_s"], entry[tag]["host_s"]),
                      file=sys.stderr, flush=True)
            result["cases"][case] = entry
    line = json.dumps(result)
    print(line)
    out = arg("--out", None)
    if out:
        with open(out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
