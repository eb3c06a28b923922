"""Reading a cell VCF: read_cellVCF on the GPU (vrx_cellvcf.h) against the host composition it replaces
(force_host=True: load_VCF -> read_sparse_GeneINFO).

Cases, variants x cells: 5000x10000, 50000x10000, 2000x100000.  The file is generated here in cellSNP's layout:
FORMAT GT:AD:DP:OTH:PL:ALL, one biallelic SNP per line, about 2 % of the sample fields a call and the rest '.:.:.:.:.:.'
(gzip level 6).  The sample regions are drawn from a pool of 64 random lines, which keeps the generation short; a
line is longer than gzip's window, so the repeats do not help the compression.  Per case, after one warm-up call,
the median over the repeats of the host clock around the device call (inflation included), and the median of every
entry of its ``seconds`` split (inflate, upload, kernels, download, host).  The host path takes minutes at these
sizes: it is timed the same way on a file that holds the first ``host_lines`` lines, and ``host_s`` is that time
scaled by variants / host_lines; both numbers are recorded.  On that smaller file the two paths must return the same
bits.  One JSON line; --out FILE writes it too (profiles/cell_vcf_bench.json).

    python tests/perf/cell_vcf_bench.py [--reps 3] [--cases 5000x10000,50000x10000,2000x100000]
                                        [--host-fields 2000000] [--out FILE]
"""
import gzip
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import vireo_amd                                                     # noqa: E402
from vireo_amd import _lib                                           # noqa: E402

FORMAT = "GT:AD:DP:OTH:PL:ALL"
BLANK = ".:.:.:.:.:."
POOL = 64


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def sample_region(rng, n_cell, rate=0.02):
    fields = [BLANK] * n_cell
    for j in np.flatnonzero(rng.random(n_cell) < rate):
        dp = int(rng.integers(1, 40))
        ad = int(rng.integers(0, dp + 1))
        pl = rng.integers(0, 400, 3)
        fields[j] = "%s:%d:%d:0:%d,%d,%d:%d,%d,0,0,0" % (["0/0", "1/0", "1/1"][int(rng.integers(3))], ad, dp, pl[0], pl[1],
                                                         pl[2], dp - ad, ad)
    return "\t".join(fields)


def make_files(path, head_path, n_var, n_cell, n_head, seed=1):
    """the whole file and one of its first n_head lines -> (text bytes, calls) of the whole file"""
    rng = np.random.default_rng(seed)
    pool = [sample_region(rng, n_cell) for _ in range(POOL)]
    calls = [sum(1 for f in p.split("\t") if f != BLANK) for p in pool]
    head = "##fileformat=VCFv4.2\n##contig=<ID=1>\n#" + "\t".join(
        "CHROM POS ID REF ALT QUAL FILTER INFO FORMAT".split() + ["AAAC%08d-1" % k for k in range(n_cell)]) + "\n"
    raw = n_calls = 0
    with gzip.open(path, "wb", compresslevel=6) as fh, gzip.open(head_path, "wb", compresslevel=6) as hh:
        fh.write(head.encode())
        hh.write(head.encode())
        for v in range(n_var):
            k = int(rng.integers(POOL))
            text = ("\t".join([str(1 + v * 22 // n_var), str(1000 + 10 * v), ".", "ACGT"[v % 4], "CGTA"[v % 4], ".", "PASS",
                               "AD=%d;DP=%d;OTH=0" % (v % 7, 10 + v % 31), FORMAT, pool[k]]) + "\n").encode()
            fh.write(text)
            if v < n_head:
                hh.write(text)
            raw += len(text)
            n_calls += calls[k]
    return raw, n_calls


def timed(path, reps, force_host):
    walls, splits, got = [], [], None
    for rep in range(reps + 1):                                      # the first call is the warm-up
        t0 = time.perf_counter()
        got = vireo_amd.read_cellVCF(path, force_host=force_host)
        wall = time.perf_counter() - t0
        assert got["path"] == ("host" if force_host else "device"), (got["path"], got["reason"])
        if rep:
            walls.append(wall)
            splits.append(got["seconds"])
    return float(np.median(walls)), {k: float(np.median([s[k] for s in splits])) for k in splits[0]}, got


def main():
    reps = int(arg("--reps", "3"))
    cases = arg("--cases", "5000x10000,50000x10000,2000x100000").split(",")
    host_fields = int(arg("--host-fields", "2000000"))
    _lib.require_gpu()
    result = dict(device=_lib.device_info(0)["name"], reps=reps, segment=int(_lib.lib().vrx_cellvcf_segment()), cases={})
    with tempfile.TemporaryDirectory() as tmp:
        for case in cases:
            n_var, n_cell = (int(x) for x in case.split("x"))
            n_head = min(n_var, max(20, host_fields // n_cell))
            path, head_path = os.path.join(tmp, case + ".vcf.gz"), os.path.join(tmp, case + ".head.vcf.gz")
            raw, n_calls = make_files(path, head_path, n_var, n_cell, n_head)
            device_s, split, dev = timed(path, reps, False)
            assert dev["n_repaired"] == 0 and dev["AD"].shape == (n_var, n_cell) and dev["AD"].nnz == n_calls
            head_host_s, _, host = timed(head_path, reps, True)
            head_dev = vireo_amd.read_cellVCF(head_path)
            assert head_dev["path"] == "device", head_dev["reason"]
            for key in ("AD", "DP"):
                for part in ("indptr", "indices", "data"):
                    a, b = getattr(head_dev[key], part), getattr(host[key], part)
                    assert a.dtype == b.dtype and np.array_equal(a, b), (key, part)
                    assert np.array_equal(getattr(dev[key][:n_head], part), b), (key, part)
            assert head_dev["variants"] == host["variants"] == dev["variants"][:n_head]
            result["cases"][case] = dict(
                text_bytes=raw, gz_bytes=os.path.getsize(path), sample_fields=n_var * n_cell, calls=n_calls,
                device_s=device_s, seconds=split, inflate_share=split["inflate"] / device_s,
                host_lines=n_head, host_lines_s=head_host_s, host_s=head_host_s * n_var / n_head)
            print("%s: device %.3f s (inflate %.3f s), host %.1f s scaled from %d lines in %.3f s"
                  % (case, device_s, split["inflate"], head_host_s * n_var / n_head, n_head, head_host_s),
                  file=sys.stderr, flush=True)
            del dev, host, head_dev
    line = json.dumps(result)
    print(line)
    out = arg("--out", None)
    if out:
        with open(out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
