"""SNP-to-gene matching and gene-level counts (snp_gene_match / gene_counts, vrx_genematch.h).

Matching shapes, SNPs x genes over 24 chromosomes (chromosome sizes proportional to 1 .. 24 reversed, genes of
log-uniform length 1 kb .. 300 kb, SNPs uniform, input grouped by chromosome as a VCF is), default gaps:
  1e6x20000, 7.4e6x60000
Aggregation shape:
  c3x20000        the c3 counts of vireo_amd.synth (100 000 variants x 50 000 cells, ~1e8 entries) onto 20 000 genes,
                  every variant in one gene, a tenth in two
Per shape, after a warm-up call, the median over the repeats of
  kernel_ms       hipEvents around the kernels of the call(s)
  device_path_s   host clock around prepare + match_prepared: codes, grouping, upload, both passes, download of
                  flags, counts and rows (arrays only)                                   [matching]
  wall_s          host clock around the public function, transfers and the Python lists / SciPy matrices included
Baselines: matching -- the NumPy restatement of the reference's loop (tests/genematch_np.match_rows), timed ONCE on
SUBSET evenly spaced SNPs and SCALED by the number of SNPs (host_scaled_from_subset); the device's answers on that
subset must equal it.  Aggregation -- the two SciPy products G @ AD, G @ DP (CSR G, CSC counts), G given; the
result must equal the device's.
One JSON line; --out FILE writes it too (profiles/genematch_bench.json).

    python tests/perf/genematch_bench.py [--reps R] [--shapes 1e6x20000,7.4e6x60000,c3x20000] [--out FILE]
"""
import json
import os
import sys
import time

import numpy as np
from scipy.sparse import csc_matrix

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from vireo_amd import _lib, gene_counts, snp_gene_match              # noqa: E402
from vireo_amd import gene_match as GM                               # noqa: E402
from vireo_amd import synth                                          # noqa: E402
from tests import genematch_np as GN                                 # noqa: E402

SUBSET = 400
MATCH = {"1e6x20000": (1_000_000, 20_000), "7.4e6x60000": (7_400_000, 60_000)}
COUNT = {"c3x20000": ("c3", 20_000)}


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def match_case(seed, n_snp, n_gene, n_chrom=24):
    rng = np.random.default_rng(seed)
    w = np.arange(n_chrom, 0, -1, dtype=np.float64)
    size = (w / w[0] * 2.4e8).astype(np.int64)
    gc = np.sort(rng.choice(n_chrom, n_gene, p=w / w.sum()))
    start = (rng.random(n_gene) * size[gc]).astype(np.int64)
    stop = start + np.exp(rng.uniform(np.log(1e3), np.log(3e5), n_gene)).astype(np.int64)
    sc = np.sort(rng.choice(n_chrom, n_snp, p=w / w.sum()))
    pos = (rng.random(n_snp) * size[sc]).astype(np.int64)
    label = np.array(["chr%d" % (c + 1) for c in range(n_chrom)])
    genes = dict(chrom=label[gc], start=start, stop=stop, gene=GN.gene_names(n_gene))
    return dict(CHROM=label[sc], POS=pos), genes


def bench_match(spec, reps):
    n_snp, n_gene = MATCH[spec]
    var, genes = match_case(1, n_snp, n_gene)
    wall, path, kern = [], [], []
    for r in range(reps + 1):                                        # the first round is a warm-up
        t = time.perf_counter()
        gene_list, flag_list = snp_gene_match(var, genes)
        w = time.perf_counter() - t
        tm = {}
        t = time.perf_counter()
        p = GM.prepare(var["CHROM"], var["POS"], genes["chrom"], genes["start"], genes["stop"])
        flag, ptr, rows = GM.match_prepared(p, timing=tm)
        d = time.perf_counter() - t
        assert flag.tolist() == flag_list
        if r:
            wall.append(w)
            path.append(d)
            kern.append(tm["kernel_ms"])
    sub = np.unique(np.linspace(0, n_snp - 1, SUBSET).astype(int))
    t = time.perf_counter()
    flags, want = GN.match_rows(var["CHROM"][sub], var["POS"][sub], genes["chrom"], genes["start"], genes["stop"])
    host_s = (time.perf_counter() - t) * n_snp / sub.size
    assert flags == flag[sub].tolist()
    assert all(np.array_equal(rows[ptr[i]:ptr[i + 1]], w_) for i, w_ in zip(sub, want))
    per_chrom = np.bincount(p["code"], minlength=p["n_code"]) * np.diff(p["chrom_ptr"])
    med_k = float(np.median(kern))
    return dict(shape=spec, n_snp=n_snp, n_gene=n_gene, n_chrom=24, reps=reps, listed=int(ptr[-1]),
                flags=np.bincount(flag, minlength=5).tolist(), pair_evaluations_per_walk=float(per_chrom.sum()),
                kernel_ms=med_k, device_path_s=float(np.median(path)),
                wall_s=dict(median=float(np.median(wall)), min=float(min(wall)), max=float(max(wall))),
                host_restatement_s=host_s, host_scaled_from_subset=[int(sub.size), n_snp],
                speedup_wall_vs_host_restatement=host_s / float(np.median(wall)),
                speedup_device_path_vs_host_restatement=host_s / float(np.median(path)),
                speedup_kernel_vs_host_restatement=host_s / (med_k * 1e-3))


def bench_count(spec, reps):
    cfg, n_gene = COUNT[spec]
    wl = synth.donor_workload(*synth.CONFIGS[cfg], seed=0)
    n_var, n_cell = wl["shape"]
    AD = csc_matrix((wl["ad"].astype(np.int64), wl["rowidx"], wl["colptr"]), shape=(n_var, n_cell))
    DP = csc_matrix((wl["dp"].astype(np.int64), wl["rowidx"].copy(), wl["colptr"].copy()), shape=(n_var, n_cell))
    rng = np.random.default_rng(2)
    names = GN.gene_names(n_gene)
    first = rng.integers(0, n_gene, n_var)
    second = (first + 1 + rng.integers(0, n_gene - 1, n_var)) % n_gene
    two = rng.random(n_var) < 0.1
    lists = [names[[a, b]] if t else names[[a]] for a, b, t in zip(first, second, two)]
    wall, kern = [], []
    for r in range(reps + 1):
        tm = {}
        t = time.perf_counter()
        A, D, got_names = gene_counts(AD, DP, lists, gene_names=names, timing=tm)
        w = time.perf_counter() - t
        if r:
            wall.append(w)
            kern.append(tm["kernel_ms"])
    G = GN.gene_matrix(lists, names, n_var)
    t = time.perf_counter()
    wA, wD = csc_matrix(G @ AD), csc_matrix(G @ DP)
    scipy_s = time.perf_counter() - t
    for got, want in ((A, wA), (D, wD)):
        want.eliminate_zeros()
        want.sort_indices()
        assert got.shape == want.shape and got.nnz == want.nnz and (got != want).nnz == 0
    med = float(np.median(wall))
    return dict(shape=spec, n_var=n_var, n_cell=n_cell, n_gene=n_gene, entries=int(DP.nnz), reps=reps,
                pairs=int(DP.nnz + np.bincount(wl["rowidx"], minlength=n_var)[two].sum()), out_nnz=int(D.nnz),
                kernel_ms=float(np.median(kern)), wall_s=dict(median=med, min=float(min(wall)), max=float(max(wall))),
                scipy_products_s=scipy_s, speedup_wall_vs_scipy=scipy_s / med,
                speedup_kernel_vs_scipy=scipy_s / (float(np.median(kern)) * 1e-3))


def main():
    reps = int(arg("--reps", 3))
    shapes = arg("--shapes", ",".join(list(MATCH) + list(COUNT))).split(",")
    _lib.require_gpu()
    rows = [bench_match(s, reps) if s in MATCH else bench_count(s, reps) for s in shapes]
    out = dict(workload="snp_gene_match (default gaps, multi_gene) and gene_counts, inputs on the host",
               device=_lib.device_info(0)["name"], shapes=rows)
    line = json.dumps(out)
    print(line)
    if "--out" in sys.argv:
        with open(arg("--out", ""), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
