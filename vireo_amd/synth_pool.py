"""Synthetic pools of several samples with known truth: the matrix-level counterpart of simulate/synth_pool.py.

    python -m vireo_amd.synth_pool -c DIR1,DIR2,... -o OUT_DIR [-b FILE1,FILE2,...] [-d RATE]
                                   [--nCELL N] [--minorSAMPLE F] [--randomSEED S]

The reference pools BAM files: it draws the cells of every sample, renames them to pooled barcodes, joins pairs
of them into doublets, and rewrites each read's cell tag to the pooled barcode (synth_pool.py:126-141); cellSNP
then piles the pooled BAM up again.  Pile-up is additive over reads, so on a fixed variant list the counts of a
pooled cell are the sum of the count columns of its source cells, and the BAM step is not needed: the pooled
matrices are a sparse column merge of the samples' matrices (``pool_counts``, on the GPU: csrc/vrx_pool.h).

The barcode logic (``sample_barcodes``, ``pool_barcodes``) is the reference's, draw for draw on NumPy's legacy
global generator, and writes the same barcodes_pool.tsv and cell_info.tsv.  ``pool_plan`` turns its result into
the column plan, ``PoolPlan.truth`` into the labels a demultiplexer is scored against
(``vireo_amd.get_confusion``).

-c takes cellSNP folders where the reference's -s takes BAM files; -b defaults to each folder's
cellSNP.samples.tsv.  The folders must list the same variants (CHROM, POS, REF, ALT, in order).  Written to
OUT_DIR: barcodes_pool.tsv, cell_info.tsv, cellSNP.samples.tsv (equal to barcodes_pool.tsv),
cellSNP.tag.AD.mtx, cellSNP.tag.DP.mtx and cellSNP.base.vcf.gz -- the first folder's file, byte for byte, so
the AD / DP / OTH totals of its INFO column are those of that sample, not of the pool.

Out of scope: intersecting differing variant lists, the OTH matrix, and applying cellSNP's count / MAF filters
again to the pooled counts.  One deviation from the reference: a pooled barcode with three or more source cells
(two cells of one sample that share a pooled name both heading doublets) is a ValueError; a BAM-level pool would
merge them silently.
"""
import ctypes as C
import itertools
import os
import shutil
import sys
from optparse import OptionGroup, OptionParser

import numpy as np
from scipy.sparse import csc_matrix

from . import _lib

_I32P = C.POINTER(C.c_int32)
_I64P = C.POINTER(C.c_int64)


# ---- barcodes --------------------------------------------------------------------------------------

def sample_barcodes(barcodes, n_cell_each=1000, minor_sample=1.0, seed=None):
    """Down-sample every sample to n_cell_each barcodes and the first one to round(minor_sample * n_cell_each)
    (what synth_pool.py:23-36 does): one ``np.random.permutation`` per sample on the legacy global generator,
    reseeded when seed is given; a sample keeps the cells its permutation names first.  Like the reference it
    replaces the entries of the list ``barcodes`` and returns that list.  A sample with fewer barcodes than
    n_cell_each is a ValueError (the reference prints and exits); it is raised before anything is drawn."""
    short = [k for k, cells in enumerate(barcodes) if len(cells) < n_cell_each]
    if short:
        raise ValueError("sample_barcodes: sample %d has %d cell barcodes, fewer than n_cell_each = %d"
                         % (short[0] + 1, len(barcodes[short[0]]), n_cell_each))
    if seed is not None:
        np.random.seed(seed)
    keep = [n_cell_each] * len(barcodes)
    if keep:
        keep[0] = min(n_cell_each, round(minor_sample * n_cell_each))
    for k, cells in enumerate(barcodes):
        order = np.random.permutation(len(cells))
        barcodes[k] = [cells[j] for j in order[:n_cell_each][:keep[k]]]
    return barcodes


def _sample_tag(name):
    """what follows the first "-" of a barcode (up to the next one)"""
    fields = name.split("-")
    if len(fields) < 2:
        raise ValueError("pool_barcodes: barcode %r has no '-'" % (str(name),))
    return fields[1]


def _write_lines(path, lines):
    with open(path, "w") as f:
        f.write("".join(ln + "\n" for ln in lines))


def pool_barcodes(barcodes, out_dir=None, doublet_rate=None, sample_suffix=True, seed=None):
    """Pooled barcodes of every sample's cells, with doublets (what synth_pool.py:39-95 does) -> a list per sample.

    With sample_suffix the last character of a barcode is replaced by the sample number (1, 2, ..., two digits
    from sample 10 on).  doublet_rate None means n_cells / 100000.  Of one ``np.random.permutation`` of all cells
    the first round(n_cells / (1 + 1 / rate)) are each paired with the cell that many places on; both take the first
    one's name plus "S" when the text after the first "-" is equal for the two, else "D".  With out_dir,
    barcodes_pool.tsv (``np.unique`` of all names) and cell_info.tsv (pooled name, original name, sample number)
    are written there, byte for byte as the reference writes them; without, nothing is written.  A rate outside
    [0, 1] and a doublet member without "-" are ValueErrors."""
    if seed is not None:
        np.random.seed(seed)
    sizes = [len(cells) for cells in barcodes]
    origin = [name for cells in barcodes for name in cells]
    sample = np.repeat(np.arange(1, len(sizes) + 1), sizes).tolist()
    pooled = [name[:-1] + str(k) for name, k in zip(origin, sample)] if sample_suffix else list(origin)
    n_cells = len(pooled)
    if doublet_rate is not None and not 0 <= doublet_rate <= 1:
        raise ValueError("pool_barcodes: doublet rate needs to be between 0 and 1, got %r" % (doublet_rate,))
    rate = n_cells / 100000.0 if doublet_rate is None else doublet_rate
    n_pair = round(n_cells / (1 + 1 / rate)) if rate != 0 else 0
    if 2 * n_pair > n_cells:
        raise ValueError("pool_barcodes: %d doublets need more than the %d cells" % (n_pair, n_cells))
    order = np.random.permutation(n_cells)
    for head, mate in zip(order[:n_pair].tolist(), order[n_pair:2 * n_pair].tolist()):
        same = _sample_tag(pooled[head]) == _sample_tag(pooled[mate])
        pooled[head] = pooled[mate] = pooled[head] + ("S" if same else "D")
    if out_dir is not None:
        _write_lines(os.path.join(out_dir, "barcodes_pool.tsv"), np.unique(pooled).tolist())
        _write_lines(os.path.join(out_dir, "cell_info.tsv"), ["CB_pool\tCB_origin\tSample_id"] + [
            "%s\t%s\t%d" % row for row in zip(pooled, origin, sample)])
    ends = np.cumsum(sizes).tolist()
    return [pooled[e - n:e] for e, n in zip(ends, sizes)]


# ---- the plan ---------------------------------------------------------------------------------------

class PoolPlan:
    """Which source cells make up every pooled cell.

    barcodes     pooled barcodes, one per pooled cell (``np.unique`` order: the lines of barcodes_pool.tsv)
    src0, src1   int32 per pooled cell: its first source cell, and its second or -1; source cells are numbered
                 sample after sample in each sample's barcode order (the rows of cell_info.tsv)
    sizes        source cells per sample
    sample       int per source cell: its sample, counted from 1 like Sample_id of cell_info.tsv
    A pooled column is the sum of ALL source cells that carry its barcode, doublet or not: two cells of one
    sample that end up with the same pooled name are one cell of the pool, as they would be after a BAM merge."""

    def __init__(self, barcodes, src0, src1, sizes):
        self.barcodes = np.asarray(barcodes)
        self.src0 = np.ascontiguousarray(src0, dtype=np.int32).reshape(-1)
        self.src1 = np.ascontiguousarray(src1, dtype=np.int32).reshape(-1)
        self.sizes = [int(n) for n in sizes]
        self.n_src = int(sum(self.sizes))
        self.sample = np.repeat(np.arange(1, len(self.sizes) + 1), self.sizes)
        n = self.src0.size
        if self.src1.size != n or self.barcodes.shape != (n,):
            raise ValueError("PoolPlan: barcodes, src0 and src1 must have one entry per pooled cell")
        if n and (self.src0.min() < 0 or self.src0.max() >= self.n_src or self.src1.min() < -1
                  or self.src1.max() >= self.n_src):
            raise ValueError("PoolPlan: a source cell outside [0, %d)" % self.n_src)

    @property
    def n_pool(self):
        return int(self.src0.size)

    def subset(self, idx):
        """the plan of the pooled cells idx alone, on the same source cells"""
        idx = np.asarray(idx, dtype=np.int64).reshape(-1)
        return PoolPlan(self.barcodes[idx], self.src0[idx], self.src1[idx], self.sizes)

    def matrix(self):
        """P, 0/1 int64 CSC of shape (source cells, pooled cells): the pooled counts are ``X_all @ P``"""
        two = self.src1 >= 0
        cols = np.concatenate([np.arange(self.n_pool), np.flatnonzero(two)])
        rows = np.concatenate([self.src0, self.src1[two]]).astype(np.int64)
        P = csc_matrix((np.ones(rows.size, dtype=np.int64), (rows, cols)), shape=(self.n_src, self.n_pool))
        return P

    def truth(self):
        """per pooled cell: its sample number as a string, or "doublet" when its two source cells come from
        different samples (a pair from one sample -- the reference's "S" tag -- is genetically a singlet)"""
        one = self.sample[self.src0] if self.n_pool else np.zeros(0, dtype=np.int64)
        two = self.sample[np.maximum(self.src1, 0)] if self.n_pool else one
        mixed = (self.src1 >= 0) & (one != two)
        out = one.astype(str).astype(object)
        out[mixed] = "doublet"
        return np.array(out, dtype=str) if self.n_pool else np.zeros(0, dtype=str)


def pool_plan(barcodes_in, barcodes_out):
    """The column plan of a pool: barcodes_in the source barcodes per sample, barcodes_out what
    ``pool_barcodes`` made of them -> PoolPlan.  The device path adds one or two source columns per pooled
    cell; a pooled barcode carried by three or more source cells is a ValueError naming it."""
    sizes = [len(b) for b in barcodes_in]
    if len(barcodes_out) != len(sizes) or any(len(o) != n for o, n in zip(barcodes_out, sizes)):
        raise ValueError("pool_plan: barcodes_in and barcodes_out differ in their numbers of samples or cells")
    flat = np.array(list(itertools.chain(*barcodes_out)), dtype=str)
    names, inv, count = np.unique(flat, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    if count.size and count.max() > 2:
        raise ValueError("pool_plan: pooled barcode %r has %d source cells; at most two can be pooled"
                         % (str(names[np.argmax(count > 2)]), int(count[np.argmax(count > 2)])))
    order = np.argsort(inv, kind="stable")                         # source cells by pooled cell, each in source order
    first = np.zeros(names.size + 1, dtype=np.int64)
    np.cumsum(count, out=first[1:])
    src0 = order[first[:-1]] if names.size else np.zeros(0, dtype=np.int64)
    src1 = np.full(names.size, -1, dtype=np.int64)
    two = np.flatnonzero(count == 2)
    src1[two] = order[first[two] + 1]
    return PoolPlan(names, src0, src1, sizes)


# ---- the counts -------------------------------------------------------------------------------------

def _is_merged(s):
    return len(s) == 5 and isinstance(s[0], tuple)


class DevicePool(_lib.Handle):
    """The merged (ad, dp) columns of every sample on one GPU (C handle ``vrx_pool``): ``run`` pools them by a
    plan; several plans can run on one upload.  samples: a list of (AD, DP), each variants x cells in any format
    ``device_counts`` takes (or the tuple ``merge_counts`` returns), all with the same number of variants."""

    def __init__(self, samples, device=None, sizes=None):
        from .counts import default_device, merge_counts
        merged = [s if _is_merged(s) else merge_counts(*s) for s in samples]
        if not merged:
            raise ValueError("pool_counts: no sample")
        self.n_var = int(merged[0][0][0])
        for i, m in enumerate(merged):
            if int(m[0][0]) != self.n_var:
                raise ValueError("pool_counts: sample %d has %d variants, sample 1 has %d"
                                 % (i + 1, m[0][0], self.n_var))
        self.sizes = [int(m[0][1]) for m in merged]
        self.n_src = sum(self.sizes)
        if sizes is not None:
            self._check_sizes(sizes)
        colptr = np.zeros(self.n_src + 1, dtype=np.int64)
        at, base = 0, 0
        for m in merged:
            n = int(m[0][1])
            colptr[at + 1:at + n + 1] = np.asarray(m[1][1:], dtype=np.int64) + base
            at += n
            base += int(m[1][-1])
        rowidx, ad, dp = (np.ascontiguousarray(np.concatenate([np.asarray(m[k], dtype=np.int32) for m in merged]))
                          for k in (2, 3, 4))
        del merged
        _lib.require_gpu()
        self.device = default_device() if device is None else device
        L = _lib.lib()
        super().__init__("DevicePool", lambda out: L.vrx_pool_create(
            self.device, self.n_var, self.n_src, colptr.ctypes.data_as(_I64P), rowidx.ctypes.data_as(_I32P),
            ad.ctypes.data_as(_I32P), dp.ctypes.data_as(_I32P), out), L.vrx_pool_destroy)

    def _check_sizes(self, sizes):
        if [int(n) for n in sizes] != self.sizes:
            raise ValueError("pool_counts: the plan has %s cells per sample, the samples have %s columns"
                             % (list(sizes), self.sizes))

    def run(self, plan, merged=False, timing=None, download=True):
        """-> (AD, DP) int64 SciPy CSC of shape (variants, pooled cells), AD's zeros dropped, or with merged
        the tuple ``DeviceCounts.from_merged`` takes.  A summed count of 2^31 or more is a ValueError naming the
        pooled barcode.  timing (a dict) receives kernel_ms; download=False stops after the kernels."""
        self._check_sizes(plan.sizes)
        n_pool = plan.n_pool
        colptr = np.zeros(n_pool + 1, dtype=np.int64)
        bad, ms = C.c_int64(-1), C.c_double(0.0)
        L = _lib.lib()
        _lib.check(L.vrx_pool_run(self._h, n_pool, plan.src0.ctypes.data_as(_I32P), plan.src1.ctypes.data_as(_I32P),
                                  colptr.ctypes.data_as(_I64P), C.byref(bad), C.byref(ms)))
        if timing is not None:
            timing["kernel_ms"] = ms.value
        if bad.value >= 0:
            raise ValueError("pool_counts: pooled barcode %r: a summed count does not fit 31 bits"
                             % (str(plan.barcodes[bad.value]),))
        if not download:
            return None
        total = int(colptr[-1])
        rowidx, ad, dp = (np.empty(total, dtype=np.int32) for _ in range(3))
        _lib.check(L.vrx_pool_read(self._h, rowidx.ctypes.data_as(_I32P), ad.ctypes.data_as(_I32P),
                                   dp.ctypes.data_as(_I32P)))
        shape = (self.n_var, n_pool)
        if merged:
            return shape, colptr, rowidx, ad, dp
        DP = csc_matrix((dp.astype(np.int64), rowidx, colptr), shape=shape)
        AD = csc_matrix((ad.astype(np.int64), rowidx.copy(), colptr.copy()), shape=shape)
        for X in (AD, DP):
            X.has_sorted_indices = True
            X.has_canonical_format = True
        AD.eliminate_zeros()
        if total and dp.min() == 0:
            DP.eliminate_zeros()
        return AD, DP


def pool_counts(samples, plan, device=None, merged=False, timing=None):
    """The counts of a pool: every pooled column is the sum of its source columns (``PoolPlan``), computed on
    the GPU.  samples: a list of (AD, DP), one per sample and in the plan's sample order, each variants x cells
    in any format ``device_counts`` takes; all must have the same number of variants, and each as many columns
    as its barcode list.  -> (AD, DP) as int64 SciPy CSC with AD's zeros dropped (like ``synth.as_scipy``), or
    with merged=True the tuple ``DeviceCounts.from_merged(*...)`` takes."""
    pool = DevicePool(samples, device=device, sizes=plan.sizes)
    try:
        return pool.run(plan, merged=merged, timing=timing)
    finally:
        pool.close()


def _take_columns(X, cols):
    from scipy.sparse import issparse
    if issparse(X):
        return X.tocsc()[:, cols]
    return np.asarray(X)[:, cols]


def synth_pool(samples, barcodes, n_cell=None, minor_sample=1.0, doublet_rate=None, seed=None, out_dir=None,
               device=None):
    """A synthetic pool of several samples: ``sample_barcodes`` when n_cell is given, then ``pool_barcodes``
    (the calls of synth_pool.py:275-279, both reseeded with seed), ``pool_plan`` and ``pool_counts``.
    samples: (AD, DP) per sample, barcodes: the barcodes of its columns.  -> dict(AD, DP, barcodes (pooled, the
    columns of AD and DP), cell_info (rows of (CB_pool, CB_origin, Sample_id)), truth (``PoolPlan.truth``),
    plan).  The caller's lists are left alone."""
    if len(samples) != len(barcodes):
        raise ValueError("synth_pool: %d samples, %d barcode lists" % (len(samples), len(barcodes)))
    full = [list(b) for b in barcodes]
    for i, (s, b) in enumerate(zip(samples, full)):
        if s[0].shape[1] != len(b):
            raise ValueError("synth_pool: sample %d has %d columns and %d barcodes" % (i + 1, s[0].shape[1], len(b)))
    barcodes_in = [list(b) for b in full]
    if n_cell is not None:
        barcodes_in = sample_barcodes(barcodes_in, n_cell, minor_sample, seed)
        picked = []
        for s, b, keep in zip(samples, full, barcodes_in):
            at = {}
            for i, x in enumerate(b):
                at.setdefault(x, i)                                 # (list.index of the reference: the first)
            cols = np.array([at[x] for x in keep], dtype=np.int64)
            picked.append((_take_columns(s[0], cols), _take_columns(s[1], cols)))
        samples = picked
    barcodes_out = pool_barcodes(barcodes_in, out_dir, doublet_rate, seed=seed)
    plan = pool_plan(barcodes_in, barcodes_out)
    AD, DP = pool_counts(samples, plan, device=device)
    cell_info = [(barcodes_out[ss][ii], barcodes_in[ss][ii], str(ss + 1))
                 for ss in range(len(barcodes_out)) for ii in range(len(barcodes_out[ss]))]
    return dict(AD=AD, DP=DP, barcodes=plan.barcodes, cell_info=cell_info, truth=plan.truth(), plan=plan)


# ---- the command ------------------------------------------------------------------------------------

def build_parser():
    parser = OptionParser()
    parser.add_option("--cellData", "-c", dest="cell_data", default=None,
                      help="cellSNP output folders of the samples, comma separated")
    parser.add_option("--barcodeFiles", "-b", dest="barcodes_files", default=None,
                      help="Input barcode files, comma separated [default: each folder's cellSNP.samples.tsv]")
    parser.add_option("--doubletRate", "-d", dest="doublet_rate", type="float", default=None,
                      help="Doublet rate [default: n/100000]")
    parser.add_option("--outDir", "-o", dest="out_dir", default=None, help="Directory for output files")
    group = OptionGroup(parser, "Cell barcodes sampling")
    group.add_option("--nCELL", type="int", dest="n_cell", default=None,
                     help="The number of cells in each sample [default: %default]")
    group.add_option("--minorSAMPLE", type="float", dest="minor_sample", default=1.0,
                     help="Ratio size of minor sample [default: %default]")
    group.add_option("--randomSEED", type="int", dest="random_seed", default=None,
                     help="The random seed in numpy [default: %default]")
    parser.add_option_group(group)
    return parser


def write_mtx(path, X):
    """X (canonical CSC, counts below 2^31, no stored zeros) as MatrixMarket coordinate integer, variant-major
    like cellSNP writes it"""
    coo = X.tocsr().tocoo()
    r, c, v = (np.ascontiguousarray(a, dtype=np.int32) for a in (coo.row, coo.col, coo.data))
    _lib.check(_lib.lib().vrx_mtx_write(path.encode(), X.shape[0], X.shape[1], r.size, r.ctypes.data_as(_I32P),
                                        c.ctypes.data_as(_I32P), v.ctypes.data_as(_I32P)))


def main(argv=None):
    from .io_utils import read_cellSNP
    parser = build_parser()
    argv = sys.argv[1:] if argv is None else argv
    (opt, _args) = parser.parse_args(argv)
    if opt.cell_data is None or opt.out_dir is None:
        print("Error: need the samples' cellSNP folders (-c) and an output folder (-o); -h for the arguments.")
        sys.exit(1)
    dirs = opt.cell_data.split(",")
    files = opt.barcodes_files.split(",") if opt.barcodes_files is not None else \
        [os.path.join(d, "cellSNP.samples.tsv") for d in dirs]
    if len(files) != len(dirs):
        print("Error: barcodes files are not equal to cellSNP folders.")
        sys.exit(1)
    samples, barcodes, variants = [], [], None
    for d, f in zip(dirs, files):
        dat = read_cellSNP(d)
        fixed = dat["FixedINFO"]
        ident = [list(fixed[k]) for k in ("CHROM", "POS", "REF", "ALT")]
        if variants is None:
            variants = ident
        elif ident != variants:
            print("Error: %s does not list the same variants (CHROM, POS, REF, ALT) as %s." % (d, dirs[0]))
            sys.exit(1)
        with open(f, "r") as fid:
            lines = [x.rstrip() for x in fid.readlines()]
        if dat["AD"].shape[1] != len(lines) or dat["AD"].shape != dat["DP"].shape:
            print("Error: %s has %d cells, %s lists %d barcodes." % (d, dat["AD"].shape[1], f, len(lines)))
            sys.exit(1)
        samples.append((dat["AD"], dat["DP"]))
        barcodes.append(lines)
    os.makedirs(opt.out_dir, exist_ok=True)
    try:
        res = synth_pool(samples, barcodes, n_cell=opt.n_cell, minor_sample=opt.minor_sample,
                         doublet_rate=opt.doublet_rate, seed=opt.random_seed, out_dir=opt.out_dir)
    except ValueError as e:
        print("Error: %s" % e)
        sys.exit(1)
    shutil.copyfile(os.path.join(opt.out_dir, "barcodes_pool.tsv"), os.path.join(opt.out_dir, "cellSNP.samples.tsv"))
    write_mtx(os.path.join(opt.out_dir, "cellSNP.tag.AD.mtx"), res["AD"])
    write_mtx(os.path.join(opt.out_dir, "cellSNP.tag.DP.mtx"), res["DP"])
    shutil.copyfile(os.path.join(dirs[0], "cellSNP.base.vcf.gz"), os.path.join(opt.out_dir, "cellSNP.base.vcf.gz"))
    truth = res["truth"]
    print("[synth_pool] %d samples, %d source cells -> %d pooled cells (%d doublets), %d variants, %d AD and %d DP "
          "entries" % (len(dirs), res["plan"].n_src, truth.size, int(np.sum(truth == "doublet")),
                       res["AD"].shape[0], res["AD"].nnz, res["DP"].nnz))


if __name__ == "__main__":
    main()
