"""SNP-to-gene matching and gene-level counts: the front end of gene-level allele-specific expression.

``snp_gene_match`` is the reference's function of that name (vireoSNP/utils/vcf_utils.py:423-491) with its
semantics taken from its lines: for a SNP at ``pos`` and every gene of the same chromosome label (exact
equality, no ``chr`` normalisation)

    d1 = start - pos,  d2 = stop - pos,  dist = sign(d1) sign(d2) min(|d1|, |d2|)

(negative strictly inside the gene, 0 on a boundary, positive outside), the gaps are walked in the given order
and the first ``k`` with ``{g : dist_g < gaps[k]}`` non-empty answers with ``flag = k``: the single gene of
smallest ``dist`` (first in ``gene_df`` row order on ties) if ``gaps[k] > 0`` or ``multi_gene is False``,
every gene of the set in row order otherwise; no gap: ``flag = len(gaps)`` and no gene.  The reference loops
over the SNPs in Python; here all SNPs are matched in two launches (vrx_genematch.h).

``gene_counts`` is the step that follows: ``G @ AD`` and ``G @ DP`` with ``G[g, v]`` = the number of times
gene ``g`` is listed for SNP ``v``, expanded, sorted and added on the device.

The host side is NumPy: labels to codes, genes grouped by code (stable: ``gene_df`` order survives inside a
chromosome), SNPs sorted by code with the permutation handed to the kernel, which writes results in the
caller's order.  Every argument check happens before the GPU is touched.  pandas is not imported: ``gene_df``
is anything that gives columns by name.
"""
import ctypes as C
import operator

import numpy as np
from scipy.sparse import csc_matrix

from . import _lib

COORD_MAX = 2 ** 31 - 1
_I32P = C.POINTER(C.c_int32)
_I64P = C.POINTER(C.c_int64)


def _coords(values, name):
    """int32 array of coordinates in [0, 2^31 - 1]; ValueError on anything else (strings of integers pass)"""
    a = np.asarray(values)
    if a.ndim != 1:
        a = a.reshape(-1)
    try:
        if a.dtype.kind in "iub":
            v = a.astype(np.int64) if a.dtype != np.uint64 else a
        elif a.dtype.kind == "f":
            if not np.all(np.isfinite(a)) or np.any(a != np.floor(a)):
                raise ValueError
            if a.size and (a.min() < 0 or a.max() > COORD_MAX):
                raise ValueError
            v = a.astype(np.int64)
        elif a.dtype.kind in "US":
            v = a.astype(np.int64)
        else:
            items = a.tolist()
            if any(isinstance(x, float) and (x != x or x != int(x)) for x in items if not isinstance(x, str)):
                raise ValueError
            v = np.array([int(x) for x in items], dtype=object)
            if len(items) and (min(v) < 0 or max(v) > COORD_MAX):
                raise ValueError
            v = v.astype(np.int64)
    except (ValueError, TypeError, OverflowError):
        raise ValueError("%s must hold integers in [0, 2^31 - 1]" % name) from None
    if v.size and (v.min() < 0 or v.max() > COORD_MAX):
        bad = int(np.flatnonzero((v < 0) | (v > COORD_MAX))[0])
        raise ValueError("%s[%d] = %s: coordinates must lie in [0, 2^31 - 1]" % (name, bad, v[bad]))
    return np.ascontiguousarray(v, dtype=np.int32)


def _labels(values):
    a = np.asarray(values)
    if a.dtype.kind == "O" and all(isinstance(x, str) for x in a.tolist()):
        a = a.astype(str)
    return a.reshape(-1)


def _factorise(snp_chrom, gene_chrom):
    """-> (n_code, code of every SNP, code of every gene or -1): codes number the SNPs' labels; a gene whose
    label no SNP carries can match nothing and gets -1.  Equality is ``==`` of the labels as given."""
    a, b = _labels(snp_chrom), _labels(gene_chrom)
    ka, kb = a.dtype.kind, b.dtype.kind
    if (ka in "US" and kb in "US") or (ka in "iu" and kb in "iu"):
        if ka in "US":
            a, b = a.astype(str), b.astype(str)
        uniq, code = np.unique(a, return_inverse=True)
        if uniq.size == 0:
            return 0, code.astype(np.int32), np.full(b.size, -1, dtype=np.int32)
        at = np.minimum(np.searchsorted(uniq, b), uniq.size - 1)
        return int(uniq.size), code.astype(np.int32), np.where(uniq[at] == b, at, -1).astype(np.int32)
    table = {}
    code = np.fromiter((table.setdefault(x, len(table)) for x in a.tolist()), dtype=np.int32, count=a.size)
    gcode = np.fromiter((table.get(x, -1) if x == x else -1 for x in b.tolist()), dtype=np.int32, count=b.size)
    return len(table), code, gcode


def _gaps(gaps, multi_gene):
    try:
        g = [operator.index(x) for x in gaps]
    except TypeError:
        raise ValueError("gaps must be a sequence of ints") from None
    if len(g) == 0:
        raise ValueError("gaps is empty: at least one gap is needed")
    # dist lies in [-(2^31 - 1), 2^31 - 1]: "dist < gap" is "dist <= gap - 1", and clamping gap - 1 to the
    # int32 range changes no comparison
    gap_m1 = np.array([min(max(x - 1, -2 ** 31), 2 ** 31 - 1) for x in g], dtype=np.int32)
    single = np.array([1 if (x > 0 or multi_gene is False) else 0 for x in g], dtype=np.uint8)
    return gap_m1, single


def prepare(chrom, pos, gene_chrom, start, stop, multi_gene=True, gaps=(0, 1000, 10000, 100000)):
    """All host work of a match, no GPU: dict of the arrays vrx_genematch_create / _match take."""
    gap_m1, single = _gaps(gaps, multi_gene)
    pos = _coords(pos, "POS")
    start, stop = _coords(start, "start"), _coords(stop, "stop")
    n_snp, n_gene = pos.size, start.size
    if len(chrom) != n_snp:
        raise ValueError("CHROM has %d entries, POS %d" % (len(chrom), n_snp))
    if stop.size != n_gene or len(gene_chrom) != n_gene:
        raise ValueError("gene columns differ in length")
    n_code, code, gcode = _factorise(chrom, gene_chrom)
    keep = np.flatnonzero(gcode >= 0)
    order = keep[np.argsort(gcode[keep], kind="stable")]
    chrom_ptr = np.zeros(n_code + 1, dtype=np.int64)
    np.cumsum(np.bincount(gcode[keep], minlength=n_code), out=chrom_ptr[1:])
    perm = np.argsort(code, kind="stable").astype(np.int32)
    return dict(n_snp=n_snp, n_code=n_code, chrom_ptr=chrom_ptr,
                start=np.ascontiguousarray(start[order]), stop=np.ascontiguousarray(stop[order]),
                row=np.ascontiguousarray(order, dtype=np.int32),
                code=np.ascontiguousarray(code[perm]), pos=np.ascontiguousarray(pos[perm]), perm=perm,
                gap_m1=gap_m1, single=single)


def match_prepared(p, device=None, timing=None):
    """-> (flag int32[n_snp], ptr int64[n_snp + 1], rows int32[ptr[-1]]) of a ``prepare`` result: the device
    part.  ``timing`` (a dict) receives kernel_ms of the two calls."""
    from .counts import default_device
    _lib.require_gpu()
    L = _lib.lib()
    with _lib.Handle("the gene table", lambda out: L.vrx_genematch_create(
            default_device() if device is None else device, p["n_code"], p["start"].size,
            p["chrom_ptr"].ctypes.data_as(_I64P), p["start"].ctypes.data_as(_I32P), p["stop"].ctypes.data_as(_I32P),
            p["row"].ctypes.data_as(_I32P), out), L.vrx_genematch_destroy) as h:
        n = p["n_snp"]
        flag = np.zeros(n, dtype=np.int32)
        count = np.zeros(n, dtype=np.int64)
        ms1, ms2 = C.c_double(0.0), C.c_double(0.0)
        _lib.check(L.vrx_genematch_match(
            h.ptr, n, p["code"].ctypes.data_as(_I32P), p["pos"].ctypes.data_as(_I32P), p["perm"].ctypes.data_as(_I32P),
            p["gap_m1"].size, p["gap_m1"].ctypes.data_as(_I32P), p["single"].ctypes.data_as(C.POINTER(C.c_uint8)),
            flag.ctypes.data_as(_I32P), count.ctypes.data_as(_I64P), C.byref(ms1)))
        ptr = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(count, out=ptr[1:])
        rows = np.zeros(int(ptr[-1]), dtype=np.int32)
        _lib.check(L.vrx_genematch_lists(h.ptr, int(ptr[-1]), rows.ctypes.data_as(_I32P), C.byref(ms2)))
    if timing is not None:
        timing["kernel_ms"] = ms1.value + ms2.value
    return flag, ptr, rows


def snp_gene_match(varFixedINFO, gene_df, gene_key='gene', multi_gene=True,
                   gaps=[0, 1000, 10000, 100000], verbose=False):
    """The reference's ``snp_gene_match`` (vcf_utils.py:423-491) on the GPU -> (gene_list, flag_list).

    varFixedINFO: 'CHROM' and 'POS' as ``load_VCF`` returns them (POS may be strings).  gene_df: columns
    'chrom', 'start', 'stop' and ``gene_key`` by name -- a pandas DataFrame or a dict of arrays.
    gene_list[i]: the matched names of SNP i, an array of the column's dtype (empty without a match);
    flag_list[i]: the index of the gap that matched, ``len(gaps)`` for none.  Coordinates must be integers in
    [0, 2^31 - 1] and ``gaps`` non-empty: ValueError otherwise, before the GPU is touched."""
    chrom = varFixedINFO['CHROM']
    names = np.asarray(gene_df[gene_key])
    p = prepare(chrom, varFixedINFO['POS'], gene_df['chrom'], gene_df['start'], gene_df['stop'],
                multi_gene=multi_gene, gaps=gaps)
    if names.shape[0] != len(np.asarray(gene_df['start']).reshape(-1)):
        raise ValueError("gene_df[%r] and gene_df['start'] differ in length" % (gene_key,))
    flag, ptr, rows = match_prepared(p)
    if verbose:
        cur = 'None'
        for c in chrom:
            if cur != c:
                cur = c
                print('processing:', c)
    flat = names[rows]
    gene_list = [flat[ptr[i]:ptr[i + 1]] for i in range(p["n_snp"])]
    return gene_list, flag.tolist()


def gene_index(gene_list, flag_list=None, max_flag=None, gene_names=None):
    """-> (gene_names array, gptr int64[n_snp + 1], gid int32[gptr[-1]]): the map of ``gene_counts`` as a CSR
    over SNPs, host work only.  gene_names defaults to ``np.unique`` of every name in gene_list (filtered SNPs
    included, so the rows do not depend on max_flag); a listed name that is not in a given gene_names is a
    ValueError.  With flag_list and max_flag only SNPs with flag <= max_flag keep their genes."""
    n = len(gene_list)
    lens = np.fromiter((len(g) for g in gene_list), dtype=np.int64, count=n)
    parts = [np.asarray(g) for g in gene_list if len(g)]
    flat = np.concatenate(parts) if parts else np.zeros(0, dtype=str)
    if gene_names is None:
        names = np.unique(flat)
        gid = np.searchsorted(names, flat)
    else:
        names = np.asarray(gene_names).reshape(-1)
        order = np.argsort(names, kind="stable")
        srt = names[order]
        if srt.size > 1 and np.any(srt[1:] == srt[:-1]):
            raise ValueError("gene_names holds a name twice: %r" % (str(srt[1:][srt[1:] == srt[:-1]][0]),))
        if flat.size and srt.size == 0:
            raise ValueError("gene %r is not in gene_names" % (str(flat[0]),))
        at = np.minimum(np.searchsorted(srt, flat), max(srt.size - 1, 0))
        miss = np.flatnonzero(srt[at] != flat) if flat.size else np.zeros(0, dtype=np.int64)
        if miss.size:
            raise ValueError("gene %r is not in gene_names" % (str(flat[miss[0]]),))
        gid = order[at] if flat.size else np.zeros(0, dtype=np.int64)
    if (flag_list is None) != (max_flag is None):
        raise ValueError("flag_list and max_flag go together")
    if max_flag is not None:
        flags = np.asarray(flag_list).reshape(-1)
        if flags.size != n:
            raise ValueError("flag_list has %d entries, gene_list %d" % (flags.size, n))
        keep = flags <= max_flag
        gid = gid[np.repeat(keep, lens)]
        lens = np.where(keep, lens, 0)
    gptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=gptr[1:])
    return names, gptr, np.ascontiguousarray(gid, dtype=np.int32)


def gene_counts(AD, DP, gene_list, flag_list=None, max_flag=None, gene_names=None, device=None, timing=None):
    """Gene-level counts -> (AD_gene, DP_gene, gene_names): ``G @ AD`` and ``G @ DP`` as SciPy CSC int64
    matrices (n_gene, n_cell), canonical and without stored zeros, where ``G[g, v]`` is the number of times
    gene ``gene_names[g]`` occurs in ``gene_list[v]`` (a SNP with several genes adds to each; a name listed twice
    counts twice).  AD, DP: variants x cells, whatever ``merge_counts`` accepts; gene_list (and flag_list) as
    ``snp_gene_match`` returns them; see ``gene_index`` for gene_names, flag_list and max_flag.  A sum of 2^31
    or more is an OverflowError naming the gene and the cell."""
    from .counts import default_device, merge_counts
    (n_var, n_cell), colptr, rowidx, ad, dp = merge_counts(AD, DP)
    if len(gene_list) != n_var:
        raise ValueError("gene_list has %d entries, AD %d variants" % (len(gene_list), n_var))
    names, gptr, gid = gene_index(gene_list, flag_list, max_flag, gene_names)
    n_gene = int(names.size)
    _lib.require_gpu()
    L = _lib.lib()
    n_out, ms = C.c_int64(0), C.c_double(0.0)
    colptr = np.ascontiguousarray(colptr, dtype=np.int64)
    with _lib.Handle("the gene counts", lambda out: L.vrx_genecount_create(
            default_device() if device is None else device, n_var, n_cell, n_gene, colptr.ctypes.data_as(_I64P),
            rowidx.ctypes.data_as(_I32P), ad.ctypes.data_as(_I32P), dp.ctypes.data_as(_I32P),
            gptr.ctypes.data_as(_I64P), gid.ctypes.data_as(_I32P), out, C.byref(n_out), C.byref(ms)),
            L.vrx_genecount_destroy) as h:
        key = np.zeros(n_out.value, dtype=np.int64)
        sa, sd = np.zeros(n_out.value, dtype=np.int64), np.zeros(n_out.value, dtype=np.int64)
        _lib.check(L.vrx_genecount_read(h.ptr, key.ctypes.data_as(_I64P), sa.ctypes.data_as(_I64P),
                                        sd.ctypes.data_as(_I64P)))
    if timing is not None:
        timing["kernel_ms"] = ms.value
    cell, gene = (key // n_gene, key % n_gene) if n_gene else (key, key)
    big = np.flatnonzero((sa >= 2 ** 31) | (sd >= 2 ** 31))
    if big.size:
        b = big[0]
        raise OverflowError("gene %r, cell %d: the gene-level count %d does not fit 31 bits"
                            % (str(names[gene[b]]), cell[b], max(sa[b], sd[b])))

    def csc(x):
        keep = x > 0
        indptr = np.zeros(n_cell + 1, dtype=np.int64)
        np.cumsum(np.bincount(cell[keep], minlength=n_cell), out=indptr[1:])
        m = csc_matrix((x[keep], gene[keep].astype(np.int32), indptr), shape=(n_gene, n_cell))
        m.has_sorted_indices = True
        m.has_canonical_format = True
        return m

    return csc(sa), csc(sd), names


def parse_genes(path, gene_key='gene'):
    """A tab-separated gene table with a header line naming ``chrom``, ``start``, ``stop`` and the gene key
    (a leading '#' of the header is dropped; other columns are ignored) -> dict of arrays by those names."""
    with open(path, "r") as f:
        lines = [ln.rstrip("\r\n") for ln in f]
    lines = [ln for ln in lines if ln.strip() != ""]
    if not lines:
        raise ValueError("%s: no header line" % path)
    head = lines[0].lstrip("#").split("\t")
    want = ["chrom", "start", "stop", gene_key]
    for k in want:
        if k not in head:
            raise ValueError("%s: the header has no column %r" % (path, k))
    at = [head.index(k) for k in want]
    cols = [[], [], [], []]
    for no, ln in enumerate(lines[1:], 2):
        f = ln.split("\t")
        if len(f) <= max(at):
            raise ValueError("%s, line %d: %d fields, the header names %d" % (path, no, len(f), len(head)))
        for c, j in zip(cols, at):
            c.append(f[j])
    try:
        start, stop = np.array(cols[1], dtype=np.int64), np.array(cols[2], dtype=np.int64)
    except (ValueError, OverflowError):
        raise ValueError("%s: start and stop must be integers" % path) from None
    return {"chrom": np.array(cols[0], dtype=str), "start": start.reshape(-1), "stop": stop.reshape(-1),
            gene_key: np.array(cols[3], dtype=str)}
