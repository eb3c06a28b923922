"""Cell-data loaders and result writers of the ``vireo`` command (host side).

Own implementation of vireoSNP/utils/io_utils.py: read_cellSNP (:42-59), read_vartrix
(:62-88), match_donor_VCF (:10-39) and write_donor_id (:91-170: donor_ids.tsv,
summary.tsv, prob_singlet/doublet.tsv.gz, _log.txt); read_cellVCF is the cell VCF of
``vireo -c cells.vcf.gz`` (vireo.py:112-117) read on the GPU (csrc/vrx_cellvcf.h).  Output text is formatted exactly like
the reference's so that downstream tools (and users' grep) keep working.
"""
import gzip
import os
import shutil
import time
from itertools import combinations

import ctypes as C

import numpy as np
from scipy.sparse import coo_matrix, csc_matrix, csr_matrix

from . import _lib
from .bgzf import BgzfStatus
from .vcf_utils import (_DonorText, _SLAB_BYTES, _SLAB_LIMIT, _VCF_STATUS, _labels_blob, _sparse_geno, load_VCF,
                        match_SNPs, read_sparse_GeneINFO)


def _read_mtx_arrays(path, n_threads=0):
    """-> ((n_rows, n_cols), row, col, val) int32 COO arrays in file order from the library's
    multi-threaded parser (vrx_mtx_read), or None for what it does not read (gzipped files,
    symmetric / complex / array storage)"""
    path = str(path)
    L = _lib.lib()
    n_rows, n_cols, nnz = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    if path.endswith(".gz") or L.vrx_mtx_header(path.encode(), C.byref(n_rows), C.byref(n_cols),
                                                C.byref(nnz)) != 0:
        return None
    row = np.empty(nnz.value, dtype=np.int32)
    col = np.empty(nnz.value, dtype=np.int32)
    val = np.empty(nnz.value, dtype=np.int32)
    i32 = C.POINTER(C.c_int32)
    _lib.check(L.vrx_mtx_read(path.encode(), nnz.value, row.ctypes.data_as(i32),
                              col.ctypes.data_as(i32), val.ctypes.data_as(i32), int(n_threads)))
    return (n_rows.value, n_cols.value), row, col, val


def read_mtx(path, n_threads=0):
    """MatrixMarket coordinate file -> scipy COO matrix (int64 counts), parsed by the library's
    multi-threaded reader (vrx_mtx_read) instead of scipy.io.mmread (io_utils.py:57): the same
    entries in file order, duplicates kept (``.tocsc()`` sums them, like after mmread).
    Gzipped files and symmetric / complex / array storage fall back to scipy."""
    got = _read_mtx_arrays(path, n_threads)
    if got is None:
        from scipy.io import mmread
        return mmread(str(path))
    shape, row, col, val = got
    return coo_matrix((val.astype(np.int64), (row, col)), shape=shape)


def read_mtx_csc(path, n_threads=0):
    """``mmread(path).tocsc()`` (io_utils.py:57) without SciPy's single-threaded COO -> CSC
    conversion: the library parses the file (vrx_mtx_read) and sorts the entries into columns on
    all cores (vrx_coo_to_csc).  A file whose columns do not come out strictly increasing
    (duplicate entries, or not variant-major) goes through SciPy's conversion, which sorts and sums
    duplicates like the reference's."""
    got = _read_mtx_arrays(path, n_threads)
    if got is None:
        from scipy.io import mmread
        return mmread(str(path)).tocsc()
    shape, row, col, val = got
    nnz = row.size
    indptr = np.empty(shape[1] + 1, dtype=np.int64)
    indices = np.empty(nnz, dtype=np.int32)
    data = np.empty(nnz, dtype=np.int64)
    canonical = C.c_int32(0)
    i32, i64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    _lib.check(_lib.lib().vrx_coo_to_csc(shape[0], shape[1], nnz, row.ctypes.data_as(i32),
                                         col.ctypes.data_as(i32), val.ctypes.data_as(i32),
                                         indptr.ctypes.data_as(i64), indices.ctypes.data_as(i32),
                                         data.ctypes.data_as(i64), C.byref(canonical), int(n_threads)))
    if not canonical.value:
        return coo_matrix((val.astype(np.int64), (row, col)), shape=shape).tocsc()
    out = csc_matrix((data, indices, indptr), shape=shape)
    out.has_canonical_format = True                           # (checked column by column in the library)
    return out


def read_cellSNP(dir_name, layers=['AD', 'DP']):
    """cellSNP output folder -> dict with AD, DP (CSC), samples, variants, ...
    (io_utils.py:42-59)."""
    dat = load_VCF(dir_name + "/cellSNP.base.vcf.gz", load_sample=False, biallelic_only=False)
    for layer in layers:
        dat[layer] = read_mtx_csc(dir_name + "/cellSNP.tag.%s.mtx" % layer)
    dat['samples'] = np.genfromtxt(dir_name + "/cellSNP.samples.tsv", dtype=str)
    return dat


def read_vartrix(alt_mtx, ref_mtx, cell_file, vcf_file=None):
    """VarTrix alt/ref matrices -> AD, DP = ref + alt (io_utils.py:62-88)."""
    if vcf_file is not None:
        dat = load_VCF(vcf_file, load_sample=False, biallelic_only=False)
        dat['variants'] = np.array(dat['variants'])
    else:
        dat = {}
    dat['AD'] = read_mtx_csc(alt_mtx)
    dat['DP'] = read_mtx_csc(ref_mtx) + dat['AD']
    dat['samples'] = np.genfromtxt(cell_file, dtype=str)
    return dat


_CELL_STATUS = _VCF_STATUS + ((64, "a kept line whose FORMAT differs from the first kept line's"),
                              (128, "a kept line whose sample-field count is not the #CHROM line's"),
                              (256, "an entry with fewer subfields than FORMAT has names"))
_STR_SPACE = " \t\n\r\x0b\x0c\x1c\x1d\x1e\x1f"                     # what str.rstrip() removes, ASCII
_CELL_FORMAT_MAX = 255


def _cell_reason(status):
    return "; ".join(text for bit, text in _CELL_STATUS if status & bit)


def _cell_host(vcf_file, biallelic_only, keys, axes, reason):
    """read_cellVCF as the composition it replaces: load_VCF, read_sparse_GeneINFO"""
    t0 = time.perf_counter()
    vcf = load_VCF(vcf_file, biallelic_only=biallelic_only)
    dat = read_sparse_GeneINFO(vcf['GenoINFO'], keys=keys, axes=axes)
    for k in ('samples', 'variants', 'FixedINFO', 'contigs', 'comments', 'n_SNP_tagged'):
        dat[k] = vcf[k]
    sec = dict(inflate=0.0, upload=0.0, kernels=0.0, download=0.0, host=time.perf_counter() - t0)
    dat.update(path='host', reason=reason, n_lines=len(vcf['variants']), n_repaired=0, seconds=sec)
    return dat


def _first_kept_format(slab, biallelic_only):
    """-> (FORMAT bytes of the slab's first kept line or None when it keeps none, why the host path is due or None):
    the one line of a cell VCF that is split here before the device sees the file"""
    pos, n = 0, len(slab)
    while pos < n:
        end = slab.find(b"\n", pos)
        end = n if end < 0 else end
        f = bytes(slab[pos:end]).decode("latin-1").rstrip(_STR_SPACE).split("\t", 9)
        pos = end + 1
        if f[0].startswith("#"):
            return None, _cell_reason(8)
        if len(f) < 9:
            return None, _cell_reason(16)
        if biallelic_only and (len(f[3]) > 1 or len(f[4]) > 1):
            continue
        return f[8].encode("latin-1"), None
    return None, None


def _cell_repair(lines, format_list):
    """the sparse layout (vcf_utils._sparse_geno) of every flagged line, one line at a time: raises the IndexError
    that load_VCF raises on a short entry"""
    out = []
    for raw in lines:
        f = raw.decode("ascii").rstrip().split("\t")
        out.append(_sparse_geno([f[9:]], [f[8].split(":")], format_list)[0])
    return out


def read_cellVCF(vcf_file, biallelic_only=True, keys=('AD', 'DP'), axes=(-1, -1), device=None, slab_bytes=None,
                 force_host=False):
    """cellSNP's cells.vcf.gz -> the dict the ``vireo`` command takes from ``load_VCF(vcf_file, biallelic_only)``
    (vcf_utils.py:80-159, parse_sample_info :12-57) and ``read_sparse_GeneINFO`` (:192-205): one float64 CSR matrix
    (variants x cells) per name in ``keys``, samples, variants, FixedINFO, contigs, comments and n_SNP_tagged, with the
    same index dtypes, explicit zeros and entry order, from one pass over the text on the GPU (``vrx_cellvcf_*``,
    csrc/vrx_cellvcf.h).  The file is inflated on the device when it is BGZF (``vireo_amd.bgzf``; by Python's gzip
    otherwise, or with VIREO_INFLATE=host) and fed in slabs of whole lines (``slab_bytes``, default 256 MiB); the
    device finds the lines, the filter, the entries among the sample fields, their cells and the two values; lines
    with a value outside its grammar ('.' or 1-9 digits after the last comma) come back flagged and their values are parsed here by the host functions; variants and FixedINFO are sliced from the text at the
    offsets the device returns.  Also returned: path 'device' | 'host', reason, n_lines (kept lines), n_repaired,
    seconds dict(inflate, upload, kernels, download, host).  The host path, the composition above, is taken with
    ``force_host`` or VIREO_CELL_VCF=host, for keys / axes other than two keys with axis -1, and for files whose
    lines the device cannot vouch for (``reason`` says which).  Without ``force_host`` there is no fallback for a
    missing GPU."""
    keys, axes = list(keys), list(axes)

    def host(reason):
        return _cell_host(vcf_file, biallelic_only, keys, axes, reason)

    if force_host or os.environ.get("VIREO_CELL_VCF") == "host":
        return host("forced")
    if len(keys) != 2 or axes != [-1, -1]:
        return host("the device reads two keys with axis -1")
    _lib.require_gpu()
    from .counts import default_device
    L = _lib.lib()
    device = default_device() if device is None else int(device)
    slab_bytes = _SLAB_BYTES if slab_bytes is None else int(slab_bytes)
    if not 1 <= slab_bytes <= _SLAB_LIMIT:
        raise ValueError("slab_bytes must lie in 1 ... %d" % _SLAB_LIMIT)
    t_all = time.perf_counter()
    sec = dict(inflate=0.0, upload=0.0, kernels=0.0, download=0.0, host=0.0)
    text = None
    try:
        text = _DonorText(vcf_file, sec, device)
        head = text.header()
        for raw in head:                                          # the '#' lines as load_VCF's text layer sees them
            core = raw[:-2] if raw.endswith(b"\r\n") else raw.rstrip(b"\n")
            if b"\r" in core or (raw and max(raw) >= 0x80):
                return host(_cell_reason(32))
        fixed, fkeys, contigs, comments, samples = {}, [], [], [], []
        for raw in head:
            line = raw.decode("ascii").rstrip()
            if line.startswith("##contig="):
                contigs.append(line)
            if line.startswith("#CHROM"):
                cols = line[1:].split("\t")
                fkeys = cols[:8]
                fixed = {k: [] for k in fkeys}
                samples = cols[9:]
            else:
                comments.append(line)
        S = len(samples)
        if S == 0:
            return host("no sample columns")
        with _lib.Handle("the cell VCF reader",
                         lambda out: L.vrx_cellvcf_create(device, S, int(bool(biallelic_only)), out),
                         L.vrx_cellvcf_destroy) as reader:
            info = np.zeros(4, dtype=np.int64)
            t2 = np.zeros(2)
            fmt = format_list = None
            variants, repair = [], []
            p_indptr, p_cell, p_v0, p_v1 = [], [], [], []
            n_entries = 0
            for slab in text.slabs(slab_bytes):
                if len(slab) > _SLAB_LIMIT:
                    return host("a line of 2 GiB")
                if fmt is None:
                    fmt, why = _first_kept_format(slab, biallelic_only)
                    if why is not None:
                        return host(why)
                    if fmt is not None:
                        format_list = fmt.decode("latin-1").split(":")
                        if not 1 <= len(fmt) <= _CELL_FORMAT_MAX:
                            return host("a FORMAT of %d bytes" % len(fmt))
                        if keys[0] not in format_list or keys[1] not in format_list:
                            return host("FORMAT does not name the keys")
                        _lib.check(L.vrx_cellvcf_format(reader.ptr, fmt, len(fmt), format_list.index(keys[0]),
                                                        format_list.index(keys[1])))
                raw = (C.c_char * len(slab)).from_buffer(slab)
                _lib.check(L.vrx_cellvcf_slab(reader.ptr, raw, len(slab), info.ctypes.data_as(_lib._I64),
                                              _lib.dptr(t2)))
                del raw
                sec['upload'] += t2[0]
                sec['kernels'] += t2[1]
                if info[3]:
                    return host(_cell_reason(int(info[3])))
                R, E = int(info[0]), int(info[1])
                if R == 0:
                    continue
                indptr, flag = np.empty(R + 1, np.int64), np.empty(R, np.int32)
                span, off = np.empty((R, 2), np.int64), np.empty((R, 10), np.int32)
                cell, v0, v1 = np.empty(E, np.int32), np.empty(E, np.int32), np.empty(E, np.int32)
                _lib.check(L.vrx_cellvcf_rows(reader.ptr, indptr.ctypes.data_as(_lib._I64),
                                              cell.ctypes.data_as(_lib._I32),
                                              v0.ctypes.data_as(_lib._I32), v1.ctypes.data_as(_lib._I32),
                                              flag.ctypes.data_as(_lib._I32), span.ctypes.data_as(_lib._I64),
                                              off.ctypes.data_as(_lib._I32), _lib.dptr(t2)))
                sec['download'] += t2[0]
                assert indptr[0] == 0 and indptr[R] == E
                for r in np.flatnonzero(flag):                        # the text of a flagged line outlives its slab
                    repair.append((len(variants) + int(r), bytes(slab[span[r, 0]:span[r, 1]])))
                start, tab7 = span[:, 0].tolist(), off[:, 7].tolist()
                for r in range(R):                                # CHROM ... INFO: the text in front of the eighth tab
                    f = slab[start[r]:tab7[r]].decode("ascii").split("\t")
                    for k, v in zip(fkeys, f):
                        fixed[k].append(v)
                    variants.append("_".join((f[0], f[1], f[3], f[4])))
                p_indptr.append(indptr[:-1] + n_entries)
                p_cell.append(cell)
                p_v0.append(v0)
                p_v1.append(v1)
                n_entries += E
    except BgzfStatus as e:                                           # the whole file on the host: gzip raises its own
        return host("BGZF " + e.reason)
    finally:
        if text is not None:
            text.close()

    n_var = len(variants)
    if n_var == 0:
        return host("no kept lines")
    indptr = np.concatenate(p_indptr + [np.array([n_entries], dtype=np.int64)])
    indices = np.concatenate(p_cell).astype(np.int64)
    data = [np.concatenate(p).astype(np.float64) for p in (p_v0, p_v1)]
    # the host functions on the flagged lines, in the order in which the composition meets them: the sparse layout of
    # every line (where load_VCF would raise), the tag warning, then the values one key at a time (where
    # read_sparse_GeneINFO would)
    try:
        layouts = _cell_repair([raw for _, raw in repair], format_list)
    except IndexError:
        return host("a flagged line with a short entry")
    for (r, _), geno in zip(repair, layouts):
        if geno['indices'] != indices[indptr[r]:indptr[r + 1]].tolist():
            return host("a flagged line the host reads differently")
    if n_entries < 0.1 * n_var:
        print('[vireo] Warning: too few variants with tags!',
              '\t'.join(k + ": " + str(n_entries) for k in format_list))
    for key, values in zip(keys, data):
        for (r, _), geno in zip(repair, layouts):
            values[indptr[r]:indptr[r + 1]] = read_sparse_GeneINFO(geno, keys=[key], axes=[-1])[key].data
    dat = {key: csr_matrix((values, indices, indptr), shape=(n_var, S)) for key, values in zip(keys, data)}
    sec['host'] = time.perf_counter() - t_all - sec['inflate'] - sec['upload'] - sec['kernels'] - sec['download']
    dat.update(samples=samples, variants=variants, FixedINFO=fixed, contigs=contigs, comments=comments,
               n_SNP_tagged=np.full(len(format_list), n_entries, dtype=np.int64), path='device', reason=None,
               n_lines=n_var, n_repaired=len(repair), seconds=sec)
    return dat


def match_donor_VCF(cell_dat, donor_vcf):
    """keep the variants present in both the cell data and the donor VCF, in cell order
    (io_utils.py:10-39)."""
    mm = match_SNPs(cell_dat['variants'], donor_vcf['variants'])
    keep = np.where(mm != None)[0]                                   # noqa: E711
    if len(keep) == 0:
        print("[vireo] warning: no variants matched to donor VCF, please check chr format!")
    else:
        print("[vireo] %d out %d variants matched to donor VCF"
              % (len(keep), len(cell_dat['variants'])))
    other = mm[keep].astype(int)
    cell_dat['AD'] = cell_dat['AD'][keep, :]
    cell_dat['DP'] = cell_dat['DP'][keep, :]
    cell_dat["variants"] = [cell_dat["variants"][x] for x in keep]
    for k in cell_dat["FixedINFO"]:
        cell_dat["FixedINFO"][k] = [cell_dat["FixedINFO"][k][x] for x in keep]
    donor_vcf["variants"] = [donor_vcf["variants"][x] for x in other]
    for k in donor_vcf["FixedINFO"]:
        donor_vcf["FixedINFO"][k] = [donor_vcf["FixedINFO"][k][x] for x in other]
    for k in donor_vcf["GenoINFO"]:
        donor_vcf["GenoINFO"][k] = [donor_vcf["GenoINFO"][k][x] for x in other]
    return cell_dat, donor_vcf


def _gzip_file(path):
    with open(path, "rb") as src, gzip.open(path + ".gz", "wb") as dst:
        shutil.copyfileobj(src, dst)
    os.remove(path)


def _write_table_gz(path, header, row_names, table):
    """<header>, then <row name> TAB "%.2e" ... per row, gzipped (the reference writes the text
    with a Python loop and runs ``gzip -f``, io_utils.py:147-170); formatted and deflated on
    several threads by libvireo_hip.so"""
    table = np.ascontiguousarray(table, dtype=np.float64)
    blob, off = _labels_blob(row_names)
    _lib.check(_lib.lib().vrx_write_table(
        path.encode(), ("\t".join(header) + "\n").encode(), blob,
        off.ctypes.data_as(C.c_void_p), _lib.dptr(table), table.shape[0], table.shape[1],
        b"%.2e", 1))


def write_donor_id(out_dir, donor_names, cell_names, n_vars, res_vireo):
    """donor_ids.tsv, summary.tsv, prob_singlet.tsv.gz, prob_doublet.tsv.gz, _log.txt (and
    prop_ambient.tsv when the result carries ambient_Psi) with the
    reference's thresholds (prob_max < 0.9 -> unassigned, doublet >= 0.9, n_vars < 10 ->
    unassigned) and number formats (io_utils.py:91-170)."""
    ID_prob, doublet_prob = res_vireo['ID_prob'], res_vireo['doublet_prob']
    prob_max = np.max(ID_prob, axis=1)
    prob_dbl = np.max(doublet_prob, axis=1)
    best_singlet = np.array(donor_names, "U100")[np.argmax(ID_prob, axis=1)]
    pair_names = [",".join(x) for x in combinations(donor_names, 2)]
    best_doublet = np.array(pair_names, "U100")[np.argmax(doublet_prob, axis=1)]
    donor_ids = best_singlet.copy()
    donor_ids[prob_max < 0.9] = "unassigned"
    donor_ids[prob_dbl >= 0.9] = "doublet"
    donor_ids[n_vars < 10] = "unassigned"

    with open(out_dir + "/_log.txt", "w") as f:
        f.write("logLik: %.3e\n" % (res_vireo['LB_doublet']))
        f.write("thetas: \n%s\n" % (res_vireo['theta_shapes']))

    uniq, count = np.unique(donor_ids, return_counts=True)
    with open(out_dir + "/summary.tsv", "w") as f:
        f.write("Var1\tFreq\n")
        for u, c in zip(uniq, count):
            f.write("%s\t%d\n" % (u, c))
    print("[vireo] final donor size:")
    print("\t".join(str(x) for x in uniq))
    print("\t".join(str(x) for x in count))

    with open(out_dir + "/donor_ids.tsv", "w") as f:
        f.write("\t".join(["cell", "donor_id", "prob_max", "prob_doublet", "n_vars",
                           "best_singlet", "best_doublet", "doublet_logLikRatio"]) + "\n")
        for i in range(len(cell_names)):
            f.write("\t".join([cell_names[i], donor_ids[i], "%.2e" % prob_max[i],
                               "%.2e" % prob_dbl[i], "%d" % n_vars[i], best_singlet[i],
                               best_doublet[i], "%.3f" % res_vireo['doublet_LLR'][i]]) + "\n")

    if res_vireo.get('ambient_Psi') is not None:      # io_utils.py:157-164, not gzipped
        psi, llr = res_vireo['ambient_Psi'], res_vireo['Psi_LLRatio']
        with open(out_dir + "/prop_ambient.tsv", "w") as f:
            f.write("\t".join(["cell"] + list(donor_names) + ['logLik_ratio']) + "\n")
            for i in range(len(cell_names)):
                f.write("\t".join([cell_names[i]] + ["%.4e" % x for x in psi[i, :]] +
                                   ["%.2f" % llr[i]]) + "\n")

    for name, header, table in (("prob_singlet.tsv", donor_names, ID_prob),
                                ("prob_doublet.tsv", pair_names, doublet_prob)):
        _write_table_gz(out_dir + "/" + name + ".gz", ["cell"] + list(header), cell_names, table)
