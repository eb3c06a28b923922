"""VCF text I/O used by the ``vireo`` command (host side, but for ``load_donor_GPb``).

Own implementation of what the command needs from vireoSNP/utils/vcf_utils.py: loading a
cellSNP / donor VCF (:80-159), its sparse per-cell AD/DP (:192-205), donor genotype
probabilities from GT / GP / PL tags (:299-336), SNP matching with or without the ``chr``
prefix (:339-350) and writing the estimated donor genotypes (:208-296).  Return
structures keep the reference's dict keys so downstream code reads the same.
``load_donor_GPb`` does the donor side of ``vireo -d`` -- load, match to the cell variants,
convert -- in one pass over the text on the GPU (csrc/vrx_vcf.h); the host functions stay
as its yardstick and its host path.
"""
import gzip
import os
import shutil
import subprocess
import sys
import time

import ctypes as C

import numpy as np
from scipy.sparse import csr_matrix

from . import _lib, bgzf
from .gene_match import snp_gene_match                         # noqa: F401  (vcf_utils.py:423-491)
from .vireo_base import donor_match, match

_MISSING = (".", "./.", ".|.")


def _text_lines(path):
    """The lines of a VCF as the reference's loader meets them (vcf_utils.py:112-126): a .gz / .bgz file is read in
    binary, cut at '\\n' only and decoded as UTF-8 one line at a time, so a lone '\\r' stays inside its line and a bad
    byte raises when its line is reached; a plain file is read in text mode.  The '\\n' itself is left off: every
    use of a line starts with rstrip()."""
    if path.endswith(".gz") or path.endswith(".bgz"):
        with gzip.open(path, "rb") as fh:
            rest = b""
            while True:
                block = fh.read(_READ_BYTES)
                if not block:
                    break
                parts = (rest + block).split(b"\n")
                rest = parts.pop()
                for raw in parts:
                    yield raw.decode("utf-8")
            if rest:
                yield rest.decode("utf-8")
    else:
        with open(path, "r") as fh:
            yield from fh


def _sparse_geno(rows, formats, format_list):
    """cells x variants sparse layout of the FORMAT fields (vcf_utils.py:30-57): for every
    variant the cells with a call, one string per requested key."""
    out = {k: [] for k in format_list}
    indices, indptr = [], [0]
    tagged = np.zeros(len(format_list), np.int64)
    want = set(format_list)
    if any(set(fmt) != want for fmt in formats):       # every line's names first (:32-35), then the entries
        print("Error: require the same format for all variants.")
        raise SystemExit
    blank = ":".join(["."] * len(format_list))
    for fmt, calls in zip(formats, rows):
        pos = [fmt.index(k) for k in format_list]
        for cell, call in enumerate(calls):
            if call == blank or call == ".":
                continue
            parts = call.split(":")
            for k, p in zip(format_list, pos):
                out[k].append(parts[p])
            indices.append(cell)
            tagged += 1
        indptr.append(len(indices))
    out["indices"], out["indptr"] = indices, indptr
    out["shape"] = (len(rows[0]) if rows else 0, len(rows))
    return out, tagged


def _dense_geno(rows, formats, format_list):
    """variants x samples lists per key (vcf_utils.py:58-69); absent keys become '.'"""
    out = {k: [] for k in format_list}
    tagged = np.zeros(len(format_list), np.int64)
    for fmt, calls in zip(formats, rows):
        split = [c.split(":") for c in calls]
        for j, k in enumerate(format_list):
            if k in fmt:
                p = fmt.index(k)
                out[k].append([s[p] for s in split])
                tagged[j] += 1
            else:
                out[k].append(["."] * len(split))
    return out, tagged


def load_VCF(vcf_file, biallelic_only=False, load_sample=True, sparse=True,
             format_list=None):
    """-> dict(variants, FixedINFO, contigs, comments[, samples, GenoINFO, n_SNP_tagged])
    like the reference loader (vcf_utils.py:80-159)."""
    fixed, contigs, comments = {}, [], []
    keys, samples, variants, heads, rows = None, [], [], [], []
    n_keys = sys.maxsize                                # before the #CHROM line: more fields than a line has
    for line in _text_lines(vcf_file):
        if line.startswith("#"):
            line = line.rstrip()
            if line.startswith("##contig="):
                contigs.append(line)
            if line.startswith("#CHROM"):
                cols = line[1:].split("\t")
                keys = cols[:8]
                n_keys = len(keys)
                for k in keys:
                    fixed[k] = []
                if load_sample:
                    samples = cols[9:]
            else:
                comments.append(line)
            continue
        f = line.rstrip().split("\t")
        if biallelic_only and (len(f[3]) > 1 or len(f[4]) > 1):
            continue
        if load_sample:
            # FORMAT, or none: looked at after the last line (:22); kept as text, a list per line more slows the
            # garbage collector by a quarter of the whole call
            heads.append(f[8] if len(f) > 8 else None)
            rows.append(f[9:])
        if len(f) < n_keys:                             # the reference indexes f[i] for every key (:145-146)
            if keys is None:
                raise UnboundLocalError("a data line before the #CHROM line: no key_ids yet")
            raise IndexError("list index out of range")
        for k, v in zip(keys, f):
            fixed[k].append(v)
        variants.append("_".join((f[0], f[1], f[3], f[4])))
    if None in heads:                                   # a line of eight fields raises here, after the text
        raise IndexError("list index out of range")
    formats = [x.split(":") for x in heads]
    rv = dict(variants=variants, FixedINFO=fixed, contigs=contigs, comments=comments)
    if load_sample:
        rv["samples"] = samples
        if not rows:
            rv["GenoINFO"], rv["n_SNP_tagged"] = None, None
        else:
            use = format_list if format_list is not None else formats[0]
            geno, tagged = (_sparse_geno if sparse else _dense_geno)(rows, formats, use)
            low = np.where(tagged < 0.1 * len(rows))[0]
            if len(low) > 0:
                print('[vireo] Warning: too few variants with tags!',
                      '\t'.join(use[k] + ": " + str(tagged[k]) for k in range(len(use))))
            rv["GenoINFO"], rv["n_SNP_tagged"] = geno, tagged
    return rv


def read_sparse_GeneINFO(GenoINFO, keys=['AD', 'DP'], axes=[-1, -1]):
    """float64 CSR (variants x cells) per key from the sparse FORMAT layout
    (vcf_utils.py:192-205)."""
    n_cell, n_var = (int(x) for x in GenoINFO['shape'])
    indptr = np.asarray(GenoINFO['indptr'], dtype=int)
    indices = np.asarray(GenoINFO['indices'], dtype=int)
    out = {}
    for key, ax in zip(keys, axes):
        vals = [x.split(",")[ax] for x in GenoINFO[key]]
        data = np.array([v if v != '.' else '0' for v in vals]).astype(float)
        out[key] = csr_matrix((data, indices, indptr), shape=(n_var, n_cell))
    return out


def _parse_codes_vectorised(GT_dat, tag):
    """All genotype codes of a donor VCF at once (the reference converts them one string at a time,
    vcf_utils.py:311-331: seconds per 10^5 variants): the same arithmetic on whole arrays.
    None when the input is not a regular table of well-formed codes."""
    n_var = len(GT_dat)
    n_don = len(GT_dat[0]) if n_var else 0
    if any(len(row) != n_don for row in GT_dat):        # the loop's bounds are the first row's
        return None
    flat = [code for row in GT_dat for code in row]
    missing = np.fromiter((code in _MISSING for code in flat), dtype=bool, count=len(flat))
    good = [code for code, m in zip(flat, missing) if not m]
    P = np.zeros((len(flat), 3))
    P[missing] = 1 / 3
    try:
        if tag == 'GT':
            if any(len(code) < 1 for code in good):
                return None
            first = np.array([code[0] for code in good], dtype=float)
            last = np.array([code[-1] for code in good], dtype=float)
            idx = (first + last).astype(int)
            if good and (idx.min() < 0 or idx.max() > 2):
                return None
            P[np.flatnonzero(~missing), idx] = 1
        else:
            if any(code.count(",") != 2 for code in good):
                return None
            vals = np.array(",".join(good).split(","), dtype=float).reshape(-1, 3) if good \
                else np.zeros((0, 3))
            if tag == 'PL':
                vals = 10 ** (-0.1 * (vals - vals.min(axis=1, keepdims=True)) - 0.025)
            P[~missing] = vals
    except ValueError:
        return None
    return P.reshape(n_var, n_don, 3)


def parse_donor_GPb(GT_dat, tag='GT', min_prob=0.0):
    """(n_var, n_donor, 3) genotype probabilities from GT / GP / PL strings
    (vcf_utils.py:299-336); missing calls are uniform."""
    if tag not in ('GT', 'GP', 'PL'):
        print("[parse_donor_GPb] Error: no support tag: %s" % tag)
        return None
    P = _parse_codes_vectorised(GT_dat, tag)
    if P is None:           # ragged rows or fields that are not three numbers: one code at a time
        P = np.zeros((len(GT_dat), len(GT_dat[0]), 3))
        _parse_codes_one_by_one(GT_dat, tag, P)
    P += min_prob
    P /= P.sum(axis=2, keepdims=True)
    return P


def _parse_codes_one_by_one(GT_dat, tag, P):
    """the reference's own loop (vcf_utils.py:311-331) into the zeroed P, over P's rows and columns as there
    (:328-331): a row with fewer codes raises IndexError, the codes a row has beyond them are not looked at"""
    for i in range(P.shape[0]):
        for j in range(P.shape[1]):
            code = GT_dat[i][j]
            if code in _MISSING:
                P[i, j] = 1 / 3
            elif tag == 'GT':
                P[i, j, int(float(code[0]) + float(code[-1]))] = 1
            elif tag == 'GP':
                P[i, j] = np.array(code.split(','), float)
            else:
                phred = np.array(code.split(','), float)
                P[i, j] = 10 ** (-0.1 * (phred - min(phred)) - 0.025)


def match_SNPs(SNP_ids1, SNPs_ids2):
    """match() with a retry adding the 'chr' prefix on either side (vcf_utils.py:339-350)."""
    idx = match(SNP_ids1, SNPs_ids2)
    if np.mean(idx == None) == 1:                                  # noqa: E711
        idx = match(["chr" + x for x in SNP_ids1], SNPs_ids2)
    if np.mean(idx == None) == 1:                                  # noqa: E711
        idx = match(SNP_ids1, ["chr" + x for x in SNPs_ids2])
    return idx


_TAG_CODE = {'GT': 0, 'PL': 1, 'GP': 2}
_VCF_STATUS = ((1, "equal ids among the cell variants"), (2, "a donor line repeats a matched variant"),
               (4, "two ids share a 64-bit hash"), (8, "a '#' line after the first data line"),
               (16, "a line with fewer than 9 fields"),
               (32, "a non-ASCII byte or a carriage return inside a line"))
_READ_BYTES = 8 << 20
_SLAB_BYTES = 256 << 20
_SLAB_LIMIT = (1 << 31) - 64


_DONOR_STATUS = _VCF_STATUS + ((512, "a sample field without the tag's subfield"),)


def _status_reason(status):
    return "; ".join(text for bit, text in _DONOR_STATUS if status & bit)


def _donor_host(vcf_file, tag, variants, biallelic_only, min_prob, reason):
    """load_donor_GPb as the composition it replaces: load_VCF, match_SNPs, parse_donor_GPb"""
    t0 = time.perf_counter()
    v = load_VCF(vcf_file, biallelic_only=biallelic_only, sparse=False, format_list=[tag])
    rows = v['GenoINFO'][tag] if v['GenoINFO'] is not None else []
    n_tagged = int(v['n_SNP_tagged'][0]) if rows else 0
    if variants is None:
        keep = line = np.arange(len(rows), dtype=np.int64)
        sel = rows
    else:
        mm = match_SNPs(variants, v['variants'])
        keep = np.where(mm != None)[0].astype(np.int64)             # noqa: E711
        line = mm[keep].astype(np.int64)
        sel = [rows[x] for x in line]
    GPb = parse_donor_GPb(sel, tag, min_prob) if sel else np.zeros((0, len(v['samples']), 3))
    sec = dict(inflate=0.0, upload=0.0, kernels=0.0, download=0.0, host=time.perf_counter() - t0)
    return dict(GPb=GPb, samples=v['samples'], keep=keep, line=line, n_lines=len(rows), n_tagged=n_tagged,
                n_repaired=0, path='host', reason=reason, seconds=sec)


class _DonorText:
    """The decompressed bytes of a VCF: the '#' lines at its head, then slabs of whole lines.  A BGZF file is
    inflated on ``device`` unless VIREO_INFLATE=host (bgzf.BgzfReader, which raises bgzf.BgzfStatus for a file
    the device does not vouch for), every other compressed file by gzip; bgzf.last() records which."""

    def __init__(self, path, seconds, device=None):
        t0 = time.perf_counter()
        if not path.endswith((".gz", ".bgz")):
            self.fh = open(path, "rb")
        elif bgzf.wanted() == "host":
            bgzf.note_host(path, "VIREO_INFLATE=host")
            self.fh = gzip.open(path, "rb")
        elif not bgzf.is_bgzf(path):
            bgzf.note_host(path, "not a BGZF file")
            self.fh = gzip.open(path, "rb")
        else:
            self.fh = bgzf.BgzfReader(path, device)
        seconds['inflate'] += time.perf_counter() - t0
        self.seconds = seconds
        self.buf, self.pos, self.eof = bytearray(), 0, False

    def close(self):
        self.fh.close()

    def _more(self):
        t0 = time.perf_counter()
        chunk = self.fh.read(_READ_BYTES)
        self.seconds['inflate'] += time.perf_counter() - t0
        if not chunk:
            self.eof = True
        else:
            del self.buf[:self.pos]
            self.pos = 0
            self.buf += chunk

    def header(self):
        lines = []
        while True:
            if self.pos >= len(self.buf):
                if self.eof:
                    break
                self._more()
                continue
            if self.buf[self.pos] != 0x23:
                break
            end = self.buf.find(b"\n", self.pos)
            if end < 0 and not self.eof:
                self._more()
                continue
            end = len(self.buf) if end < 0 else end + 1
            lines.append(bytes(self.buf[self.pos:end]))
            self.pos = end
        return lines

    def slabs(self, slab_bytes):
        """bytearrays of at most slab_bytes that end at a line end; a longer line gets a slab that holds it"""
        while True:
            while not self.eof and len(self.buf) - self.pos < slab_bytes:
                self._more()
            if self.pos >= len(self.buf):
                return
            cut = self.buf.rfind(b"\n", self.pos, self.pos + slab_bytes)
            while cut < 0:
                cut = self.buf.find(b"\n", self.pos + slab_bytes)
                if cut < 0:
                    if self.eof:
                        cut = len(self.buf) - 1
                    else:
                        self._more()
            slab = self.buf[self.pos:cut + 1]
            self.pos = cut + 1
            yield slab


def load_donor_GPb(vcf_file, tag='GT', variants=None, biallelic_only=True, min_prob=0.0,
                   device=None, slab_bytes=None, force_host=False):
    """Genotype probabilities of the donor VCF's variants that occur in ``variants`` (the cell data's
    "CHROM_POS_REF_ALT" ids), in the order of ``variants``: what ``load_VCF(sparse=False, format_list=[tag])``
    (vcf_utils.py:80-159), ``match_donor_VCF`` (io_utils.py:10-39; ``match_SNPs`` with its "chr" retries, :339-350)
    and ``parse_donor_GPb`` (:299-336) give together, bit for bit, from one pass over the text on the GPU
    (``vrx_vcf_*``).  ``variants=None``: every kept line in file order.  The file is inflated on the device when it is
    BGZF (``vireo_amd.bgzf``; by Python's gzip otherwise, or with VIREO_INFLATE=host) and fed in slabs of whole lines
    (``slab_bytes``, default 256 MiB); the device finds the lines, ids, filter, tag counts,
    matches and the unnormalised values of the codes; rows outside its grammar come back flagged and are parsed
    here by the host functions; ``P += min_prob; P /= P.sum(2)`` is NumPy's.  Returns dict(GPb (n_rows, n_sample,
    3), samples, keep (indices into variants), line (ordinal among the kept lines), n_lines, n_tagged, n_repaired,
    path 'device' | 'host', reason, seconds dict(inflate, upload, kernels, download, host)).  The host path, the
    composition above, is taken with ``force_host`` or VIREO_DONOR_VCF=host and for files whose lines the device
    cannot vouch for (``reason`` says which).  Without ``force_host`` there is no fallback for a missing GPU."""
    if force_host or os.environ.get("VIREO_DONOR_VCF") == "host":
        return _donor_host(vcf_file, tag, variants, biallelic_only, min_prob, "forced")
    if tag not in _TAG_CODE:
        return _donor_host(vcf_file, tag, variants, biallelic_only, min_prob, "tag %s has no device grammar" % tag)
    _lib.require_gpu()
    from .counts import default_device
    L = _lib.lib()
    device = default_device() if device is None else int(device)
    slab_bytes = _SLAB_BYTES if slab_bytes is None else int(slab_bytes)
    if not 1 <= slab_bytes <= _SLAB_LIMIT:
        raise ValueError("slab_bytes must lie in 1 ... %d" % _SLAB_LIMIT)
    t_all = time.perf_counter()
    sec = dict(inflate=0.0, upload=0.0, kernels=0.0, download=0.0, host=0.0)

    def host(reason):
        return _donor_host(vcf_file, tag, variants, biallelic_only, min_prob, reason)

    text = None
    try:
        text = _DonorText(vcf_file, sec, device)
        head = text.header()
        chrom = [x for x in head if x.startswith(b"#CHROM")]
        if any(max(x) >= 0x80 for x in chrom) or any(b"\r" in x.rstrip(b"\r\n") for x in head):
            return host(_status_reason(32))
        samples = chrom[-1].decode("ascii").rstrip()[1:].split("\t")[9:] if chrom else []
        S = len(samples)
        if S == 0:
            return host("no sample columns")
        if variants is None:
            n_ids, blob, off = -1, None, None
        else:
            enc = [str(x).encode() for x in variants]
            n_ids, blob = len(enc), b"".join(enc)
            off = np.zeros(n_ids + 1, dtype=np.int64)
            np.cumsum([len(x) for x in enc], out=off[1:])
        table = 10 ** (-0.1 * np.arange(4096.) - 0.025) if tag == 'PL' else None
        with _lib.Handle("the donor VCF reader", lambda out: L.vrx_vcf_create(
                device, _TAG_CODE[tag], S, int(bool(biallelic_only)), n_ids, blob,
                None if off is None else off.ctypes.data_as(_lib._I64), _lib.dptr(table), out),
                L.vrx_vcf_destroy) as reader:
            info = np.zeros(4, dtype=np.int64)
            t2 = np.zeros(2)
            status = C.c_int32(0)
            for mode in ((-1,) if variants is None else (0, 1, 2)):
                if text is None:                                      # a "chr" retry of match_SNPs: the file once more
                    text = _DonorText(vcf_file, sec, device)
                    text.header()
                _lib.check(L.vrx_vcf_begin(reader.ptr, mode, C.byref(status)))
                if status.value:
                    return host(_status_reason(status.value))
                n_lines = n_tagged = 0
                parts, repair = [], []
                for slab in text.slabs(slab_bytes):
                    if len(slab) > _SLAB_LIMIT:
                        return host("a line of 2 GiB")
                    raw = (C.c_char * len(slab)).from_buffer(slab)
                    _lib.check(L.vrx_vcf_slab(reader.ptr, raw, len(slab), info.ctypes.data_as(_lib._I64),
                                              _lib.dptr(t2)))
                    sec['upload'] += t2[0]
                    sec['kernels'] += t2[1]
                    if info[3]:
                        return host(_status_reason(int(info[3])))
                    n_lines += int(info[0])
                    n_tagged += int(info[1])
                    m = int(info[2])
                    if m == 0:
                        continue
                    rows, slot, line = np.empty((m, S, 3)), np.empty(m, np.int64), np.empty(m, np.int64)
                    flag, span = np.empty(m, np.int32), np.empty((m, 2), np.int64)
                    _lib.check(L.vrx_vcf_rows(reader.ptr, _lib.dptr(rows), slot.ctypes.data_as(_lib._I64),
                                              line.ctypes.data_as(_lib._I64), flag.ctypes.data_as(_lib._I32),
                                              span.ctypes.data_as(_lib._I64), _lib.dptr(t2)))
                    sec['kernels'] += t2[0]
                    sec['download'] += t2[1]
                    parts.append((rows, slot, line, flag))
                    for r in np.flatnonzero(flag):                    # the text of a flagged row outlives its slab
                        repair.append((int(slot[r]), bytes(slab[span[r, 0]:span[r, 1]])))
                    del raw
                text.close()
                text = None
                if parts or variants is None:
                    break
    except bgzf.BgzfStatus as e:                                      # the whole file on the host: gzip raises its own
        return host("BGZF " + e.reason)
    finally:
        if text is not None:
            text.close()

    if parts:
        rows, slot, line, flag = (np.concatenate([p[k] for p in parts]) for k in range(4))
    else:
        rows, slot, line, flag = np.zeros((0, S, 3)), np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int32)
    if variants is not None and len(parts) > 0:
        order = np.argsort(slot, kind="stable")
        rows, slot, line, flag = rows[order], slot[order], line[order], flag[order]
    # the host functions on the flagged lines: FORMAT and the codes in file order (where load_VCF would raise),
    # the values one row at a time in cell order (where parse_donor_GPb would)
    codes = {}
    for where, raw in repair:
        f = raw.decode("ascii").rstrip().split("\t")
        codes[where] = _dense_geno([f[9:]], [f[8].split(":")], [tag])[0][tag][0]
    if repair and flag[0] and len(codes[int(slot[0])]) != S:
        # parse_donor_GPb sizes its result by the first row, which is not the header's sample count here
        return host("the first row has %d sample fields for %d samples" % (len(codes[int(slot[0])]), S))
    if n_lines and n_tagged < 0.1 * n_lines:
        print('[vireo] Warning: too few variants with tags!', tag + ": " + str(n_tagged))
    for r in np.flatnonzero(flag):
        fixed = np.zeros((1, S, 3))
        _parse_codes_one_by_one([codes[int(slot[r])]], tag, fixed)
        rows[r] = fixed[0]
    rows += min_prob
    rows /= rows.sum(axis=2, keepdims=True)
    sec['host'] = time.perf_counter() - t_all - sec['inflate'] - sec['upload'] - sec['kernels'] - sec['download']
    return dict(GPb=rows, samples=samples, keep=slot, line=line, n_lines=n_lines, n_tagged=n_tagged,
                n_repaired=len(repair), path='device', reason=None, seconds=sec)


def match_VCF_samples(VCF_file1, VCF_file2, GT_tag1, GT_tag2):
    """Align the donors of two VCF files by their genotype probabilities (vcf_utils.py:353-420): the
    biallelic variants both files hold (with or without the ``chr`` prefix), the distance between every
    donor of the first and every donor of the second from one pass on the GPU (``donor_match``), and the
    Hungarian assignment.  GT_tag1 / GT_tag2: GT, GP or PL.  Prints the reference's lines and returns its
    dict: matched_GPb_diff, matched_donors1, matched_donors2, full_GPb_diff, full_donors1, full_donors2,
    matched_n_var."""
    dat1 = load_VCF(VCF_file1, biallelic_only=True, sparse=False, format_list=[GT_tag1])
    var_ids1 = np.array(dat1['variants'])
    donors1 = np.array(dat1['samples'])
    GPb1 = parse_donor_GPb(dat1['GenoINFO'][GT_tag1], GT_tag1)
    print('Shape for Geno Prob in VCF1:', GPb1.shape)

    dat2 = load_VCF(VCF_file2, biallelic_only=True, sparse=False, format_list=[GT_tag2])
    var_ids2 = np.array(dat2['variants'])
    donors2 = np.array(dat2['samples'])
    GPb2 = parse_donor_GPb(dat2['GenoINFO'][GT_tag2], GT_tag2)
    print('Shape for Geno Prob in VCF2:', GPb2.shape)

    found = match_SNPs(var_ids2, var_ids1)
    use2 = np.where(found != None)[0]                              # noqa: E711
    use1 = found[use2].astype(int)
    print("n_variants in VCF1, VCF2 and matched: %d, %d, %d" % (var_ids1.shape[0], var_ids2.shape[0], len(use2)))

    idx1, idx2, diff = donor_match(GPb1[use1], GPb2[use2], axis=1, return_delta=True)
    print("aligned donors:")
    print(donors1[idx1])
    print(donors2[idx2])
    return dict(matched_GPb_diff=diff[idx1, :][:, idx2], matched_donors1=donors1[idx1],
                matched_donors2=donors2[idx2], full_GPb_diff=diff, full_donors1=donors1,
                full_donors2=donors2, matched_n_var=len(use1))


class _GenoArrays(dict):
    """What ``GenoINFO_maker`` returns: the reference's dict of per-variant string lists
    (vcf_utils.py:208-231), formed only when somebody reads a tag; ``write_VCF`` takes the integer
    arrays behind it and lets the library format the records."""
    _NAMES = ('0/0', '1/0', '1/1')

    def __init__(self, call, AD, DP, PL):
        super().__init__()
        self.call, self.AD, self.DP, self.PL = call, AD, DP, PL

    def _strings(self, tag):
        n = self.call.shape[0]
        if tag == 'GT':
            return [[self._NAMES[x] for x in self.call[i]] for i in range(n)]
        if tag == 'PL':
            txt = self.PL.astype(str)
            return [[",".join(x) for x in txt[i]] for i in range(n)]
        txt = getattr(self, tag).astype(str)
        return [list(txt[i]) for i in range(n)]

    def __missing__(self, tag):
        if tag not in ('GT', 'AD', 'DP', 'PL'):
            raise KeyError(tag)
        self[tag] = self._strings(tag)
        return dict.__getitem__(self, tag)

    def __contains__(self, tag):
        return tag in ('GT', 'AD', 'DP', 'PL')

    def keys(self):
        return ['GT', 'AD', 'DP', 'PL']

    def __iter__(self):
        return iter(self.keys())

    def __len__(self):
        return 4

    def items(self):
        return [(k, self[k]) for k in self.keys()]


def _labels_blob(labels):
    """(concatenated utf-8 labels, int64 offsets) for the native writers"""
    enc = [str(x).encode() for x in labels]
    off = np.zeros(len(enc) + 1, dtype=np.int64)
    np.cumsum([len(b) for b in enc], out=off[1:])
    return b"".join(enc), off


def GenoINFO_maker(GT_prob, AD_reads, DP_reads):
    """GT / AD / DP / PL of the estimated donor genotypes (vcf_utils.py:208-231): the called
    genotype, the rounded read counts and PL = round(-10 log10 GT_prob).  Floors GT_prob at
    1e-10 in place, like the reference."""
    call = np.argmax(GT_prob, axis=2)
    GT_prob[GT_prob < 10 ** (-10)] = 10 ** (-10)
    PL = np.round(-10 * np.log10(GT_prob)).astype(int)
    return _GenoArrays(call, np.round(AD_reads).astype(int), np.round(DP_reads).astype(int), PL)


_FORMAT_HEADER = {
    "GT": '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">',
    "AD": '##FORMAT=<ID=AD,Number=1,Type=Integer,Description="Read depth for each allele">',
    "DP": '##FORMAT=<ID=DP,Number=1,Type=Integer,Description="Read Depth">',
    "PL": '##FORMAT=<ID=PL,Number=G,Type=Integer,Description="Phred-scaled genotype likelihoods">',
}


def write_VCF(out_file, VCF_dat, GenoTags=['GT', 'AD', 'DP', 'PL']):
    """VCF of the donor genotypes, (b)gzipped when the name ends in .gz
    (vcf_utils.py:234-296)."""
    plain = out_file.split(".gz")[0] if out_file.endswith(".gz") else out_file
    if "samples" not in VCF_dat:
        VCF_dat["samples"] = []
        if GenoTags != []:
            print("No sample available: GenoTags will be ignored.")
    cols = ["CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO", "FORMAT"]
    head = [line for line in VCF_dat['comments']
            if not any(line.startswith("##FORMAT=<ID=" + t) for t in GenoTags)]
    head += [_FORMAT_HEADER[t] for t in GenoTags if t in _FORMAT_HEADER]
    head.append("#" + "\t".join(cols + list(VCF_dat['samples'])))
    geno = VCF_dat.get('GenoINFO')
    if (isinstance(geno, _GenoArrays) and list(GenoTags) == ['GT', 'AD', 'DP', 'PL']
            and geno.PL.shape[2:] == (3,) and geno.call.shape[1] == len(VCF_dat['samples'])
            and len({len(VCF_dat['variants']), geno.call.shape[0], geno.AD.shape[0],
                     geno.DP.shape[0], geno.PL.shape[0]}) == 1
            and geno.AD.shape[1] == geno.DP.shape[1] == geno.PL.shape[1] == geno.call.shape[1]):
        # the records are formatted (and gzipped) by the library from the integer arrays
        fixed = VCF_dat['FixedINFO']
        n = len(VCF_dat['variants'])
        prefix = ["\t".join([fixed[c][i] for c in cols[:8]] + ["GT:AD:DP:PL"]) for i in range(n)]
        blob, off = _labels_blob(prefix)
        i64 = lambda a: np.ascontiguousarray(a, dtype=np.int64)     # noqa: E731
        call = np.ascontiguousarray(geno.call, dtype=np.int8)
        ad, dp, pl = i64(geno.AD), i64(geno.DP), i64(geno.PL)
        void = lambda a: a.ctypes.data_as(C.c_void_p)               # noqa: E731
        # (like the generic path below: the result is always <plain name>.gz)
        _lib.check(_lib.lib().vrx_write_vcf_records(
            (plain + ".gz").encode(), ("\n".join(head) + "\n").encode(), blob, void(off),
            void(call), void(ad), void(dp), void(pl), n, call.shape[1], 1))
        return
    with open(plain, "w") as out:
        for line in head:
            out.write(line + "\n")
        fmt = ":".join(GenoTags)
        for i in range(len(VCF_dat['variants'])):
            rec = [VCF_dat['FixedINFO'][c][i] for c in cols[:8]] + [fmt]
            for s in range(len(VCF_dat['samples'])):
                rec.append(":".join(VCF_dat['GenoINFO'][t][i][s] for t in GenoTags))
            out.write("\t".join(rec) + "\n")
    tool = "bgzip" if shutil.which("bgzip") is not None else "gzip"
    subprocess.run([tool, "-f", plain], stdout=subprocess.PIPE)
