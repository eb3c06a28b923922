// Cell VCF text on the device: the kernels behind the vrx_cellvcf_* entries of include/vireo_hip.h.
//
// cellSNP's cells.vcf.gz has one line per variant and one sample field per cell, nearly all of them '.' or '.:.:.': a
// line is about two bytes per cell long, so no wavefront gets a whole line.  Per slab of whole lines:
//   vrx_vcf_mark, hipcub   the line starts (vrx_vcf.h)
//   vrx_cellvcf_lines      a wavefront per line: rstrip(), the first nine tabs, the biallelic filter, FORMAT compared
//                          on bytes with the FORMAT of the first kept line, the nine field offsets kept for the host,
//                          the number of VRX_CELLVCF_SEGMENT-byte segments its sample region is cut into
//   (hipcub)               segments scanned into a first segment per line, kept lines into row ordinals
//   vrx_cellvcf_count      a wavefront per segment, VRX_VCF_CHUNK bytes per step: tabs by ballot; the lane that holds a
//                          tab owns the field behind it and decides missing / entry on its bytes, reading past the chunk
//                          or the segment on its own; -> tabs and entries of the segment
//   (hipcub)               both scanned: a segment's first cell is the tabs before it in its line, its first entry slot
//                          the entries before it in the slab
//   vrx_cellvcf_emit       the same walk; an entry's lane finds the two subfields, takes the text after the last comma,
//                          parses it and writes (cell, value, value) at its slot
//   vrx_cellvcf_rows       a thread per line: the kept lines compacted into rows (indptr, flag, span, offsets), the
//                          sample-field count checked against the #CHROM line's
// A field belongs to the segment that holds the tab in front of it.  The count and the emit pass classify a field with
// one function, so a slot is never outside the counted entries.  No atomics touch the data: flags and status bits are
// set with atomicOr, the number of flagged lines is an integer sum.  Every read lies below the line's end after rstrip().
#pragma once

#include "vrx_vcf.h"

#define VRX_CELLVCF_SEGMENT 2048    // bytes of a line's sample region per wavefront (a multiple of VRX_VCF_CHUNK)
#define VRX_CELLVCF_FIELD_CAP 1024  // bytes of one sample field an entry's lane walks before it hands the line to the host
#define VRX_CELLVCF_FORMAT_MAX 255  // bytes of FORMAT the device compares
#define VRX_CELLVCF_OFFS 10         // per line: the first nine tabs (the ninth = the end without sample fields), the end

// status bits beside VRX_VCF_ST_COMMENT / _SHORT / _BYTES: any of them sends the whole file down the host path
enum {
    VRX_CELLVCF_ST_FORMAT = 64,     // a kept line whose FORMAT bytes differ from the first kept line's
    VRX_CELLVCF_ST_FIELDS = 128,    // a kept line whose sample-field count is not the #CHROM line's
    VRX_CELLVCF_ST_SUBFIELD = 256,  // an entry with fewer ':' subfields than FORMAT has names (IndexError in load_VCF)
};
enum { VRX_CELLVCF_ROW_REPAIR = 1 };  // row flag: the host parses the values of this line

static_assert(VRX_CELLVCF_SEGMENT % VRX_VCF_CHUNK == 0, "a segment is walked in whole chunks");

// ---- per line -----------------------------------------------------------------------------------------------------
struct VrxCellLinesArgs {
    const uint8_t* text;
    uint32_t n;              // bytes in the slab
    const uint32_t* lstart;  // n_lines
    uint32_t n_lines;
    int32_t biallelic_only;
    const uint8_t* fmt;      // FORMAT of the first kept line of the file
    uint32_t fmt_len;        // 0: no kept line yet (the host saw that this slab has none either)
    // out
    int32_t* kept;           // n_lines
    int32_t* nseg;           // n_lines (+ one zero behind them for the scan)
    uint32_t* off;           // [n_lines][VRX_CELLVCF_OFFS], kept lines only
    uint32_t* status;
};

__global__ __launch_bounds__(VRX_VCF_BLOCK) void vrx_cellvcf_lines(const VrxCellLinesArgs g) {
    const uint32_t line = blockIdx.x * VRX_VCF_WAVES + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (line >= g.n_lines) return;
    const uint8_t* b = g.text;
    const uint32_t s = g.lstart[line];
    uint32_t e = vrx_vcf_raw_end(b, g.n, g.lstart, g.n_lines, line);
    while (e > s && vrx_vcf_space(b[e - 1])) --e;
    int32_t kept = 0;
    uint32_t st = 0, nseg = 0;
    uint32_t tp[9];
    do {
        if (e == s) {
            st = VRX_VCF_ST_SHORT;
            break;
        }
        if (b[s] == '#') {
            st = VRX_VCF_ST_COMMENT;
            break;
        }
        const uint32_t nt = vrx_vcf_nine_tabs(b, s, e, lane, tp);
        if (nt < 8) {
            st = VRX_VCF_ST_SHORT;
            break;
        }
        if (nt < 9) tp[8] = e;
        if (g.biallelic_only && (tp[3] - tp[2] - 1 > 1 || tp[4] - tp[3] - 1 > 1)) break;
        kept = 1;
        const uint32_t fs = tp[7] + 1, fe = tp[8];
        bool differs = fe - fs != g.fmt_len;
        if (!differs) {
            bool d = false;
            for (uint32_t k = lane; k < g.fmt_len; k += 64) d |= b[fs + k] != g.fmt[k];
            differs = __ballot(d) != 0;
        }
        if (differs) st = VRX_CELLVCF_ST_FORMAT;
        nseg = (e - tp[8] + VRX_CELLVCF_SEGMENT - 1) / VRX_CELLVCF_SEGMENT;
    } while (0);
    if (lane == 0) {
        g.kept[line] = kept;
        g.nseg[line] = (int32_t)nseg;
        if (kept) {
            uint32_t* o = g.off + (size_t)line * VRX_CELLVCF_OFFS;
#pragma unroll
            for (int k = 0; k < 9; ++k) o[k] = tp[k];
            o[9] = e;
        }
        if (st) atomicOr(g.status, st);
    }
}

// ---- per segment --------------------------------------------------------------------------------------------------
// the sample field behind the tab at p, in a line that ends at e: '.' or n_fmt dots joined by ':' is a missing call
// (vcf_utils.py:40, :47); every other field, the empty one too, is an entry
__device__ __forceinline__ bool vrx_cellvcf_missing(const uint8_t* b, uint32_t p, uint32_t e, uint32_t n_fmt) {
    uint32_t q = p + 1;
    if (q >= e || b[q] != '.') return false;
    if (q + 1 == e || b[q + 1] == '\t') return true;
    for (uint32_t k = 1; k < n_fmt; ++k) {
        q += 2;
        if (q >= e || b[q - 1] != ':' || b[q] != '.') return false;
    }
    return q + 1 == e || b[q + 1] == '\t';
}

struct VrxCellSegArgs {
    const uint8_t* text;
    const uint32_t* off;       // [n_lines][VRX_CELLVCF_OFFS]
    const int32_t* segbase;    // n_lines + 1: the first segment of every line, the number of segments behind them
    uint32_t n_lines, n_seg;
    uint32_t n_fmt;            // names in FORMAT
    int32_t key0, key1;        // the two subfields that are read
    // the count pass writes these, n_seg each
    int32_t* seg_tabs;
    int32_t* seg_entries;
    // the emit pass reads their exclusive scans (n_seg + 1 each) and writes the entries
    const int32_t* tab0;
    const int32_t* ent0;
    int32_t* cell;
    int32_t* v0;
    int32_t* v1;
    int32_t* lineflag;         // n_lines, zeroed
    uint32_t* status;
};

// the text after the last comma of one subfield, as it is read byte by byte
struct VrxCellValue {
    uint32_t v, n_digit, n_dot, other;
    __device__ void reset() { v = n_digit = n_dot = other = 0; }
    __device__ void take(uint8_t c) {
        const uint32_t d = (uint32_t)c - '0';
        if (d <= 9) {
            v = v * 10 + d;  // (wraps past nine digits, where ok() is false)
            ++n_digit;
        } else if (c == '.') {
            ++n_dot;
        } else {
            other = 1;
        }
    }
    // '.' counts as 0 (vcf_utils.py:202); 1-9 decimal digits are the integer float() makes of them
    __device__ bool ok() const { return !other && ((n_dot == 1 && n_digit == 0) || (n_dot == 0 && n_digit >= 1 && n_digit <= 9)); }
    __device__ int32_t value() const { return n_dot ? 0 : (int32_t)v; }
};

template <bool EMIT>
__device__ __forceinline__ void vrx_cellvcf_walk(const VrxCellSegArgs& g, uint32_t seg, uint32_t lane) {
    // the line of the segment: the first one whose segments end behind seg
    uint32_t lo_l = 0, hi_l = g.n_lines - 1;
    while (lo_l < hi_l) {
        const uint32_t mid = (lo_l + hi_l) >> 1;
        if ((uint32_t)g.segbase[mid + 1] > seg)
            hi_l = mid;
        else
            lo_l = mid + 1;
    }
    const uint32_t line = lo_l;
    const uint32_t first = (uint32_t)g.segbase[line];
    const uint8_t* b = g.text;
    const uint32_t* o = g.off + (size_t)line * VRX_CELLVCF_OFFS;
    const uint32_t e = o[9];
    const uint32_t lo = o[8] + (seg - first) * VRX_CELLVCF_SEGMENT;
    const uint32_t hi = min(lo + (uint32_t)VRX_CELLVCF_SEGMENT, e);
    uint32_t n_tab = 0, n_ent = 0;
    int32_t cell0 = 0, slot0 = 0;
    if (EMIT) {
        cell0 = g.tab0[seg] - g.tab0[first];
        slot0 = g.ent0[seg];
    }
    const unsigned long long below = (1ull << lane) - 1;
    for (uint32_t base = lo; base < hi; base += VRX_VCF_CHUNK) {
        const uint32_t pos = base + lane;
        const bool tab = pos < hi && b[pos] == '\t';
        const bool entry = tab && !vrx_cellvcf_missing(b, pos, e, g.n_fmt);
        const unsigned long long mt = __ballot(tab), me = __ballot(entry);
        if (EMIT && entry) {
            const int32_t j = cell0 + (int32_t)(n_tab + (uint32_t)__popcll(mt & below));
            const int32_t slot = slot0 + (int32_t)(n_ent + (uint32_t)__popcll(me & below));
            uint32_t q = pos + 1;
            const uint32_t lim = min(e, q + (uint32_t)VRX_CELLVCF_FIELD_CAP);
            VrxCellValue t;
            t.reset();
            int32_t sub = 0, val0 = 0, val1 = 0;
            bool bad = false;
            for (; q < lim; ++q) {
                const uint8_t c = b[q];
                if (c == '\t') break;
                if (c == ':') {
                    if (sub == g.key0) val0 = t.value(), bad |= !t.ok();
                    if (sub == g.key1) val1 = t.value(), bad |= !t.ok();
                    ++sub;
                    t.reset();
                } else if (c == ',') {
                    t.reset();
                } else {
                    t.take(c);
                }
            }
            if (sub == g.key0) val0 = t.value(), bad |= !t.ok();
            if (sub == g.key1) val1 = t.value(), bad |= !t.ok();
            if (q == lim && lim < e && b[lim] != '\t') {
                bad = true;  // longer than the cap: the host counts its subfields too
            } else if ((uint32_t)sub + 1 < g.n_fmt) {
                atomicOr(g.status, (uint32_t)VRX_CELLVCF_ST_SUBFIELD);
            }
            g.cell[slot] = j;
            g.v0[slot] = val0;
            g.v1[slot] = val1;
            if (bad) atomicOr(&g.lineflag[line], (int32_t)VRX_CELLVCF_ROW_REPAIR);
        }
        n_tab += (uint32_t)__popcll(mt);
        n_ent += (uint32_t)__popcll(me);
    }
    if (!EMIT && lane == 0) {
        g.seg_tabs[seg] = (int32_t)n_tab;
        g.seg_entries[seg] = (int32_t)n_ent;
    }
}

__global__ __launch_bounds__(VRX_VCF_BLOCK) void vrx_cellvcf_count(const VrxCellSegArgs g) {
    const uint32_t seg = blockIdx.x * VRX_VCF_WAVES + (threadIdx.x >> 6);
    if (seg < g.n_seg) vrx_cellvcf_walk<false>(g, seg, threadIdx.x & 63);
}

__global__ __launch_bounds__(VRX_VCF_BLOCK) void vrx_cellvcf_emit(const VrxCellSegArgs g) {
    const uint32_t seg = blockIdx.x * VRX_VCF_WAVES + (threadIdx.x >> 6);
    if (seg < g.n_seg) vrx_cellvcf_walk<true>(g, seg, threadIdx.x & 63);
}

// ---- kept lines -> rows -------------------------------------------------------------------------------------------
struct VrxCellRowsArgs {
    uint32_t n, n_lines, n_seg;
    int32_t n_sample;
    const uint32_t* lstart;
    const int32_t* kept;
    const int32_t* ord;        // inclusive scan of kept
    const int32_t* segbase;
    const int32_t* tab0;
    const int32_t* ent0;
    const uint32_t* off;
    const int32_t* lineflag;
    // out: a row per kept line, in file order
    int64_t* indptr;           // rows + 1, within the slab
    int32_t* flag;
    int64_t* span;             // [rows][2]: the line's bytes in the slab, line end included
    int32_t* roff;             // [rows][VRX_CELLVCF_OFFS]
    uint32_t* status;
    uint32_t* n_flagged;
};

__global__ __launch_bounds__(VRX_VCF_BLOCK) void vrx_cellvcf_rows(const VrxCellRowsArgs g) {
    const uint32_t line = blockIdx.x * VRX_VCF_BLOCK + threadIdx.x;
    if (line >= g.n_lines) return;
    if (line == g.n_lines - 1) g.indptr[g.ord[line]] = g.ent0[g.n_seg];
    if (!g.kept[line]) return;
    const int32_t r = g.ord[line] - 1;
    const int32_t first = g.segbase[line], last = g.segbase[line + 1];
    if (g.tab0[last] - g.tab0[first] != g.n_sample) atomicOr(g.status, (uint32_t)VRX_CELLVCF_ST_FIELDS);
    g.indptr[r] = g.ent0[first];
    const int32_t f = g.lineflag[line];
    g.flag[r] = f;
    if (f) atomicAdd(g.n_flagged, 1u);
    g.span[(size_t)r * 2] = g.lstart[line];
    g.span[(size_t)r * 2 + 1] = line + 1 < g.n_lines ? g.lstart[line + 1] : g.n;
    const uint32_t* o = g.off + (size_t)line * VRX_CELLVCF_OFFS;
#pragma unroll
    for (int k = 0; k < VRX_CELLVCF_OFFS; ++k) g.roff[(size_t)r * VRX_CELLVCF_OFFS + k] = (int32_t)o[k];
}
