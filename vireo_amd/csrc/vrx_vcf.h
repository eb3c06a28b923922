// Donor VCF text on the device: the kernels behind the vrx_vcf_* entries of include/vireo_hip.h.
//
// A slab is a run of whole lines of the decompressed file.  Per slab:
//   vrx_vcf_mark    one flag per byte (the byte starts a line) and the number of lines; bytes on which Python's text
//                   layer would change the line structure (non-ASCII, a '\r' not followed by '\n') set a status bit
//   (hipcub)        the flagged positions compacted into the line starts
//   vrx_vcf_lines   a wavefront per line: rstrip(), the first nine tabs by ballot over VRX_VCF_CHUNK bytes per step,
//                   the biallelic filter, the position of the tag in FORMAT, every sample field of the line counted
//                   for the tag's subfield (the one thing load_VCF asks of a line nobody matches), the 64-bit hash of
//                   CHROM_POS_REF_ALT,
//                   a binary search of the sorted cell hashes, the hit verified on the bytes, the cell variant's slot
//                   claimed with an integer compare-and-swap
//   (hipcub)        kept lines scanned into file ordinals, matched lines compacted
//   vrx_vcf_rows    a wavefront per matched line: the tabs after FORMAT by ballot, one lane per sample field, the
//                   three unnormalised values of the tag's code written to the row
// Integers, table entries and one correctly rounded division only: a row is bitwise a function of its line.
// Whatever is outside the accepted grammar is flagged for the host and never guessed at.
// vrx_vcf_mark, vrx_vcf_space, vrx_vcf_raw_end and vrx_vcf_nine_tabs also serve the cell VCF kernels (vrx_cellvcf.h).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#define VRX_VCF_CHUNK 64  // bytes of a line that one wavefront looks at per step (one byte per lane)
#define VRX_VCF_BLOCK 256
#define VRX_VCF_WAVES (VRX_VCF_BLOCK / 64)
#define VRX_VCF_MARK_BYTES 16  // bytes per thread of vrx_vcf_mark
#define VRX_VCF_PL_MAX 4095

enum { VRX_VCF_GT = 0, VRX_VCF_PL = 1, VRX_VCF_GP = 2 };
// status bits: any of them sends the whole call down the host path
enum {
    VRX_VCF_ST_DUP_CELL = 1,    // two cell ids with the same bytes
    VRX_VCF_ST_DUP_DONOR = 2,   // a second donor line claimed a cell variant
    VRX_VCF_ST_COLLISION = 4,   // equal hashes on different bytes
    VRX_VCF_ST_COMMENT = 8,     // a '#' line after the first data line
    VRX_VCF_ST_SHORT = 16,      // a line with fewer than 9 fields (load_VCF indexes f[8])
    VRX_VCF_ST_BYTES = 32,      // a non-ASCII byte or a '\r' that is not followed by '\n'
    // (64, 128 and 256 are the cell reader's, vrx_cellvcf.h)
    VRX_VCF_ST_SUBFIELD = 512,  // a sample field of a kept line without the tag's subfield (IndexError in load_VCF)
};
enum { VRX_VCF_ROW_REPAIR = 1 };  // row flag: the host parses this line

// per line, written by vrx_vcf_lines: x = end after rstrip() (bit 31: rstrip() removed something), y = position of the
// ninth tab (= end when the line has 9 fields only), z = index of the tag in FORMAT (-1: absent), w = slot (-1: none)
typedef int4 VrxVcfLine;

__device__ __forceinline__ bool vrx_vcf_space(uint8_t c) {  // what str.rstrip() removes, ASCII
    return c == ' ' || (c >= 9 && c <= 13) || (c >= 28 && c <= 31);
}

// where line `line` of the slab ends: its line end excluded, the last line of a slab may lack one
__device__ __forceinline__ uint32_t vrx_vcf_raw_end(const uint8_t* b, uint32_t n, const uint32_t* lstart, uint32_t n_lines,
                                                    uint32_t line) {
    return line + 1 < n_lines ? lstart[line + 1] - 1 : (b[n - 1] == '\n' ? n - 1 : n);
}

// the first nine tabs of [s, e) into tp, by a whole wavefront: every step looks at VRX_VCF_CHUNK bytes, one per lane.
// -> how many were found (at most 9); the same in every lane
__device__ __forceinline__ uint32_t vrx_vcf_nine_tabs(const uint8_t* b, uint32_t s, uint32_t e, uint32_t lane,
                                                      uint32_t (&tp)[9]) {
    uint32_t nt = 0;
    for (uint32_t base = s; base < e && nt < 9; base += VRX_VCF_CHUNK) {
        const uint32_t pos = base + lane;
        unsigned long long m = __ballot(pos < e && b[pos] == '\t');
        while (m && nt < 9) {
            const uint32_t p = base + (uint32_t)__builtin_ctzll(m);
            m &= m - 1;
#pragma unroll
            for (int k = 0; k < 9; ++k)
                if (nt == (uint32_t)k) tp[k] = p;
            ++nt;
        }
    }
    return nt;
}

// 64-bit FNV-1a, one byte at a time: the cell ids and the ids of the donor lines go through this one function
__device__ __forceinline__ uint64_t vrx_vcf_hash_step(uint64_t h, uint8_t c) {
    return (h ^ (uint64_t)c) * 0x100000001B3ull;
}
#define VRX_VCF_HASH_SEED 0xCBF29CE484222325ull

// CHROM_POS_REF_ALT of a line as a byte sequence (vcf_utils.py:100), optionally with "chr" in front
struct VrxVcfId {
    const uint8_t* b;
    uint32_t s[4], e[4];
    int chr;
    __device__ uint32_t size() const {
        return (chr ? 3u : 0u) + 3u + (e[0] - s[0]) + (e[1] - s[1]) + (e[2] - s[2]) + (e[3] - s[3]);
    }
    template <class F>
    __device__ void each(F&& f) const {
        if (chr) {
            f((uint8_t)'c');
            f((uint8_t)'h');
            f((uint8_t)'r');
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k) f((uint8_t)'_');
            for (uint32_t p = s[k]; p < e[k]; ++p) f(b[p]);
        }
    }
};

// ---- cell table ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(VRX_VCF_BLOCK) void vrx_vcf_hash_ids(const uint8_t* bytes, const int64_t* off, int64_t n,
                                                                   uint64_t* hash, int32_t* idx) {
    const int64_t i = (int64_t)blockIdx.x * VRX_VCF_BLOCK + threadIdx.x;
    if (i >= n) return;
    uint64_t h = VRX_VCF_HASH_SEED;
    for (int64_t p = off[i]; p < off[i + 1]; ++p) h = vrx_vcf_hash_step(h, bytes[p]);
    hash[i] = h;
    idx[i] = (int32_t)i;
}

// neighbours of the sorted table with equal hashes: compared on bytes
__global__ __launch_bounds__(VRX_VCF_BLOCK) void vrx_vcf_table_check(const uint8_t* bytes, const int64_t* off, int64_t n,
                                                                      const uint64_t* hash, const int32_t* idx,
                                                                      uint32_t* status) {
    const int64_t i = (int64_t)blockIdx.x * VRX_VCF_BLOCK + threadIdx.x + 1;
    if (i >= n || hash[i] != hash[i - 1]) return;
    const int64_t a = off[idx[i]], b = off[idx[i - 1]];
    const int64_t la = off[idx[i] + 1] - a, lb = off[idx[i - 1] + 1] - b;
    bool same = la == lb;
    for (int64_t k = 0; same && k < la; ++k) same = bytes[a + k] == bytes[b + k];
    atomicOr(status, same ? VRX_VCF_ST_DUP_CELL : VRX_VCF_ST_COLLISION);
}

// ---- line starts --------------------------------------------------------------------------------------------------
// flag has room for n rounded up to VRX_VCF_MARK_BYTES, text for 16 bytes more than that
__global__ __launch_bounds__(VRX_VCF_BLOCK) void vrx_vcf_mark(const uint8_t* text, uint32_t n, uint8_t* flag,
                                                               uint32_t* n_lines, uint32_t* status) {
    __shared__ uint32_t block_lines;
    if (threadIdx.x == 0) block_lines = 0;
    __syncthreads();
    const uint64_t base64 = ((uint64_t)blockIdx.x * VRX_VCF_BLOCK + threadIdx.x) * VRX_VCF_MARK_BYTES;
    uint32_t count = 0;
    bool bad = false;
    if (base64 < n) {
        const uint32_t base = (uint32_t)base64;
        uint8_t c[VRX_VCF_MARK_BYTES + 1];
        if (base + VRX_VCF_MARK_BYTES < n) {
            const uint4 v = *reinterpret_cast<const uint4*>(text + base);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < VRX_VCF_MARK_BYTES; ++k) c[k] = (uint8_t)(w[k >> 2] >> ((k & 3) * 8));
            c[VRX_VCF_MARK_BYTES] = text[base + VRX_VCF_MARK_BYTES];
        } else {
#pragma unroll
            for (int k = 0; k <= VRX_VCF_MARK_BYTES; ++k) c[k] = base + k < n ? text[base + k] : (uint8_t)0;
        }
        uint8_t prev = base ? text[base - 1] : (uint8_t)'\n';
        uint32_t f[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < VRX_VCF_MARK_BYTES; ++k) {
            const bool valid = base + k < n;
            const uint32_t start = valid && prev == '\n';
            f[k >> 2] |= start << ((k & 3) * 8);
            count += start;
            // (past the end c[k + 1] is 0: a '\r' that ends the data is a line end of its own for Python)
            if (valid && (c[k] >= 0x80 || (c[k] == '\r' && c[k + 1] != '\n'))) bad = true;
            prev = c[k];
        }
        *reinterpret_cast<uint4*>(flag + base) = make_uint4(f[0], f[1], f[2], f[3]);
    }
    if (count) atomicAdd(&block_lines, count);
    if (bad) atomicOr(status, (uint32_t)VRX_VCF_ST_BYTES);
    __syncthreads();
    if (threadIdx.x == 0 && block_lines) atomicAdd(n_lines, block_lines);
}

// ---- per line -----------------------------------------------------------------------------------------------------
struct VrxVcfLinesArgs {
    const uint8_t* text;
    uint32_t n;               // bytes in the slab
    const uint32_t* lstart;   // n_lines
    uint32_t n_lines;
    int32_t tag;              // VRX_VCF_GT / PL / GP
    int32_t biallelic_only;
    int32_t mode;             // -1: no matching; 0: ids as they are; 1: "chr" + cell id; 2: "chr" + donor id
    // the cell table
    int64_t n_ids;
    const uint8_t* id_bytes;
    const int64_t* id_off;
    const uint64_t* hash;     // sorted
    const int32_t* idx;       // the cell variant of every sorted hash
    int32_t* claim;           // n_ids, 0 = free
    // out
    int32_t* kept;
    int32_t* tagged;
    uint8_t* match;
    VrxVcfLine* rec;
    uint32_t* status;
};

__global__ __launch_bounds__(VRX_VCF_BLOCK) void vrx_vcf_lines(const VrxVcfLinesArgs g) {
    const uint32_t line = blockIdx.x * VRX_VCF_WAVES + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (line >= g.n_lines) return;
    const uint8_t* b = g.text;
    const uint32_t s = g.lstart[line];
    const uint32_t raw_end = vrx_vcf_raw_end(b, g.n, g.lstart, g.n_lines, line);
    uint32_t e = raw_end;
    while (e > s && vrx_vcf_space(b[e - 1])) --e;
    int32_t kept = 0, tagidx = -1, slot = -1;
    uint32_t samp = e, st = 0;
    do {
        if (e == s) {
            st = VRX_VCF_ST_SHORT;
            break;
        }
        if (b[s] == '#') {
            st = VRX_VCF_ST_COMMENT;
            break;
        }
        // the first nine tabs: every step looks at VRX_VCF_CHUNK bytes, one per lane
        uint32_t tp[9];
        const uint32_t nt = vrx_vcf_nine_tabs(b, s, e, lane, tp);
        if (nt < 8) {
            st = VRX_VCF_ST_SHORT;
            break;
        }
        VrxVcfId id;
        id.b = b;
        id.chr = g.mode == 2;
        id.s[0] = s, id.e[0] = tp[0];
        id.s[1] = tp[0] + 1, id.e[1] = tp[1];
        id.s[2] = tp[2] + 1, id.e[2] = tp[3];
        id.s[3] = tp[3] + 1, id.e[3] = tp[4];
        if (g.biallelic_only && (id.e[2] - id.s[2] > 1 || id.e[3] - id.s[3] > 1)) break;
        kept = 1;
        // FORMAT: the first ':'-separated name equal to the tag (tags have two letters)
        const uint32_t fs = tp[7] + 1, fe = nt >= 9 ? tp[8] : e;
        if (nt >= 9) samp = tp[8];
        const uint8_t t0 = g.tag == VRX_VCF_GT ? 'G' : (g.tag == VRX_VCF_PL ? 'P' : 'G');
        const uint8_t t1 = g.tag == VRX_VCF_GT ? 'T' : (g.tag == VRX_VCF_PL ? 'L' : 'P');
        int32_t k = 0;
        for (uint32_t p = fs; p <= fe;) {
            uint32_t q = p;
            while (q < fe && b[q] != ':') ++q;
            if (q - p == 2 && b[p] == t0 && b[p + 1] == t1) {
                tagidx = k;
                break;
            }
            ++k;
            p = q + 1;
        }
        // load_VCF splits every sample field of a kept line and indexes the tag's subfield (vcf_utils.py:60-65),
        // whether a cell variant matches the line or not: a field with fewer subfields raises there
        if (tagidx > 0 && nt >= 9) {
            bool lacks = false;
            for (uint32_t base = tp[8]; base < e; base += VRX_VCF_CHUNK) {
                const uint32_t pos = base + lane;
                if (pos < e && b[pos] == '\t') {  // the lane that holds a tab counts the ':' of the field behind it
                    int32_t need = tagidx;
                    for (uint32_t p = pos + 1; p < e && b[p] != '\t' && need > 0; ++p) need -= b[p] == ':';
                    lacks |= need > 0;
                }
            }
            if (__ballot(lacks) != 0) st = VRX_VCF_ST_SUBFIELD;
        }
        if (g.mode < 0) {
            slot = 0;
            break;
        }
        if (g.n_ids == 0) break;
        if (g.mode == 1) {  // "chr" + cell id == donor id: the donor id without its first three bytes
            if (!(id.e[0] - id.s[0] >= 3 && b[s] == 'c' && b[s + 1] == 'h' && b[s + 2] == 'r')) break;
            id.s[0] += 3;
        }
        uint64_t h = VRX_VCF_HASH_SEED;
        id.each([&](uint8_t c) { h = vrx_vcf_hash_step(h, c); });
        int64_t lo = 0, hi = g.n_ids;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (g.hash[mid] < h)
                lo = mid + 1;
            else
                hi = mid;
        }
        if (lo >= g.n_ids || g.hash[lo] != h) break;
        const int32_t cell = g.idx[lo];
        const int64_t c0 = g.id_off[cell];
        const uint32_t len = (uint32_t)(g.id_off[cell + 1] - c0);
        bool same = len == id.size();
        uint32_t at = 0;
        id.each([&](uint8_t c) {
            if (same && (at >= len || g.id_bytes[c0 + at] != c)) same = false;
            ++at;
        });
        if (!same) {
            st = VRX_VCF_ST_COLLISION;
            break;
        }
        int32_t old = 0;
        if (lane == 0) old = atomicCAS(&g.claim[cell], 0, 1);
        old = __shfl(old, 0);
        if (old != 0) {
            st = VRX_VCF_ST_DUP_DONOR;
            break;
        }
        slot = cell;
    } while (0);
    if (lane == 0) {
        g.kept[line] = kept;
        g.tagged[line] = kept && tagidx >= 0;
        g.match[line] = slot >= 0;
        g.rec[line] = make_int4((int32_t)(e | (e != raw_end ? 0x80000000u : 0u)), (int32_t)samp, tagidx, slot);
        if (st) atomicOr(g.status, st);
    }
}

// ---- per matched line ----------------------------------------------------------------------------------------------
__device__ const double VRX_VCF_P10[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                                            1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};

// an unsigned decimal integer of at most VRX_VCF_PL_MAX at [p, q): false when it is anything else
__device__ __forceinline__ bool vrx_vcf_uint(const uint8_t* b, uint32_t p, uint32_t q, uint32_t* out) {
    if (p >= q || q - p > 9) return false;
    uint32_t v = 0;
    for (; p < q; ++p) {
        const uint32_t d = (uint32_t)b[p] - '0';
        if (d > 9) return false;
        v = v * 10 + d;
    }
    *out = v;
    return v <= VRX_VCF_PL_MAX;
}

// digits[.digits] at [p, q) with at most 15 significant and 22 fractional digits: the digits as an integer over an
// exact power of ten, both exact doubles, so the quotient is the correctly rounded value that float() returns
__device__ __forceinline__ bool vrx_vcf_decimal(const uint8_t* b, uint32_t p, uint32_t q, double* out) {
    uint64_t m = 0;
    uint32_t n_int = 0, n_frac = 0;
    bool dot = false;
    for (; p < q; ++p) {
        const uint8_t c = b[p];
        if (c == '.') {
            if (dot) return false;
            dot = true;
            continue;
        }
        const uint32_t d = (uint32_t)c - '0';
        if (d > 9) return false;
        m = m * 10 + d;
        if (m >= 1000000000000000ull) return false;
        if (dot)
            ++n_frac;
        else
            ++n_int;
    }
    if (n_int == 0 || (dot && n_frac == 0) || n_frac > 22) return false;
    *out = (double)m / VRX_VCF_P10[n_frac];
    return true;
}

// the code at [p, q) -> three unnormalised values (vcf_utils.py:311-331); false: outside the accepted grammar
__device__ __forceinline__ bool vrx_vcf_code(const uint8_t* b, uint32_t p, uint32_t q, int tag, const double* pl_table,
                                             double* v) {
    const uint32_t len = q - p;
    if ((len == 1 && b[p] == '.') || (len == 3 && b[p] == '.' && b[p + 2] == '.' && (b[p + 1] == '/' || b[p + 1] == '|'))) {
        v[0] = v[1] = v[2] = 1.0 / 3;
        return true;
    }
    if (tag == VRX_VCF_GT) {
        if (len < 1) return false;
        const uint32_t d0 = (uint32_t)b[p] - '0', d1 = (uint32_t)b[q - 1] - '0';
        if (d0 > 9 || d1 > 9 || d0 + d1 > 2) return false;
        v[0] = d0 + d1 == 0, v[1] = d0 + d1 == 1, v[2] = d0 + d1 == 2;
        return true;
    }
    // three comma-separated numbers
    uint32_t c1 = p;
    while (c1 < q && b[c1] != ',') ++c1;
    uint32_t c2 = c1 + 1;
    while (c2 < q && b[c2] != ',') ++c2;
    if (c1 >= q || c2 >= q) return false;
    for (uint32_t r = c2 + 1; r < q; ++r)
        if (b[r] == ',') return false;
    if (tag == VRX_VCF_PL) {
        uint32_t a[3];
        if (!vrx_vcf_uint(b, p, c1, a) || !vrx_vcf_uint(b, c1 + 1, c2, a + 1) || !vrx_vcf_uint(b, c2 + 1, q, a + 2))
            return false;
        const uint32_t lo = min(a[0], min(a[1], a[2]));
        v[0] = pl_table[a[0] - lo], v[1] = pl_table[a[1] - lo], v[2] = pl_table[a[2] - lo];
        return true;
    }
    return vrx_vcf_decimal(b, p, c1, v) && vrx_vcf_decimal(b, c1 + 1, c2, v + 1) && vrx_vcf_decimal(b, c2 + 1, q, v + 2);
}

struct VrxVcfRowsArgs {
    const uint8_t* text;
    uint32_t n, n_lines;
    const uint32_t* lstart;
    const VrxVcfLine* rec;
    const int32_t* ord;       // inclusive scan of kept
    const int32_t* mlist;     // the matched lines of the slab, in file order
    int64_t first, count;     // this launch: matched rows [first, first + count)
    int64_t line_base;        // kept lines of the slabs before this one
    int32_t tag, n_sample, matching;
    const double* pl_table;   // VRX_VCF_PL_MAX + 1 entries
    // out, `count` rows each
    double* gpb;              // [count][n_sample][3]
    int64_t* slot;
    int64_t* ordinal;
    int32_t* flag;
    int64_t* span;            // [count][2]: the line's bytes in the slab, line end included
};

__global__ __launch_bounds__(VRX_VCF_BLOCK) void vrx_vcf_rows(const VrxVcfRowsArgs g) {
    const int64_t r = (int64_t)blockIdx.x * VRX_VCF_WAVES + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (r >= g.count) return;
    const uint8_t* b = g.text;
    const uint32_t line = (uint32_t)g.mlist[g.first + r];
    const VrxVcfLine rec = g.rec[line];
    const uint32_t e = (uint32_t)rec.x & 0x7FFFFFFFu;
    const int32_t tagidx = rec.z;
    const uint32_t S = (uint32_t)g.n_sample;
    double* out = g.gpb + r * (int64_t)S * 3;
    bool bad = false;
    uint32_t n_field = 0;
    // the ninth tab opens sample field 0: every later tab opens the next one, and the lane that holds a tab parses
    // the field behind it
    for (uint32_t base = (uint32_t)rec.y; base < e; base += VRX_VCF_CHUNK) {
        const uint32_t pos = base + lane;
        const bool tab = pos < e && b[pos] == '\t';
        const unsigned long long m = __ballot(tab);
        const uint32_t j = n_field + (uint32_t)__popcll(m & ((1ull << lane) - 1));
        if (tab && j < S) {
            uint32_t p = pos + 1, q = p;
            while (q < e && b[q] != '\t') ++q;
            double v[3] = {0.0, 0.0, 0.0};
            bool ok = true;
            if (tagidx < 0) {  // a FORMAT without the tag: every sample counts as '.'
                v[0] = v[1] = v[2] = 1.0 / 3;
            } else {
                for (int32_t k = 0; k < tagidx && ok; ++k) {
                    while (p < q && b[p] != ':') ++p;
                    if (p >= q)
                        ok = false;  // missing subfield
                    else
                        ++p;
                }
                if (ok) {
                    uint32_t t = p;
                    while (t < q && b[t] != ':') ++t;
                    ok = vrx_vcf_code(b, p, t, g.tag, g.pl_table, v);
                }
            }
            if (ok) {
                out[(int64_t)j * 3] = v[0];
                out[(int64_t)j * 3 + 1] = v[1];
                out[(int64_t)j * 3 + 2] = v[2];
            } else {
                bad = true;
            }
        }
        n_field += (uint32_t)__popcll(m);
    }
    const bool repair = __ballot(bad) != 0 || n_field != S || ((uint32_t)rec.x >> 31);
    if (lane == 0) {
        const int64_t ordinal = g.line_base + g.ord[line] - 1;
        g.slot[r] = g.matching ? (int64_t)rec.w : ordinal;
        g.ordinal[r] = ordinal;
        g.flag[r] = repair ? VRX_VCF_ROW_REPAIR : 0;
        g.span[r * 2] = g.lstart[line];
        g.span[r * 2 + 1] = line + 1 < g.n_lines ? g.lstart[line + 1] : g.n;
    }
}
