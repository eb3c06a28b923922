// SNP-to-gene matching (vrx_genematch_*) and gene-level counts (vrx_genecount_*): snp_gene_match
// (vireoSNP/utils/vcf_utils.py:423-491) for every SNP in two launches, and the G @ AD, G @ DP that follow it.
// Included by vrx_genematch.hip only.  Integers throughout: every result equals the reference's exactly.
//
// Matching.  For a SNP at pos and a gene (start, stop) of its chromosome (:468-473)
//   d1 = start - pos, d2 = stop - pos, dist = sign(d1) sign(d2) min(|d1|, |d2|)
// All coordinates lie in [0, 2^31 - 1], so d1, d2 and dist lie in [-(2^31 - 1), 2^31 - 1]: 32-bit arithmetic is
// exact.  Where a sign is 0 the minimum is 0 as well, so dist = (d1 < 0) != (d2 < 0) ? -m : m.  The walk over
// the gaps (:466-482) asks "is {g : dist_g < gap_k} empty" for k = 0, 1, ...: it is not exactly when the
// smallest dist of the chromosome is below gap_k, so the first pass needs the minimum alone to find k, and
// "dist < gap" is evaluated as dist <= gap - 1 with gap - 1 clamped to the int32 range (below -(2^31 - 1)
// nothing matches, from 2^31 - 1 on everything does).  The nearest gene (:481) is np.argmin over the matching
// genes in gene_df row order -- the first row that reaches the chromosome's minimum, since that minimum is
// below the gap; several genes (gap <= 0 and multi_gene) are all rows with dist <= gap - 1 in row order.
//
// One lane per SNP, the SNPs sorted by chromosome code (perm[j] = where the j-th sorted SNP's results go, so
// the results are in the caller's order whatever the input interleaving).  A workgroup covers 256 consecutive
// sorted SNPs, hence a contiguous range of codes -- one code nearly always; for every code of the range it
// stages the chromosome's (start, stop) pairs tile by tile in LDS, and the lanes of that code walk the tile.
// Every such lane reads the same LDS address in the same instruction: a broadcast, no bank conflict.
//   pass 1   walk for (minimum, first row reaching it); pick k; if the answer is a set, walk again and count
//   scan     exclusive sum of the counts (hipCUB)
//   pass 2   the single row, or walk once more and write the rows with dist <= gap_k - 1 in order
// The count walk and the emit walk evaluate the same predicate on the same data, so a lane writes exactly
// `count` rows from its offset: no atomics, no bound to overrun.
//
// Gene counts.  Every entry (variant v, cell c, ad, dp) of the merged CSC becomes one (key, value) per gene
// of v, key = c n_gene + gene and value = ad 2^32 + dp; a radix sort by key (hipCUB) brings equal (cell, gene)
// together, in column-major order, and the first entry of every run adds up its run in 64 bits.
#pragma once

#include "vrx_common.h"

constexpr int VRX_GM_BLOCK = 256;  // SNPs of a workgroup
constexpr int VRX_GM_TILE = 1024;  // genes of one LDS tile: 8 KiB of (start, stop)

struct VrxGmArgs {
    int64_t n_snp;
    const int32_t* code;       // by sorted position, non-decreasing
    const int32_t* pos;        // by sorted position
    const int32_t* perm;       // sorted position -> output index
    const int32_t* chrom_ptr;  // n_chrom + 1 offsets into gene / grow
    const int2* gene;          // (start, stop), grouped by code, gene_df row order inside a code
    const int32_t* grow;       // gene_df row of a grouped gene
    int32_t n_gap;
    const int32_t* gap_m1;     // gap - 1, clamped
    const uint8_t* single;     // gap > 0 or not multi_gene: the answer is the nearest gene
    int32_t* flag;             // by output index
    int64_t* count;            // by output index
    const int64_t* offset;     // by output index: exclusive sum of count
    int32_t* thr;              // by sorted position: gap_m1 of the winning gap
    int32_t* first;            // by sorted position: gene_df row of the nearest gene, -1 without genes
    uint8_t* multi;            // by sorted position: the answer is the set {dist <= thr}
    int32_t* rows;             // the ragged lists
};

__device__ __forceinline__ int32_t vrx_gm_dist(int2 g, int32_t pos) {
    const int32_t d1 = g.x - pos, d2 = g.y - pos;
    const int32_t a1 = d1 < 0 ? -d1 : d1, a2 = d2 < 0 ? -d2 : d2;
    const int32_t m = a1 < a2 ? a1 : a2;
    return ((d1 < 0) != (d2 < 0)) ? -m : m;
}

// MODE 0: best / first <- minimum and the first grouped gene reaching it (first < 0: none seen yet)
// MODE 1: n <- number of genes with dist <= thr            (lanes with `mine`)
// MODE 2: out[n++] <- gene_df rows of those genes, in order (lanes with `mine`)
// c_lo .. c_hi and therefore every loop bound and barrier are uniform over the workgroup.
template <int MODE>
__device__ __forceinline__ void vrx_gm_walk(const VrxGmArgs& g, int2* tile, int32_t c_lo, int32_t c_hi, bool mine,
                                            int32_t code, int32_t pos, int32_t thr, int32_t& best, int32_t& first,
                                            int64_t& n, int32_t* out) {
    for (int32_t c = c_lo; c <= c_hi; ++c) {
        const int32_t g0 = g.chrom_ptr[c], g1 = g.chrom_ptr[c + 1];
        const bool walk = mine && code == c;
        for (int32_t t0 = g0; t0 < g1; t0 += VRX_GM_TILE) {
            const int nt = g1 - t0 < VRX_GM_TILE ? g1 - t0 : VRX_GM_TILE;
            __syncthreads();  // the previous tile has been read by every lane
            for (int i = threadIdx.x; i < nt; i += VRX_GM_BLOCK) tile[i] = g.gene[t0 + i];
            __syncthreads();
            if (!walk) continue;
            for (int i = 0; i < nt; ++i) {
                const int32_t d = vrx_gm_dist(tile[i], pos);
                if (MODE == 0) {
                    if (first < 0 || d < best) {  // strictly below: the first row keeps a tie
                        best = d;
                        first = t0 + i;
                    }
                } else if (MODE == 1) {
                    n += d <= thr ? 1 : 0;
                } else if (d <= thr) {
                    out[n++] = g.grow[t0 + i];
                }
            }
        }
    }
}

__device__ __forceinline__ void vrx_gm_range(const VrxGmArgs& g, int64_t& j, bool& live, int32_t& c_lo, int32_t& c_hi) {
    const int64_t j0 = (int64_t)blockIdx.x * VRX_GM_BLOCK;  // (< n_snp: the grid is ceil(n_snp / block))
    const int64_t j1 = j0 + VRX_GM_BLOCK < g.n_snp ? j0 + VRX_GM_BLOCK : g.n_snp;
    j = j0 + threadIdx.x;
    live = j < g.n_snp;
    c_lo = g.code[j0];
    c_hi = g.code[j1 - 1];
}

__global__ __launch_bounds__(VRX_GM_BLOCK) void vrx_gm_pass1(VrxGmArgs g) {
    __shared__ int2 tile[VRX_GM_TILE];
    int64_t j;
    bool live;
    int32_t c_lo, c_hi;
    vrx_gm_range(g, j, live, c_lo, c_hi);
    const int32_t code = live ? g.code[j] : -1, pos = live ? g.pos[j] : 0;
    int32_t best = 0, first = -1;
    int64_t n = 0;
    vrx_gm_walk<0>(g, tile, c_lo, c_hi, live, code, pos, 0, best, first, n, nullptr);
    int32_t k = g.n_gap;
    if (first >= 0)
        for (int32_t q = 0; q < g.n_gap; ++q)
            if (best <= g.gap_m1[q]) {
                k = q;
                break;
            }
    const bool hit = live && k < g.n_gap;
    const bool multi = hit && !g.single[k];
    const int32_t thr = hit ? g.gap_m1[k] : 0;
    n = hit ? 1 : 0;
    if (__syncthreads_or(multi)) {
        int64_t m = 0;
        vrx_gm_walk<1>(g, tile, c_lo, c_hi, multi, code, pos, thr, best, first, m, nullptr);
        if (multi) n = m;
    }
    if (live) {
        const int64_t o = g.perm[j];
        g.flag[o] = k;
        g.count[o] = n;
        g.thr[j] = thr;
        g.first[j] = first >= 0 ? g.grow[first] : -1;
        g.multi[j] = multi ? 1 : 0;
    }
}

__global__ __launch_bounds__(VRX_GM_BLOCK) void vrx_gm_pass2(VrxGmArgs g) {
    __shared__ int2 tile[VRX_GM_TILE];
    int64_t j;
    bool live;
    int32_t c_lo, c_hi;
    vrx_gm_range(g, j, live, c_lo, c_hi);
    const int32_t code = live ? g.code[j] : -1, pos = live ? g.pos[j] : 0;
    const int64_t o = live ? g.perm[j] : 0;
    const bool multi = live && g.multi[j];
    int32_t* out = live ? g.rows + g.offset[o] : nullptr;
    if (live && !multi && g.count[o] == 1) out[0] = g.first[j];
    if (__syncthreads_or(multi)) {
        int32_t best = 0, first = 0;
        int64_t n = 0;
        vrx_gm_walk<2>(g, tile, c_lo, c_hi, multi, code, pos, multi ? g.thr[j] : 0, best, first, n, out);
    }
}

// ---- gene counts ----------------------------------------------------------------------------------

constexpr int VRX_GC_BLOCK = 256;

__global__ __launch_bounds__(VRX_GC_BLOCK) void vrx_gc_count(int64_t nnz, const int32_t* __restrict__ rowidx,
                                                             const int64_t* __restrict__ gptr, int64_t* __restrict__ cnt) {
    const int64_t e = (int64_t)blockIdx.x * VRX_GC_BLOCK + threadIdx.x;
    if (e >= nnz) return;
    const int32_t v = rowidx[e];
    cnt[e] = gptr[v + 1] - gptr[v];
}

// the column of entry e: the largest c with colptr[c] <= e (colptr[n_cell] = nnz > e, so c < n_cell)
__device__ __forceinline__ int64_t vrx_gc_column(const int64_t* __restrict__ colptr, int64_t n_cell, int64_t e) {
    int64_t lo = 0, hi = n_cell;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo + 1) / 2;
        if (colptr[mid] <= e)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(VRX_GC_BLOCK) void vrx_gc_emit(int64_t nnz, int64_t n_cell, int64_t n_gene,
                                                            const int64_t* __restrict__ colptr,
                                                            const int32_t* __restrict__ rowidx,
                                                            const int32_t* __restrict__ ad, const int32_t* __restrict__ dp,
                                                            const int64_t* __restrict__ gptr, const int32_t* __restrict__ gid,
                                                            const int64_t* __restrict__ off, uint64_t* __restrict__ key,
                                                            uint64_t* __restrict__ val) {
    const int64_t e = (int64_t)blockIdx.x * VRX_GC_BLOCK + threadIdx.x;
    if (e >= nnz) return;
    const int32_t v = rowidx[e];
    const int64_t q0 = gptr[v], q1 = gptr[v + 1];
    if (q0 == q1) return;
    const uint64_t base = (uint64_t)vrx_gc_column(colptr, n_cell, e) * (uint64_t)n_gene;
    const uint64_t pair = ((uint64_t)(uint32_t)ad[e] << 32) | (uint64_t)(uint32_t)dp[e];
    int64_t t = off[e];
    for (int64_t q = q0; q < q1; ++q, ++t) {
        key[t] = base + (uint64_t)gid[q];
        val[t] = pair;
    }
}

__global__ __launch_bounds__(VRX_GC_BLOCK) void vrx_gc_heads(int64_t n, const uint64_t* __restrict__ key,
                                                             int32_t* __restrict__ head) {
    const int64_t t = (int64_t)blockIdx.x * VRX_GC_BLOCK + threadIdx.x;
    if (t >= n) return;
    head[t] = (t == 0 || key[t] != key[t - 1]) ? 1 : 0;
}

// the first entry of a run adds the run up: 64-bit sums of values below 2^31, at most 2^31 of them
__global__ __launch_bounds__(VRX_GC_BLOCK) void vrx_gc_reduce(int64_t n, const uint64_t* __restrict__ key,
                                                              const uint64_t* __restrict__ val,
                                                              const int32_t* __restrict__ head,
                                                              const int32_t* __restrict__ seg, uint64_t* __restrict__ out_key,
                                                              int64_t* __restrict__ out_ad, int64_t* __restrict__ out_dp) {
    const int64_t t = (int64_t)blockIdx.x * VRX_GC_BLOCK + threadIdx.x;
    if (t >= n || !head[t]) return;
    const uint64_t k = key[t];
    int64_t a = 0, d = 0;
    for (int64_t u = t; u < n && key[u] == k; ++u) {
        a += (int64_t)(val[u] >> 32);
        d += (int64_t)(val[u] & 0xffffffffu);
    }
    const int32_t s = seg[t];
    out_key[s] = k;
    out_ad[s] = a;
    out_dp[s] = d;
}
