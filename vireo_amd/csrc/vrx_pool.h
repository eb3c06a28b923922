// Pooling cell columns of several samples (vrx_pool_* of include/vireo_hip.h): a pooled column is the sum of one
// or two source columns of the merged (ad, dp) CSC, on the union of their row patterns.
//
// Three steps: vrx_pool_pass<false> writes the length of every pooled column (len A for one source, len A + len B -
// shared rows for two), vrx_pool_scan_* turn the lengths into 64-bit offsets, vrx_pool_pass<true> writes the entries.
//
// The merge of a pair carries no dependency from one entry of a column to the next.  An entry of A at index i
// binary-searches B for its row: p = entries of B below that row, and whether B holds the row.  In the merged
// list with shared rows kept twice it would sit at i + p; the shared rows below it -- exactly the entries of
// A[0, i) that B holds too -- are taken off, so its slot is i + p - shared(A[0, i)), and where B holds the row its
// counts are added.  An entry of B at index k searches A the same way and writes itself at k + p - shared(B[0, k))
// only when A lacks its row.  shared(.) is a prefix count of the lanes' own "found" bits: a wavefront ballot and
// a population count, plus the running total of the chunks the group has already walked.  Every output entry is
// written once, by one lane, at a slot that depends on nothing but the two columns.
//
// Column lengths are heavy-tailed (deep cells against shallow ones), so a pooled column whose sources hold up to
// VRX_POOL_WAVE_LIMIT entries goes to one wavefront and a longer one to a whole workgroup; the host orders the
// columns (workgroup columns first).  A summed count of 2^31 or more records the smallest pooled column where it
// happened (atomicMin on one word); the entry is still written, the caller discards the result.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

constexpr int VRX_POOL_BLOCK = 256;
constexpr int VRX_POOL_WAVES = VRX_POOL_BLOCK / 64;
constexpr int VRX_POOL_WAVE_LIMIT = 2048;  // source entries of a pooled column one wavefront walks (32 chunks)
constexpr int VRX_POOL_SCAN_ITEMS = 4;
constexpr int VRX_POOL_SCAN_BLOCK = VRX_POOL_BLOCK * VRX_POOL_SCAN_ITEMS;  // lengths one workgroup scans

struct VrxPoolArgs {
    int64_t n_long, n_short;  // cols[0, n_long): a workgroup each; cols[n_long, n_long + n_short): a wavefront each
    const int32_t* cols;      // pooled column numbers in that order
    const int32_t* src0;      // per pooled column: first source column
    const int32_t* src1;      // second source column or -1
    const int64_t* colptr;    // the sources: n_src + 1 offsets
    const int32_t* row;
    const int32_t* ad;
    const int32_t* dp;
    int64_t* len;        // count: entries of every pooled column
    const int64_t* out;  // emit: n_pool + 1 offsets
    int32_t* orow;
    int32_t* oad;
    int32_t* odp;
    int32_t* bad;  // smallest pooled column with a sum of 2^31 or more (starts at INT32_MAX)
};

// entries of r[0, n) below key (r strictly increasing)
__device__ inline int32_t vrx_pool_lower(const int32_t* __restrict__ r, int32_t n, int32_t key) {
    int32_t lo = 0, hi = n;
    while (lo < hi) {
        const int32_t mid = (int32_t)(((uint32_t)lo + (uint32_t)hi) >> 1);
        if (r[mid] < key)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// Lanes of the group (WG: the workgroup, else the wavefront) below this one with f set; *total = all of them.
// WG: every thread of the workgroup calls it the same number of times; lds holds VRX_POOL_WAVES words.
template <bool WG>
__device__ inline int32_t vrx_pool_rank(bool f, int32_t* total, int32_t* lds) {
    const unsigned long long m = __ballot(f);
    const int l = threadIdx.x & 63;
    const int32_t below = __popcll(m & ((1ull << l) - 1ull));
    const int32_t mine = __popcll(m);
    if constexpr (!WG) {
        *total = mine;
        return below;
    } else {
        const int w = threadIdx.x >> 6;
        __syncthreads();  // (the reads of the call before)
        if (l == 0) lds[w] = mine;
        __syncthreads();
        int32_t before = 0, all = 0;
        for (int k = 0; k < VRX_POOL_WAVES; ++k) {
            const int32_t c = lds[k];
            before += k < w ? c : 0;
            all += c;
        }
        *total = all;
        return below + before;
    }
}

struct VrxPoolCol {
    int64_t a0, b0;
    int32_t na, nb;
};

__device__ inline VrxPoolCol vrx_pool_col(const VrxPoolArgs& g, int32_t j) {
    VrxPoolCol c;
    const int32_t s0 = g.src0[j], s1 = g.src1[j];
    c.a0 = g.colptr[s0];
    c.na = (int32_t)(g.colptr[s0 + 1] - c.a0);
    c.b0 = 0;
    c.nb = 0;
    if (s1 >= 0) {
        c.b0 = g.colptr[s1];
        c.nb = (int32_t)(g.colptr[s1 + 1] - c.b0);
    }
    return c;
}

template <bool WG>
__device__ inline void vrx_pool_count_col(const VrxPoolArgs& g, int32_t j, int32_t* lds) {
    constexpr int32_t W = WG ? VRX_POOL_BLOCK : 64;
    const int32_t lane = WG ? (int32_t)threadIdx.x : (int32_t)(threadIdx.x & 63);
    const VrxPoolCol c = vrx_pool_col(g, j);
    const int32_t* __restrict__ ra = g.row + c.a0;
    const int32_t* __restrict__ rb = g.row + c.b0;
    int32_t shared = 0;
    if (c.nb > 0)
        for (int32_t base = 0; base < c.na; base += W) {
            const int32_t i = base + lane;
            bool f = false;
            if (i < c.na) {
                const int32_t key = ra[i];
                const int32_t p = vrx_pool_lower(rb, c.nb, key);
                f = p < c.nb && rb[p] == key;
            }
            int32_t tot;
            vrx_pool_rank<WG>(f, &tot, lds);
            shared += tot;
        }
    if (lane == 0) g.len[j] = (int64_t)c.na + c.nb - shared;
}

template <bool WG>
__device__ inline void vrx_pool_emit_col(const VrxPoolArgs& g, int32_t j, int32_t* lds) {
    constexpr int32_t W = WG ? VRX_POOL_BLOCK : 64;
    const int32_t lane = WG ? (int32_t)threadIdx.x : (int32_t)(threadIdx.x & 63);
    const VrxPoolCol c = vrx_pool_col(g, j);
    const int32_t* __restrict__ ra = g.row + c.a0;
    const int32_t* __restrict__ rb = g.row + c.b0;
    const int64_t o = g.out[j];
    int32_t carry = 0;
    for (int32_t base = 0; base < c.na; base += W) {  // A: every entry, with B's counts where B holds the row
        const int32_t i = base + lane;
        bool f = false;
        int32_t key = 0, va = 0, vd = 0, p = 0;
        if (i < c.na) {
            key = ra[i];
            va = g.ad[c.a0 + i];
            vd = g.dp[c.a0 + i];
            p = vrx_pool_lower(rb, c.nb, key);
            f = p < c.nb && rb[p] == key;
            if (f) {
                const uint32_t sa = (uint32_t)va + (uint32_t)g.ad[c.b0 + p];
                const uint32_t sd = (uint32_t)vd + (uint32_t)g.dp[c.b0 + p];
                if ((sa | sd) >> 31) atomicMin(g.bad, j);
                va = (int32_t)sa;
                vd = (int32_t)sd;
            }
        }
        int32_t tot = 0, r = 0;
        if (c.nb > 0) r = vrx_pool_rank<WG>(f, &tot, lds);  // (c.nb is the same for the whole group)
        if (i < c.na) {
            const int64_t at = o + i + p - (carry + r);
            g.orow[at] = key;
            g.oad[at] = va;
            g.odp[at] = vd;
        }
        carry += tot;
    }
    carry = 0;
    for (int32_t base = 0; base < c.nb; base += W) {  // B: the entries whose row A lacks
        const int32_t k = base + lane;
        bool f = false;
        int32_t key = 0, p = 0;
        if (k < c.nb) {
            key = rb[k];
            p = vrx_pool_lower(ra, c.na, key);
            f = p < c.na && ra[p] == key;
        }
        int32_t tot;
        const int32_t r = vrx_pool_rank<WG>(f, &tot, lds);
        if (k < c.nb && !f) {
            const int64_t at = o + k + p - (carry + r);
            g.orow[at] = key;
            g.oad[at] = g.ad[c.b0 + k];
            g.odp[at] = g.dp[c.b0 + k];
        }
        carry += tot;
    }
}

// Workgroups [0, n_long) take one column each; the others give one column to each of their wavefronts.
template <bool EMIT>
__global__ __launch_bounds__(VRX_POOL_BLOCK) void vrx_pool_pass(VrxPoolArgs g) {
    __shared__ int32_t lds[VRX_POOL_WAVES];
    const int64_t b = blockIdx.x;
    if (b < g.n_long) {
        const int32_t j = g.cols[b];
        if constexpr (EMIT)
            vrx_pool_emit_col<true>(g, j, lds);
        else
            vrx_pool_count_col<true>(g, j, lds);
        return;
    }
    const int64_t q = (b - g.n_long) * VRX_POOL_WAVES + (threadIdx.x >> 6);
    if (q >= g.n_short) return;
    const int32_t j = g.cols[g.n_long + q];
    if constexpr (EMIT)
        vrx_pool_emit_col<false>(g, j, lds);
    else
        vrx_pool_count_col<false>(g, j, lds);
}

// ---- exclusive scan of the lengths: per workgroup, over the workgroup totals, and their sum ----------------

// inclusive scan over the workgroup's threads of s; *all = the workgroup's total.  ws: VRX_POOL_WAVES words
__device__ inline int64_t vrx_pool_block_scan(int64_t s, int64_t* all, int64_t* ws) {
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
    long long inc = s;
    for (int d = 1; d < 64; d <<= 1) {
        const long long t = __shfl_up(inc, d);
        if (l >= d) inc += t;
    }
    __syncthreads();  // (the reads of the call before)
    if (l == 63) ws[w] = inc;
    __syncthreads();
    int64_t before = 0, sum = 0;
    for (int k = 0; k < VRX_POOL_WAVES; ++k) {
        const int64_t c = ws[k];
        before += k < w ? c : 0;
        sum += c;
    }
    *all = sum;
    return before + inc;
}

// ptr[i] = sum of len[first of the workgroup, i); blk[b] = the workgroup's total
__global__ __launch_bounds__(VRX_POOL_BLOCK) void vrx_pool_scan_local(int64_t n, const int64_t* __restrict__ len,
                                                                      int64_t* __restrict__ ptr,
                                                                      int64_t* __restrict__ blk) {
    __shared__ int64_t ws[VRX_POOL_WAVES];
    const int64_t base = (int64_t)blockIdx.x * VRX_POOL_SCAN_BLOCK + (int64_t)threadIdx.x * VRX_POOL_SCAN_ITEMS;
    int64_t v[VRX_POOL_SCAN_ITEMS], s = 0;
    for (int q = 0; q < VRX_POOL_SCAN_ITEMS; ++q) {
        v[q] = base + q < n ? len[base + q] : 0;
        s += v[q];
    }
    int64_t all;
    int64_t ex = vrx_pool_block_scan(s, &all, ws) - s;
    for (int q = 0; q < VRX_POOL_SCAN_ITEMS; ++q) {
        if (base + q < n) ptr[base + q] = ex;
        ex += v[q];
    }
    if (threadIdx.x == 0) blk[blockIdx.x] = all;
}

// one workgroup: blk[b] = sum of blk[0, b), *total = the sum of all
__global__ __launch_bounds__(VRX_POOL_BLOCK) void vrx_pool_scan_blocks(int64_t nb, int64_t* __restrict__ blk,
                                                                       int64_t* __restrict__ total) {
    __shared__ int64_t ws[VRX_POOL_WAVES];
    int64_t carry = 0;
    for (int64_t base = 0; base < nb; base += VRX_POOL_BLOCK) {
        const int64_t i = base + threadIdx.x;
        const int64_t s = i < nb ? blk[i] : 0;
        int64_t all;
        const int64_t inc = vrx_pool_block_scan(s, &all, ws);
        if (i < nb) blk[i] = carry + inc - s;
        carry += all;
    }
    if (threadIdx.x == 0) *total = carry;
}

__global__ __launch_bounds__(VRX_POOL_BLOCK) void vrx_pool_scan_add(int64_t n, int64_t* __restrict__ ptr,
                                                                    const int64_t* __restrict__ blk) {
    const int64_t i = (int64_t)blockIdx.x * VRX_POOL_BLOCK + threadIdx.x;
    if (i < n) ptr[i] += blk[i / VRX_POOL_SCAN_BLOCK];
}
