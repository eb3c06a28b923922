// Barcode selection (vrx_barcode_*): one greedy round of variant_select (vireoSNP/utils/variant_select.py:22-62)
// -- the entropy of every variant's candidate barcodes (barcode_entropy, :5-19), the tie set of the
// maximum, the median filter on var_count and the r-th survivor -- on the device.  Included by
// vrx_barcode.hip only.
//
// The reference decides by float equality, so every variant's entropy is the reference's double, bit for
// bit.  What that takes:
//   order   With single-character categories the barcodes of a round have one length, so np.unique's
//           string order is the order of (class rank, value).  The host keeps a class rank per donor and
//           sends the donors in class order with the class boundaries; a variant's terms are the non-empty
//           bins c(class, value), class-major and value-minor.
//   sums    p = c / K; s = np.sum(p); the terms entr(p / s) are added by np.sum again and divided by
//           log(2).  VrxNpSum is NumPy's rule for a contiguous float64 array of n <= 128 terms: below 8
//           terms one after the other from 0.0; else eight accumulators over the blocks of 8, combined
//           pairwise, then the last n % 8 terms one after the other.  Adds and divisions only, each
//           correctly rounded: nothing here can contract into a fused multiply-add.
//   no log  The device's log is not the host's libm.  s is within a few ulp of 1, so the host tabulates
//           T[j + H][c] = entr((c / K) / s_j) with scipy for s_j = the double bits(1.0) + j, |j| <= H, and a
//           lane looks its terms up by (j, c).  A variant whose j is outside the table is counted and
//           gets NaN; the round then fails -- it is never evaluated approximately.
//
//   vrx_barcode_entropy<NC>  a variant per lane over the donor-major byte matrix GT[K][stride] (the lanes
//                            of a wave read neighbouring bytes); three sweeps over the classes (a
//                            wave-uniform loop): the number of terms, s, the entropy.  The values of a
//                            class are counted in NC registers by compare-adds.  NC = 3 and NC = 10.
//   vrx_barcode_max / _max2  the maximum by value (a NaN never wins), blocks then one block
//   vrx_barcode_flag         tie flags ent == max, by value (+0.0 == -0.0, NaN never tied)
//   vrx_barcode_gather / _median / _flag_ge
//                            var_count of the tied variants; np.median of them once sorted: the middle
//                            one, or (a + b) / 2 of the two middle ones; the filter var_count >= median
// hipCUB compacts the flagged indices (ascending variant index) and sorts the tied counts.
#pragma once

#include <hipcub/hipcub.hpp>

#include "vrx_common.h"

constexpr int VRX_BC_BLOCK = 256;
constexpr int VRX_BC_MAX_DONORS = 128;  // np.sum's recursive branch above 128 terms is not built
constexpr int VRX_BC_MAX_CAT = 10;      // single-character categories
constexpr int VRX_BC_MAX_H = 4096;
constexpr int VRX_BC_MAX_BLOCKS = 1024;  // partial maxima
constexpr int64_t VRX_BC_BITS_ONE = 0x3FF0000000000000LL;
// control words (int32): variants outside the table, tied, kept
enum { VRX_BC_OUTSIDE = 0, VRX_BC_TIED = 1, VRX_BC_KEPT = 2, VRX_BC_CTL_WORDS = 4 };
// scalars (double): the maximum, the median
enum { VRX_BC_MAX = 0, VRX_BC_MEDIAN = 1, VRX_BC_SCALARS = 2 };

// np.sum of n float64 terms fed in order (1 <= n <= 128)
struct VrxNpSum {
    double r[8];
    double res;
    int i, n8;
    __host__ __device__ __forceinline__ void init(int n) {
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = 0.0;  // (0.0 + a == a: the first block only copies)
        res = 0.0;
        i = 0;
        n8 = n < 8 ? 0 : n - (n & 7);
    }
    __host__ __device__ __forceinline__ double combine() const {
        return ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    }
    __host__ __device__ __forceinline__ void add(double a) {
        if (i < n8) {
            const int m = i & 7;
            // (only the blocks of n >= 8 terms come here, and their terms are > 0: adding +0.0 to the
            //  other seven accumulators changes nothing)
#pragma unroll
            for (int j = 0; j < 8; ++j) r[j] += (m == j) ? a : 0.0;
        } else {
            if (i == n8) res = combine();  // (n < 8: the sum of eight zeros, the 0.0 np.sum starts from)
            res += a;
        }
        ++i;
    }
    __host__ __device__ __forceinline__ double finish() { return i == n8 ? combine() : res; }
};

// f(count) for every non-empty bin of variant column `col`, class-major and value-minor
template <int NC, typename F>
__host__ __device__ __forceinline__ void vrx_barcode_walk(const uint8_t* __restrict__ col, size_t stride,
                                                          int n_class, const int32_t* __restrict__ order,
                                                          const int32_t* __restrict__ bnd, F&& f) {
    for (int c = 0; c < n_class; ++c) {
        int cnt[NC];
#pragma unroll
        for (int t = 0; t < NC; ++t) cnt[t] = 0;
        const int d1 = bnd[c + 1];
        for (int d = bnd[c]; d < d1; ++d) {
            const int g = col[(size_t)order[d] * stride];
#pragma unroll
            for (int t = 0; t < NC; ++t) cnt[t] += (g == t);
        }
#pragma unroll
        for (int t = 0; t < NC; ++t)
            if (cnt[t] > 0) f(cnt[t]);
    }
}

// The entropy of the variant whose bytes start at col; table: [2 H + 1][K + 1].  *outside: its normalising
// sum is more than H ulp from 1 (the value is then NaN).  (Host-callable too: the sums are plain C++.)
template <int NC>
__host__ __device__ __forceinline__ double vrx_barcode_variant(const uint8_t* __restrict__ col, size_t stride, int K,
                                                               int n_class, const int32_t* __restrict__ order,
                                                               const int32_t* __restrict__ bnd,
                                                               const double* __restrict__ table, int H, double log2v,
                                                               bool* outside) {
    int n = 0;
    vrx_barcode_walk<NC>(col, stride, n_class, order, bnd, [&](int) { ++n; });
    const double dK = (double)K;
    VrxNpSum acc;
    acc.init(n);
    vrx_barcode_walk<NC>(col, stride, n_class, order, bnd, [&](int c) { acc.add((double)c / dK); });
    const double s = acc.finish();
    const int64_t j = __builtin_bit_cast(int64_t, s) - VRX_BC_BITS_ONE;
    *outside = j < -(int64_t)H || j > (int64_t)H;
    if (*outside) return __builtin_bit_cast(double, (int64_t)0x7FF8000000000000LL);
    const double* T = table + (size_t)(j + H) * (size_t)(K + 1);
    acc.init(n);
    vrx_barcode_walk<NC>(col, stride, n_class, order, bnd, [&](int c) { acc.add(T[c]); });
    return acc.finish() / log2v;
}

// ent[v]: the entropy of variant v; ctl[VRX_BC_OUTSIDE] counts the variants outside the table
template <int NC>
__global__ __launch_bounds__(VRX_BC_BLOCK) void vrx_barcode_entropy(
    int64_t n_var, size_t stride, int K, int n_class, const uint8_t* __restrict__ GT,
    const int32_t* __restrict__ order, const int32_t* __restrict__ bnd, const double* __restrict__ table, int H,
    double log2v, double* __restrict__ ent, int32_t* __restrict__ ctl) {
    const int64_t v = (int64_t)blockIdx.x * VRX_BC_BLOCK + threadIdx.x;
    if (v >= n_var) return;
    bool outside;
    ent[v] = vrx_barcode_variant<NC>(GT + v, stride, K, n_class, order, bnd, table, H, log2v, &outside);
    if (outside) atomicAdd(&ctl[VRX_BC_OUTSIDE], 1);
}

// the larger by value; a NaN on either side loses (a: the running maximum, -inf at the start)
__device__ __forceinline__ double vrx_barcode_larger(double a, double x) { return x > a ? x : a; }

__device__ __forceinline__ double vrx_barcode_block_max(double m) {
    __shared__ double red[VRX_BC_BLOCK];
    red[threadIdx.x] = m;
    __syncthreads();
    for (int w = VRX_BC_BLOCK / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] = vrx_barcode_larger(red[threadIdx.x], red[threadIdx.x + w]);
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(VRX_BC_BLOCK) void vrx_barcode_max(int64_t n, const double* __restrict__ ent,
                                                                double* __restrict__ part) {
    double m = -INFINITY;
    for (int64_t i = (int64_t)blockIdx.x * VRX_BC_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * VRX_BC_BLOCK)
        m = vrx_barcode_larger(m, ent[i]);
    m = vrx_barcode_block_max(m);
    if (threadIdx.x == 0) part[blockIdx.x] = m;
}

__global__ __launch_bounds__(VRX_BC_BLOCK) void vrx_barcode_max2(int n_part, const double* __restrict__ part,
                                                                 double* __restrict__ scal) {
    double m = -INFINITY;
    for (int i = threadIdx.x; i < n_part; i += VRX_BC_BLOCK) m = vrx_barcode_larger(m, part[i]);
    m = vrx_barcode_block_max(m);
    if (threadIdx.x == 0) scal[VRX_BC_MAX] = m;
}

__global__ __launch_bounds__(VRX_BC_BLOCK) void vrx_barcode_flag(int64_t n, const double* __restrict__ ent,
                                                                 const double* __restrict__ scal,
                                                                 uint8_t* __restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * VRX_BC_BLOCK + threadIdx.x;
    if (i < n) flag[i] = ent[i] == scal[VRX_BC_MAX];
}

// keys[i] = var_count of the i-th tied variant
__global__ __launch_bounds__(VRX_BC_BLOCK) void vrx_barcode_gather(const int32_t* __restrict__ ctl,
                                                                   const int32_t* __restrict__ tidx,
                                                                   const double* __restrict__ vc,
                                                                   double* __restrict__ keys) {
    const int64_t i = (int64_t)blockIdx.x * VRX_BC_BLOCK + threadIdx.x;
    if (i < ctl[VRX_BC_TIED]) keys[i] = vc[tidx[i]];
}

// np.median of the sorted tied counts
__global__ void vrx_barcode_median(const int32_t* __restrict__ ctl, const double* __restrict__ sorted,
                                   double* __restrict__ scal) {
    const int n = ctl[VRX_BC_TIED];
    if (n < 1) return;
    scal[VRX_BC_MEDIAN] = (n & 1) ? sorted[n / 2] : (sorted[n / 2 - 1] + sorted[n / 2]) / 2.0;
}

__global__ __launch_bounds__(VRX_BC_BLOCK) void vrx_barcode_flag_ge(const int32_t* __restrict__ ctl,
                                                                    const double* __restrict__ keys,
                                                                    const double* __restrict__ scal,
                                                                    uint8_t* __restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * VRX_BC_BLOCK + threadIdx.x;
    if (i < ctl[VRX_BC_TIED]) flag[i] = keys[i] >= scal[VRX_BC_MEDIAN];
}
