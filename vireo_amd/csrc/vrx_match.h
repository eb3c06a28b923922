// Donor matching (vrx_geno_*): the genotype-distance matrix that optimal_match and donor_select of
// the reference fill one donor pair at a time (vireoSNP/utils/vireo_base.py:197-201, :230-234; used
// by match_VCF_samples, vcf_utils.py:404-405).  Included by vrx_match.hip only.
//
//   D[i][j] = (sum_n sum_t |X[n][i][t] - Z[n][j][t]|) / (n_var * n_gt)
//   X [n_var][k1][n_gt], Z [n_var][k2][n_gt], C-contiguous float64.  An L1 distance: no product to
//   contract, so no GEMM and no MFMA -- a register-tiled fp64 VALU kernel.
//
//   vrx_geno_pass   one streaming pass over a slab of variants of both operands: workgroup
//                   (chunk c, output tile (TI x TJ)) -> part[c][k1][k2], the tile's sums over the
//                   variants of its chunk
//   vrx_geno_sum    acc[i][j] (+)= the partials: 16 runs of chunks, each in chunk order, then the runs in
//                   order; after the last slab / (n_var * n_gt)
//
// A workgroup of 256 lanes is LI x LJ lane positions times n_slice = 256 / (LI * LJ) slices; the lane
// at (li, lj) owns the 4 x 4 register tile i = i0 + li + LI * a, j = j0 + lj + LJ * b (strided: the
// lanes of a wave read neighbouring donors, G doubles apart), so TI = 4 LI <= 64, TJ = 4 LJ <= 256.
// It walks the variant tiles vt = c, c + n_chunk, ... of T variants:
//   load     columns [i0, i0 + TI) of X and [j0, j0 + TJ) of Z for the T variants, coalesced (16-byte
//            loads when row length, offset and width are even), into LDS rows of odd stride
//            (TI * G | 1, TJ * G | 1 doubles: the slices of a wave read different rows)
//   sum      slice s takes the variants v = s, s + n_slice, ... of the tile; per (v, t) a lane
//            reads 4 + 4 doubles from LDS and adds 16 terms |x - z| (one subtraction, the absolute value
//            as the input modifier of the add)
// and at the end adds the slices in slice order (through LDS).  A cell's terms are therefore added in
// the order (variant tile of the chunk, variant of the slice, t), then slices, then chunks (in runs),
// then slabs: fixed for a given grid and slab size, no atomics -- two calls are bitwise identical.  A NaN
// reaches exactly the cells whose donor carries it (fabs keeps it).  All arithmetic is float64.
#pragma once

#include "vrx_common.h"

constexpr int VRX_GENO_BLOCK = 256;
constexpr int VRX_GENO_R = 4;                   // register tile edge
constexpr int VRX_GENO_LDS = 40 * 1024;         // per workgroup, as VRX_BULK_LDS_TILE (4 workgroups per CU)
constexpr int VRX_GENO_MAX_T = 1024;

struct VrxGenoShape {
    int G, LI, LJ, TI, TJ, n_slice, SX, SZ, T;
};

__host__ __device__ inline int vrx_geno_pow2_ceil(int64_t x) {
    int p = 1;
    while (p < x && p < (1 << 20)) p <<= 1;
    return p;
}

// The tile of a (k1, k2, G) problem: as many lane positions as the donors fill (LI <= 16, LJ <= 64,
// LI * LJ <= 256), fewer when G is so large that fewer than 4 variants of both operands fit the LDS
// budget; T = 0: not even one variant fits.
__host__ __device__ inline VrxGenoShape vrx_geno_shape(int64_t k1, int64_t k2, int G) {
    VrxGenoShape h;
    h.G = G;
    h.LI = vrx_geno_pow2_ceil((k1 + VRX_GENO_R - 1) / VRX_GENO_R);
    h.LJ = vrx_geno_pow2_ceil((k2 + VRX_GENO_R - 1) / VRX_GENO_R);
    if (h.LI > 16) h.LI = 16;
    if (h.LJ > 64) h.LJ = 64;
    while (h.LI * h.LJ > VRX_GENO_BLOCK) h.LJ >>= 1;
    const int budget = VRX_GENO_LDS / (int)sizeof(double);
    for (;;) {
        h.TI = VRX_GENO_R * h.LI;
        h.TJ = VRX_GENO_R * h.LJ;
        h.SX = (h.TI * G) | 1;
        h.SZ = (h.TJ * G) | 1;
        h.T = budget / (h.SX + h.SZ);
        if (h.T >= 4 || (h.LI == 1 && h.LJ == 1)) break;
        if (h.LJ >= h.LI)
            h.LJ >>= 1;
        else
            h.LI >>= 1;
    }
    h.n_slice = VRX_GENO_BLOCK / (h.LI * h.LJ);
    if (h.T > VRX_GENO_MAX_T) h.T = VRX_GENO_MAX_T;
    if (h.T > h.n_slice) h.T -= h.T % h.n_slice;  // every slice the same number of variants of a full tile
    return h;
}
// LDS (doubles): X tile [T][SX] | Z tile [T][SZ]; reused for the slices' sums [16][256]
__host__ __device__ inline size_t vrx_geno_lds_doubles(const VrxGenoShape& h) {
    const size_t tiles = (size_t)h.T * (h.SX + h.SZ);
    const size_t red = h.n_slice > 1 ? (size_t)VRX_GENO_R * VRX_GENO_R * VRX_GENO_BLOCK : 0;
    return tiles > red ? tiles : red;
}

// columns [c0, c0 + W) of nv rows of length L (P: the first row) into LDS rows of stride S
__device__ __forceinline__ void vrx_geno_load_tile(const double* __restrict__ P, int nv, int L, int c0, int W,
                                                   int S, double* tile) {
    if (((L | c0 | W) & 1) == 0) {  // pairs stay inside a row and start 16-byte aligned
        const unsigned half = (unsigned)W / 2, cnt = (unsigned)nv * half;
        for (unsigned e = threadIdx.x; e < cnt; e += VRX_GENO_BLOCK) {
            const unsigned v = e / half, j = 2 * (e - v * half);
            const double2 x = *reinterpret_cast<const double2*>(P + (size_t)v * L + c0 + j);
            tile[v * S + j] = x.x;
            tile[v * S + j + 1] = x.y;
        }
    } else {
        const unsigned cnt = (unsigned)nv * (unsigned)W;
        for (unsigned e = threadIdx.x; e < cnt; e += VRX_GENO_BLOCK) {
            const unsigned v = e / (unsigned)W, j = e - v * (unsigned)W;
            tile[v * S + j] = P[(size_t)v * L + c0 + j];
        }
    }
}

// the 16 terms of one (variant, t): x, z point at the lane's first donors, dx / dz doubles between donors
__device__ __forceinline__ void vrx_geno_terms(const double* x, const double* z, int dx, int dz,
                                               double (&acc)[VRX_GENO_R][VRX_GENO_R]) {
    double xv[VRX_GENO_R], zv[VRX_GENO_R];
#pragma unroll
    for (int a = 0; a < VRX_GENO_R; ++a) xv[a] = x[a * dx];
#pragma unroll
    for (int b = 0; b < VRX_GENO_R; ++b) zv[b] = z[b * dz];
#pragma unroll
    for (int a = 0; a < VRX_GENO_R; ++a)
#pragma unroll
        for (int b = 0; b < VRX_GENO_R; ++b) acc[a][b] += fabs(xv[a] - zv[b]);
}

// X, Z: a slab of nv variants; grid (n_chunk, output tiles, row-major over (tile_i, tile_j));
// part: [n_chunk][k1][k2] (GT = 3: unrolled; GT = 0: any n_GT)
template <int GT>
__global__ __launch_bounds__(VRX_GENO_BLOCK) void vrx_geno_pass(int nv, int k1, int k2, VrxGenoShape h,
                                                                const double* __restrict__ X,
                                                                const double* __restrict__ Z,
                                                                double* __restrict__ part) {
    extern __shared__ double lds[];
    constexpr int R = VRX_GENO_R;
    const int G = GT ? GT : h.G;
    const int tid = threadIdx.x;
    const int P = h.LI * h.LJ;
    const int lj = tid % h.LJ, li = (tid / h.LJ) % h.LI, s = tid / P;
    const int n_tj = (k2 + h.TJ - 1) / h.TJ;
    const int i0 = ((int)blockIdx.y / n_tj) * h.TI, j0 = ((int)blockIdx.y % n_tj) * h.TJ;
    const int ni = min(h.TI, k1 - i0), nj = min(h.TJ, k2 - j0);
    const int L1 = k1 * G, L2 = k2 * G;
    double* tx = lds;
    double* tz = lds + (size_t)h.T * h.SX;
    double acc[R][R];
#pragma unroll
    for (int a = 0; a < R; ++a)
#pragma unroll
        for (int b = 0; b < R; ++b) acc[a][b] = 0.0;
    const int n_vt = (nv + h.T - 1) / h.T;
    const int dx = h.LI * G, dz = h.LJ * G;  // between the donors of a lane
    for (int vt = blockIdx.x; vt < n_vt; vt += gridDim.x) {
        const int n0 = vt * h.T;
        const int cnt = min(h.T, nv - n0);
        vrx_geno_load_tile(X + (size_t)n0 * L1, cnt, L1, i0 * G, ni * G, h.SX, tx);
        vrx_geno_load_tile(Z + (size_t)n0 * L2, cnt, L2, j0 * G, nj * G, h.SZ, tz);
        __syncthreads();
        // (a lane position past the edge of D reads columns of its row that were not loaded: stale
        //  but inside the row, and its sums are never written)
        for (int v = s; v < cnt; v += h.n_slice) {
            const double* xr = tx + v * h.SX + li * G;
            const double* zr = tz + v * h.SZ + lj * G;
            if (GT) {
#pragma unroll
                for (int t = 0; t < GT; ++t) vrx_geno_terms(xr + t, zr + t, dx, dz, acc);
            } else {
                for (int t = 0; t < G; ++t) vrx_geno_terms(xr + t, zr + t, dx, dz, acc);
            }
        }
        __syncthreads();  // (the next load overwrites the tiles; after the last one: the slices' sums do)
    }
    double* out = part + (size_t)blockIdx.x * k1 * k2;
    if (h.n_slice == 1) {
#pragma unroll
        for (int a = 0; a < R; ++a)
#pragma unroll
            for (int b = 0; b < R; ++b) {
                const int i = i0 + li + h.LI * a, j = j0 + lj + h.LJ * b;
                if (i < k1 && j < k2) out[(size_t)i * k2 + j] = acc[a][b];
            }
        return;
    }
    double* red = lds;  // [R * R][256]: lane tid = s * P + (li * LJ + lj)
#pragma unroll
    for (int a = 0; a < R; ++a)
#pragma unroll
        for (int b = 0; b < R; ++b) red[(a * R + b) * VRX_GENO_BLOCK + tid] = acc[a][b];
    __syncthreads();
    for (int c = tid; c < R * R * P; c += VRX_GENO_BLOCK) {
        const int ab = c / P, p = c - ab * P;
        double sum = 0.0;
        for (int sl = 0; sl < h.n_slice; ++sl) sum += red[ab * VRX_GENO_BLOCK + sl * P + p];
        const int i = i0 + p / h.LJ + h.LI * (ab / R), j = j0 + p % h.LJ + h.LJ * (ab % R);
        if (i < k1 && j < k2) out[(size_t)i * k2 + j] = sum;
    }
}

// acc[c] = (first ? 0 : acc[c]) + the partials of cell c: a block takes 64 cells, its wave g the g-th of
// VRX_GENO_SUM_RUNS contiguous runs of chunks (in chunk order), then wave 0 adds the runs in order; with
// denom > 0 (the last slab) the mean: / denom.  Block of 64 * VRX_GENO_SUM_RUNS.
constexpr int VRX_GENO_SUM_RUNS = 16;
__global__ __launch_bounds__(64 * VRX_GENO_SUM_RUNS) void vrx_geno_sum(int n_chunk, int64_t n_cell,
                                                                       const double* __restrict__ part,
                                                                       double* __restrict__ acc, int first,
                                                                       double denom) {
    __shared__ double runs[VRX_GENO_SUM_RUNS][64];
    const int cl = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int64_t c = (int64_t)blockIdx.x * 64 + cl;
    const int len = (n_chunk + VRX_GENO_SUM_RUNS - 1) / VRX_GENO_SUM_RUNS;
    double sum = 0.0;  // (a run without chunks adds +0: nothing changes)
    if (c < n_cell)
        for (int k = g * len; k < min(n_chunk, (g + 1) * len); ++k) sum += part[(size_t)k * n_cell + c];
    runs[g][cl] = sum;
    __syncthreads();
    if (g != 0 || c >= n_cell) return;
    sum = first ? 0.0 : acc[c];
#pragma unroll
    for (int q = 0; q < VRX_GENO_SUM_RUNS; ++q) sum += runs[q][cl];
    acc[c] = denom > 0.0 ? sum / denom : sum;
}
