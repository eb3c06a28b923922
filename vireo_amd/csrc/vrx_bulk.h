// Bulk donor abundance (vrx_bulk_*): the device form of VireoBulk.fit and LikRatio_test
// (vireoSNP/utils/vireo_bulk.py:44-108, :120-167).  Included by vrx_bulk.hip only.
//
//   vrx_bulk_pass     one streaming pass over GT_prob [n][k][g] with the current (psi, theta): per
//                     workgroup the partial sums psi_raw[K] | theta_s1[G] | theta_s2[G] | logLik
//   vrx_bulk_finish   one block: the partials in workgroup order, then the trace entry, the stop
//                     rule and the M step (psi, theta)
//   vrx_bulk_ll       the pass restricted to the log-likelihood, for up to VRX_BULK_Q psi vectors
//   vrx_bulk_ll_sum   its partials in workgroup order
//
// The EM in factored form.  Per variant n with row P[k][g]:
//   tm_k = sum_g P[k][g] theta_g,  t1 = sum_k tm_k psi_k,  t0 = sum_k (1 - tm_k) psi_k,
//   w1 = AD_n / t1,  w0 = BD_n / t0,  q_k = tm_k psi_k,  q0_k = (1 - tm_k) psi_k
//   psi_raw_k  += w1 q_k + w0 q0_k                       (AD @ Z1 + BD @ Z0, :85)
//   theta_s1_g += w1 sum_k P[k][g] q_k,  theta_s2_g += w0 sum_k P[k][g] q0_k     (:89-90)
//   logLik     += AD_n log t1 + BD_n log(1 - t1)         (:94-96, of the parameters the pass READS)
// The log-likelihood the reference computes at the end of iteration `it` is that of the updated
// parameters, whose t1 is the normaliser of the next E step: pass p yields logLik[p - 1] and the
// sums of update p, so a fit of n iterations is n + 1 passes (when the stop rule fires, the update
// already summed is not applied).
//
// A workgroup walks tiles of T variants (T even: a tile starts 16-byte aligned).
//   load     the tile's T * K * G doubles, flat and coalesced (16-byte loads), into LDS rows of
//            stride K * G | 1 doubles (odd: the row-per-lane ds_read_b64 of phase 1 hit distinct
//            bank pairs)
//   phase 1  lane per variant: tm_k (kept in LDS), t1, t0, the log-likelihood term, w1, w0
//   phase 2  lane per (slice s, column j = (k, g)): the variants v = s (mod n_slice) of the tile,
//            n_slice = max(1, 256 / (K * G)); the three sums of its column in its own LDS slot
// and at the end reduces slices and donors in index order.  Every sum has a fixed order for a given
// grid, no atomics: two runs are bitwise identical.  All arithmetic is float64.
#pragma once

#include "vrx_common.h"
#include "vrx_stop.h"

constexpr int VRX_BULK_BLOCK = 256;
constexpr int VRX_BULK_Q = 8;           // psi vectors per log-likelihood pass
constexpr int VRX_BULK_BATCH = 8;       // passes the host enqueues between two reads of the control words
constexpr int VRX_BULK_LDS_TILE = 40 * 1024;  // what a workgroup's tile may take (4 workgroups per CU)
enum { VRX_BULK_STOP = 0, VRX_BULK_IT = 1, VRX_BULK_PASS = 2, VRX_BULK_CTL_WORDS = 4 };

struct VrxBulkShape {
    int K, G, L, S, SK, T, n_slice, n_acc;
};

// L = K * G columns; S, SK: the odd row strides of the tile and of tm; n_acc: accumulator slots
__host__ __device__ inline VrxBulkShape vrx_bulk_shape(int K, int G, int T) {
    VrxBulkShape h;
    h.K = K;
    h.G = G;
    h.L = K * G;
    h.S = h.L | 1;
    h.SK = K | 1;
    h.T = T;
    h.n_slice = h.L >= VRX_BULK_BLOCK ? 1 : VRX_BULK_BLOCK / h.L;
    h.n_acc = h.n_slice * h.L;
    return h;
}
// LDS of the fit pass (doubles): wave sums[4] | psi[K] | theta[G] | (pad to 16 bytes) | (w1, w0)[T] |
// (psi_raw, s1, s2)[n_acc] | tile[T][S] | tm[T][SK]
__host__ __device__ inline size_t vrx_bulk_lds_doubles(const VrxBulkShape& h) {
    return (size_t)h.K + h.G + 1 + (size_t)h.T * (h.S + h.SK + 2) + 3 * (size_t)h.n_acc + 4;
}
// LDS of the log-likelihood pass: psi[K][Q] | theta[G] | tile[T][S] | wave sums[4][Q]
__host__ __device__ inline size_t vrx_bulk_ll_lds_doubles(const VrxBulkShape& h) {
    return (size_t)VRX_BULK_Q * h.K + h.G + (size_t)h.T * h.S + 4 * VRX_BULK_Q;
}

__device__ __forceinline__ double vrx_bulk_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// variants [n0, n0 + nv) of P, flat, into rows of stride S
__device__ __forceinline__ void vrx_bulk_load_tile(const double* __restrict__ P, int n0, int nv, int L,
                                                   int S, double* tile) {
    const double* src = P + (int64_t)n0 * L;  // (n0 even: 16-byte aligned)
    const unsigned cnt = (unsigned)nv * (unsigned)L;
    const double2* src2 = reinterpret_cast<const double2*>(src);
    for (unsigned i = threadIdx.x; i < cnt / 2; i += VRX_BULK_BLOCK) {
        const double2 x = src2[i];
        const unsigned e = 2 * i, v = e / (unsigned)L, j = e - v * (unsigned)L;
        tile[v * S + j] = x.x;
        if (j + 1 < (unsigned)L)
            tile[v * S + j + 1] = x.y;
        else
            tile[(v + 1) * S] = x.y;
    }
    if ((cnt & 1u) && threadIdx.x == 0) {
        const unsigned e = cnt - 1, v = e / (unsigned)L, j = e - v * (unsigned)L;
        tile[v * S + j] = src[e];
    }
}

// tm of one donor from its LDS row (GT = 3: unrolled; GT = 0: any n_GT)
template <int GT>
__device__ __forceinline__ double vrx_bulk_tm(const double* row, const double* theta, int G) {
    double tm = 0.0;
    if (GT == 3) {
        tm = fma(row[0], theta[0], tm);
        tm = fma(row[1], theta[1], tm);
        tm = fma(row[2], theta[2], tm);
    } else {
        for (int g = 0; g < G; ++g) tm = fma(row[g], theta[g], tm);
    }
    return tm;
}

// par: psi[K] | theta[G] (device state); part: [gridDim.x][K + 2 G + 1]
template <int GT>
__global__ __launch_bounds__(VRX_BULK_BLOCK) void vrx_bulk_pass(
    int N, int K, int Grt, int T, const double* __restrict__ P, const double2* __restrict__ AB,
    const double* __restrict__ par, const int32_t* __restrict__ ctl, double* __restrict__ part) {
    if (ctl[VRX_BULK_STOP]) return;  // launched behind the stop: nothing to do
    extern __shared__ double lds[];
    const int G = GT ? GT : Grt;
    const VrxBulkShape h = vrx_bulk_shape(K, G, T);
    const int tid = threadIdx.x;
    double* wsum = lds;
    double* psi = wsum + 4;
    double* theta = psi + K;
    double2* ww = reinterpret_cast<double2*>(theta + G + ((K + G) & 1));  // (16-byte aligned)
    double* acc = reinterpret_cast<double*>(ww + T);
    double* tile = acc + 3 * h.n_acc;
    double* tmv = tile + (size_t)T * h.S;
    for (int i = tid; i < K + G; i += VRX_BULK_BLOCK) psi[i] = par[i];
    for (int i = tid; i < 3 * h.n_acc; i += VRX_BULK_BLOCK) acc[i] = 0.0;
    double ll = 0.0;
    const int n_tile = (N + T - 1) / T;
    for (int t = blockIdx.x; t < n_tile; t += gridDim.x) {
        const int n0 = t * T;
        const int nv = min(T, N - n0);
        double a = 0.0, b = 0.0;
        if (tid < nv) {  // (T <= 256: one variant per lane)
            const double2 ab = AB[n0 + tid];
            a = ab.x;
            b = ab.y;
        }
        vrx_bulk_load_tile(P, n0, nv, h.L, h.S, tile);
        __syncthreads();  // (also: psi, theta and the zeroed accumulators before the first tile)
        if (tid < nv) {
            const double* row = tile + (size_t)tid * h.S;
            double* tmr = tmv + (size_t)tid * h.SK;
            double t1 = 0.0, t0 = 0.0;
            for (int k = 0; k < K; ++k) {
                const double tm = vrx_bulk_tm<GT>(row + k * G, theta, G);
                tmr[k] = tm;
                t1 = fma(tm, psi[k], t1);
                t0 = fma(1.0 - tm, psi[k], t0);
            }
            ll += a * log(t1) + b * log(1.0 - t1);
            ww[tid] = make_double2(a / t1, b / t0);
        }
        __syncthreads();
        for (int c = tid; c < h.n_acc; c += VRX_BULK_BLOCK) {  // (one round unless K * G > 256)
            const int s = c / h.L, j = c - s * h.L, k = j / G;
            const double pk = psi[k];
            double sp = 0.0, s1 = 0.0, s2 = 0.0;
            for (int v = s; v < nv; v += h.n_slice) {
                const double p = tile[(size_t)v * h.S + j], tm = tmv[(size_t)v * h.SK + k];
                const double2 w = ww[v];
                const double x1 = w.x * (tm * pk), x0 = w.y * ((1.0 - tm) * pk);
                sp += x1 + x0;
                s1 = fma(x1, p, s1);
                s2 = fma(x0, p, s2);
            }
            acc[3 * c] += sp;
            acc[3 * c + 1] += s1;
            acc[3 * c + 2] += s2;
        }
        __syncthreads();  // (the next load overwrites the tile)
    }
    ll = vrx_bulk_wave_sum(ll);
    if ((tid & 63) == 0) wsum[tid >> 6] = ll;
    __syncthreads();  // (a workgroup without tiles arrives here too: zero sums)
    double* out = part + (size_t)blockIdx.x * (K + 2 * G + 1);
    for (int k = tid; k < K; k += VRX_BULK_BLOCK) {  // column (k, 0) carries psi_raw_k
        double s = 0.0;
        for (int sl = 0; sl < h.n_slice; ++sl) s += acc[3 * (sl * h.L + k * G)];
        out[k] = s;
    }
    for (int g = tid; g < 2 * G; g += VRX_BULK_BLOCK) {
        const int which = g < G ? 1 : 2, gg = g < G ? g : g - G;
        double s = 0.0;
        for (int sl = 0; sl < h.n_slice; ++sl)
            for (int k = 0; k < K; ++k) s += acc[3 * (sl * h.L + k * G + gg) + which];
        out[K + g] = s;
    }
    if (tid == 0) out[K + 2 * G] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// sums[w] = sum over workgroups of part[b * stride + w]: a wave per element, lane l takes b = l,
// l + 64, ... in order, then the butterfly.  Block of 1024.
__device__ __forceinline__ void vrx_bulk_reduce(int n_wg, int W, size_t stride, const double* __restrict__ part,
                                                double* sums) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, n_wave = blockDim.x >> 6;
    for (int w = wave; w < W; w += n_wave) {
        double s = 0.0;
        for (int b = lane; b < n_wg; b += 64) s += part[(size_t)b * stride + w];
        s = vrx_bulk_wave_sum(s);
        if (lane == 0) sums[w] = s;
    }
    __syncthreads();
}

// After pass p (ctl[VRX_BULK_PASS]): logLik[p - 1] and the stop rule of vireo_bulk.py:97-105 in its
// order of comparisons (a NaN makes each of them false: no stop before max_iter), else update p.
// One block, one sample: its partials part[b * stride + w], its parameters, trace and control words.
__device__ __forceinline__ void vrx_bulk_finish_one(int n_wg, int K, int G, size_t stride,
                                                    const double* __restrict__ part, double* __restrict__ par,
                                                    double* __restrict__ trace, int32_t* __restrict__ ctl,
                                                    int min_iter, int max_iter, double eps, int learn_theta,
                                                    int delay_fit_theta) {
    if (ctl[VRX_BULK_STOP]) return;
    extern __shared__ double lds[];
    const int W = K + 2 * G + 1;
    double* sums = lds;  // W, then one flag
    const int p = ctl[VRX_BULK_PASS];  // (read by every lane before the barrier in the reduction)
    vrx_bulk_reduce(n_wg, W, stride, part, sums);
    if (threadIdx.x == 0) {
        bool stop = false;
        if (p >= 1) {
            const int it = p - 1;
            const double ll = sums[W - 1];
            // (it == 0 reads logLik[-1] in the reference: the unwritten last entry, 0, or itself)
            const double prev = vrx_stop_prev(it, max_iter, it >= 1 ? trace[it - 1] : 0.0, ll);
            trace[it] = ll;
            stop = vrx_stop_judge(VRX_STOP_EM, it, min_iter, max_iter, eps, prev, ll) == VRX_STOP_STOP;
            if (it == max_iter - 1) stop = true;  // the loop ends: the update summed here is not applied
            if (stop) {
                ctl[VRX_BULK_IT] = it;
                ctl[VRX_BULK_STOP] = 1;
            }
        }
        sums[W] = stop ? 1.0 : 0.0;
        if (!stop) ctl[VRX_BULK_PASS] = p + 1;
    }
    __syncthreads();
    if (sums[W] != 0.0) return;
    double tot = 0.0;
    for (int k = 0; k < K; ++k) tot += sums[k];  // (every lane, index order)
    for (int k = threadIdx.x; k < K; k += blockDim.x) par[k] = sums[k] / tot;
    if (learn_theta && p >= delay_fit_theta)
        for (int g = threadIdx.x; g < G; g += blockDim.x) par[K + g] = sums[K + g] / (sums[K + g] + sums[K + G + g]);
}

__global__ __launch_bounds__(1024) void vrx_bulk_finish(int n_wg, int K, int G, const double* __restrict__ part,
                                                        double* __restrict__ par, double* __restrict__ trace,
                                                        int32_t* __restrict__ ctl, int min_iter, int max_iter,
                                                        double eps, int learn_theta, int delay_fit_theta) {
    vrx_bulk_finish_one(n_wg, K, G, (size_t)(K + 2 * G + 1), part, par, trace, ctl, min_iter, max_iter, eps,
                        learn_theta, delay_fit_theta);
}

// psis: nq x K (nq <= VRX_BULK_Q); part: [gridDim.x][nq]
template <int GT>
__global__ __launch_bounds__(VRX_BULK_BLOCK) void vrx_bulk_ll(
    int N, int K, int Grt, int T, int nq, const double* __restrict__ P, const double2* __restrict__ AB,
    const double* __restrict__ psis, const double* __restrict__ theta_in, double* __restrict__ part) {
    extern __shared__ double lds[];
    const int G = GT ? GT : Grt;
    const VrxBulkShape h = vrx_bulk_shape(K, G, T);
    const int tid = threadIdx.x;
    double* psi = lds;
    double* theta = psi + (size_t)VRX_BULK_Q * K;
    double* tile = theta + G;
    double* wsum = tile + (size_t)T * h.S;
    for (int i = tid; i < VRX_BULK_Q * K; i += VRX_BULK_BLOCK) {  // psi[k][q]: the q of a donor side by side
        const int k = i / VRX_BULK_Q, q = i - k * VRX_BULK_Q;
        psi[i] = q < nq ? psis[q * K + k] : 0.0;
    }
    for (int i = tid; i < G; i += VRX_BULK_BLOCK) theta[i] = theta_in[i];
    double ll[VRX_BULK_Q];
#pragma unroll
    for (int q = 0; q < VRX_BULK_Q; ++q) ll[q] = 0.0;
    const int n_tile = (N + T - 1) / T;
    for (int t = blockIdx.x; t < n_tile; t += gridDim.x) {
        const int n0 = t * T;
        const int nv = min(T, N - n0);
        double a = 0.0, b = 0.0;
        if (tid < nv) {
            const double2 ab = AB[n0 + tid];
            a = ab.x;
            b = ab.y;
        }
        vrx_bulk_load_tile(P, n0, nv, h.L, h.S, tile);
        __syncthreads();
        if (tid < nv) {
            const double* row = tile + (size_t)tid * h.S;
            double t1[VRX_BULK_Q];
#pragma unroll
            for (int q = 0; q < VRX_BULK_Q; ++q) t1[q] = 0.0;
            for (int k = 0; k < K; ++k) {
                const double tm = vrx_bulk_tm<GT>(row + k * G, theta, G);
#pragma unroll
                for (int q = 0; q < VRX_BULK_Q; ++q) t1[q] = fma(tm, psi[k * VRX_BULK_Q + q], t1[q]);
            }
#pragma unroll
            for (int q = 0; q < VRX_BULK_Q; ++q)
                if (q < nq) ll[q] += a * log(t1[q]) + b * log(1.0 - t1[q]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < VRX_BULK_Q; ++q) {
        const double s = vrx_bulk_wave_sum(ll[q]);
        if ((tid & 63) == 0) wsum[(tid >> 6) * VRX_BULK_Q + q] = s;
    }
    __syncthreads();
    if (tid < nq)
        part[(size_t)blockIdx.x * nq + tid] = ((wsum[tid] + wsum[VRX_BULK_Q + tid]) + wsum[2 * VRX_BULK_Q + tid]) +
                                              wsum[3 * VRX_BULK_Q + tid];
}

__global__ __launch_bounds__(1024) void vrx_bulk_ll_sum(int n_wg, int nq, const double* __restrict__ part,
                                                        double* __restrict__ out) {
    __shared__ double sums[VRX_BULK_Q];
    vrx_bulk_reduce(n_wg, nq, (size_t)nq, part, sums);
    if ((int)threadIdx.x < nq) out[threadIdx.x] = sums[threadIdx.x];
}

// ---- cohort: S samples on one GT_prob -------------------------------------------------------------
//   vrx_bulk_cohort_pass     the fit pass for a chunk of VRX_BULK_COHORT samples: a tile of GT_prob is
//                            loaded into LDS once, then every live sample of the chunk runs phase 1 and
//                            phase 2 off it, one after another over one tm / (w1, w0) buffer, with its own
//                            psi, theta, counts, accumulators and wave sums
//   vrx_bulk_cohort_finish   a block per sample: vrx_bulk_finish_one on that sample's partials and state
//   vrx_bulk_cohort_ll       the log-likelihood pass for a chunk; vrx_bulk_cohort_ll_sum its partials
// blockIdx.y is the chunk, blockIdx.x the workgroup that walks tiles grid-stride.  Tile size and grid are
// functions of (n_var, n_donor, n_GT) alone and a short chunk is padded with dead samples, so what a
// sample sums, and in which order, does not depend on the rest of the cohort nor on its slot in a chunk:
// its results are bitwise independent of both.  (The loops over a chunk's slots are not unrolled, so every
// slot runs the same instructions; contraction is off in these kernels and every fused multiply-add is
// written out, so a slot's rounding cannot depend on how the compiler arranged its neighbours.)
// Counts are sample-major, AB[s][n]; state is par[s][K + G], ctl[s][VRX_BULK_CTL_WORDS], trace[s][max_iter];
// partials are part[chunk][workgroup][slot][K + 2 G + 1] (fit) or [..][slot][nq] (log-likelihood).
constexpr int VRX_BULK_COHORT = 4;                 // samples per chunk (what bounds it)
constexpr int VRX_BULK_COHORT_LDS = 64 * 1024;     // what a cohort workgroup may take (2 workgroups per CU)

// per sample of a chunk (doubles): wave sums[4] | psi[K] | theta[G] | (psi_raw, s1, s2)[n_acc]
__host__ __device__ inline size_t vrx_bulk_cohort_slot_doubles(const VrxBulkShape& h) {
    return 4 + (size_t)h.K + h.G + 3 * (size_t)h.n_acc;
}
// LDS of the cohort fit pass: slots[VRX_BULK_COHORT] | (pad to 16 bytes) | (w1, w0)[T] | tile[T][S] | tm[T][SK]
__host__ __device__ inline size_t vrx_bulk_cohort_lds_doubles(const VrxBulkShape& h) {
    return VRX_BULK_COHORT * vrx_bulk_cohort_slot_doubles(h) + 1 + (size_t)h.T * (h.S + h.SK + 2);
}
// per sample of a chunk in the log-likelihood pass: psi[K][Q] | theta[G] | wave sums[4][Q]
__host__ __device__ inline size_t vrx_bulk_cohort_ll_slot_doubles(const VrxBulkShape& h) {
    return (size_t)VRX_BULK_Q * h.K + h.G + 4 * VRX_BULK_Q;
}
__host__ __device__ inline size_t vrx_bulk_cohort_ll_lds_doubles(const VrxBulkShape& h) {
    return VRX_BULK_COHORT * vrx_bulk_cohort_ll_slot_doubles(h) + (size_t)h.T * h.S;
}

template <int GT>
__global__ __launch_bounds__(VRX_BULK_BLOCK) void vrx_bulk_cohort_pass(
    int N, int K, int Grt, int T, int n_sample, const double* __restrict__ P, const double2* __restrict__ AB,
    const double* __restrict__ par, const int32_t* __restrict__ ctl, double* __restrict__ part) {
#pragma clang fp contract(off)
    const int s0 = blockIdx.y * VRX_BULK_COHORT;
    unsigned live = 0;  // (uniform: every lane reads the same words)
#pragma unroll
    for (int c = 0; c < VRX_BULK_COHORT; ++c)
        if (s0 + c < n_sample && !ctl[(size_t)(s0 + c) * VRX_BULK_CTL_WORDS + VRX_BULK_STOP]) live |= 1u << c;
    if (!live) return;  // every sample of the chunk has stopped (or is padding)
    extern __shared__ double lds[];
    const int G = GT ? GT : Grt;
    const VrxBulkShape h = vrx_bulk_shape(K, G, T);
    const int tid = threadIdx.x;
    const size_t slot = vrx_bulk_cohort_slot_doubles(h);
    const size_t head = VRX_BULK_COHORT * slot;
    double2* ww = reinterpret_cast<double2*>(lds + head + (head & 1));  // (16-byte aligned)
    double* tile = reinterpret_cast<double*>(ww + T);
    double* tmv = tile + (size_t)T * h.S;
    // The loops over the slots of the chunk are NOT unrolled: every slot runs the same instructions.
#pragma unroll 1
    for (int c = 0; c < VRX_BULK_COHORT; ++c) {
        if (!(live >> c & 1)) continue;
        double* psi = lds + c * slot + 4;
        const double* src = par + (size_t)(s0 + c) * (K + G);
        for (int i = tid; i < K + G; i += VRX_BULK_BLOCK) psi[i] = src[i];
        double* acc = psi + K + G;
        for (int i = tid; i < 3 * h.n_acc; i += VRX_BULK_BLOCK) acc[i] = 0.0;
    }
    double ll[VRX_BULK_COHORT];  // (indexed by constants only: registers)
#pragma unroll
    for (int j = 0; j < VRX_BULK_COHORT; ++j) ll[j] = 0.0;
    const int n_tile = (N + T - 1) / T;
    for (int t = blockIdx.x; t < n_tile; t += gridDim.x) {
        const int n0 = t * T;
        const int nv = min(T, N - n0);
        vrx_bulk_load_tile(P, n0, nv, h.L, h.S, tile);
        __syncthreads();  // (also: the slots before the first tile)
#pragma unroll 1
        for (int c = 0; c < VRX_BULK_COHORT; ++c) {
            if (!(live >> c & 1)) continue;
            const double* psi = lds + c * slot + 4;
            const double* theta = psi + K;
            double* acc = lds + c * slot + 4 + K + G;
            if (tid < nv) {
                const double2 ab = AB[(size_t)(s0 + c) * N + n0 + tid];  // (in flight under the donor loop)
                const double* row = tile + (size_t)tid * h.S;
                double* tmr = tmv + (size_t)tid * h.SK;
                double t1 = 0.0, t0 = 0.0;
                for (int k = 0; k < K; ++k) {
                    const double tm = vrx_bulk_tm<GT>(row + k * G, theta, G);
                    tmr[k] = tm;
                    t1 = fma(tm, psi[k], t1);
                    t0 = fma(1.0 - tm, psi[k], t0);
                }
                const double la = ab.x * log(t1), lb = ab.y * log(1.0 - t1);
#pragma unroll
                for (int j = 0; j < VRX_BULK_COHORT; ++j)
                    if (j == c) ll[j] += la + lb;
                ww[tid] = make_double2(ab.x / t1, ab.y / t0);
            }
            __syncthreads();
            for (int cc = tid; cc < h.n_acc; cc += VRX_BULK_BLOCK) {  // (one round unless K * G > 256)
                const int s = cc / h.L, j = cc - s * h.L, k = j / G;
                const double pk = psi[k];
                double sp = 0.0, s1 = 0.0, s2 = 0.0;
                for (int v = s; v < nv; v += h.n_slice) {
                    const double p = tile[(size_t)v * h.S + j], tm = tmv[(size_t)v * h.SK + k];
                    const double2 w = ww[v];
                    const double x1 = w.x * (tm * pk), x0 = w.y * ((1.0 - tm) * pk);
                    sp += x1 + x0;
                    s1 = fma(x1, p, s1);
                    s2 = fma(x0, p, s2);
                }
                acc[3 * cc] += sp;
                acc[3 * cc + 1] += s1;
                acc[3 * cc + 2] += s2;
            }
            __syncthreads();  // (the next sample overwrites tm and (w1, w0), the next load the tile)
        }
    }
#pragma unroll 1
    for (int c = 0; c < VRX_BULK_COHORT; ++c) {
        if (!(live >> c & 1)) continue;
        double v = 0.0;
#pragma unroll
        for (int j = 0; j < VRX_BULK_COHORT; ++j)
            if (j == c) v = ll[j];
        v = vrx_bulk_wave_sum(v);
        if ((tid & 63) == 0) lds[c * slot + (tid >> 6)] = v;
    }
    __syncthreads();  // (a workgroup without tiles arrives here too: zero sums)
    const int W = K + 2 * G + 1;
#pragma unroll 1
    for (int c = 0; c < VRX_BULK_COHORT; ++c) {
        if (!(live >> c & 1)) continue;
        const double* wsum = lds + c * slot;
        const double* acc = wsum + 4 + K + G;
        double* out = part + (((size_t)blockIdx.y * gridDim.x + blockIdx.x) * VRX_BULK_COHORT + c) * W;
        for (int k = tid; k < K; k += VRX_BULK_BLOCK) {  // column (k, 0) carries psi_raw_k
            double s = 0.0;
            for (int sl = 0; sl < h.n_slice; ++sl) s += acc[3 * (sl * h.L + k * G)];
            out[k] = s;
        }
        for (int g = tid; g < 2 * G; g += VRX_BULK_BLOCK) {
            const int which = g < G ? 1 : 2, gg = g < G ? g : g - G;
            double s = 0.0;
            for (int sl = 0; sl < h.n_slice; ++sl)
                for (int k = 0; k < K; ++k) s += acc[3 * (sl * h.L + k * G + gg) + which];
            out[K + g] = s;
        }
        if (tid == 0) out[K + 2 * G] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
    }
}

// grid: one block per sample.  A sample that has stopped is frozen: vrx_bulk_finish_one returns before
// it touches that sample's psi, theta or trace.
__global__ __launch_bounds__(1024) void vrx_bulk_cohort_finish(int n_wg, int K, int G, const double* __restrict__ part,
                                                               double* __restrict__ par, double* __restrict__ trace,
                                                               int32_t* __restrict__ ctl, int min_iter, int max_iter,
                                                               double eps, int learn_theta, int delay_fit_theta) {
    const int s = blockIdx.x, chunk = s / VRX_BULK_COHORT, c = s - chunk * VRX_BULK_COHORT;
    const size_t W = (size_t)(K + 2 * G + 1);
    vrx_bulk_finish_one(n_wg, K, G, VRX_BULK_COHORT * W, part + ((size_t)chunk * n_wg * VRX_BULK_COHORT + c) * W,
                        par + (size_t)s * (K + G), trace + (size_t)s * max_iter,
                        ctl + (size_t)s * VRX_BULK_CTL_WORDS, min_iter, max_iter, eps, learn_theta, delay_fit_theta);
}

// psis: [n_sample][n_psi][K], of which this pass takes q0 .. q0 + nq (nq <= VRX_BULK_Q); thetas: [n_sample][G];
// part: [chunk][gridDim.x][slot][nq]
template <int GT>
__global__ __launch_bounds__(VRX_BULK_BLOCK) void vrx_bulk_cohort_ll(
    int N, int K, int Grt, int T, int n_sample, int n_psi, int q0, int nq, const double* __restrict__ P,
    const double2* __restrict__ AB, const double* __restrict__ psis, const double* __restrict__ thetas,
    double* __restrict__ part) {
#pragma clang fp contract(off)
    extern __shared__ double lds[];
    const int G = GT ? GT : Grt;
    const VrxBulkShape h = vrx_bulk_shape(K, G, T);
    const int tid = threadIdx.x;
    const int s0 = blockIdx.y * VRX_BULK_COHORT;
    const int n_slot = min(VRX_BULK_COHORT, n_sample - s0);  // (the rest of a short chunk is padding)
    const size_t slot = vrx_bulk_cohort_ll_slot_doubles(h);
    double* tile = lds + VRX_BULK_COHORT * slot;
#pragma unroll 1
    for (int c = 0; c < n_slot; ++c) {
        double* psi = lds + c * slot;
        const double* src = psis + ((size_t)(s0 + c) * n_psi + q0) * K;
        for (int i = tid; i < VRX_BULK_Q * K; i += VRX_BULK_BLOCK) {  // psi[k][q]: the q of a donor side by side
            const int k = i / VRX_BULK_Q, q = i - k * VRX_BULK_Q;
            psi[i] = q < nq ? src[(size_t)q * K + k] : 0.0;
        }
        for (int i = tid; i < G; i += VRX_BULK_BLOCK) psi[VRX_BULK_Q * K + i] = thetas[(size_t)(s0 + c) * G + i];
    }
    double ll[VRX_BULK_COHORT][VRX_BULK_Q];  // (indexed by constants only: registers)
#pragma unroll
    for (int j = 0; j < VRX_BULK_COHORT; ++j)
#pragma unroll
        for (int q = 0; q < VRX_BULK_Q; ++q) ll[j][q] = 0.0;
    const int n_tile = (N + T - 1) / T;
    for (int t = blockIdx.x; t < n_tile; t += gridDim.x) {
        const int n0 = t * T;
        const int nv = min(T, N - n0);
        vrx_bulk_load_tile(P, n0, nv, h.L, h.S, tile);
        __syncthreads();  // (also: psi and theta of every slot before the first tile)
        if (tid < nv) {
            const double* row = tile + (size_t)tid * h.S;
#pragma unroll 1
            for (int c = 0; c < n_slot; ++c) {  // (not unrolled: every slot runs the same instructions)
                const double2 ab = AB[(size_t)(s0 + c) * N + n0 + tid];
                const double* psi = lds + c * slot;
                const double* theta = psi + VRX_BULK_Q * K;
                double t1[VRX_BULK_Q];
#pragma unroll
                for (int q = 0; q < VRX_BULK_Q; ++q) t1[q] = 0.0;
                for (int k = 0; k < K; ++k) {
                    const double tm = vrx_bulk_tm<GT>(row + k * G, theta, G);
#pragma unroll
                    for (int q = 0; q < VRX_BULK_Q; ++q) t1[q] = fma(tm, psi[k * VRX_BULK_Q + q], t1[q]);
                }
#pragma unroll
                for (int q = 0; q < VRX_BULK_Q; ++q) {
                    if (q >= nq) continue;
                    const double la = ab.x * log(t1[q]), lb = ab.y * log(1.0 - t1[q]);
#pragma unroll
                    for (int j = 0; j < VRX_BULK_COHORT; ++j)
                        if (j == c) ll[j][q] += la + lb;
                }
            }
        }
        __syncthreads();  // (the next load overwrites the tile)
    }
#pragma unroll 1
    for (int c = 0; c < n_slot; ++c) {
        double* wsum = lds + c * slot + VRX_BULK_Q * K + G;
#pragma unroll
        for (int q = 0; q < VRX_BULK_Q; ++q) {
            double v = 0.0;
#pragma unroll
            for (int j = 0; j < VRX_BULK_COHORT; ++j)
                if (j == c) v = ll[j][q];
            v = vrx_bulk_wave_sum(v);
            if ((tid & 63) == 0) wsum[(tid >> 6) * VRX_BULK_Q + q] = v;
        }
    }
    __syncthreads();
    for (int i = tid; i < n_slot * nq; i += VRX_BULK_BLOCK) {
        const int c = i / nq, q = i - c * nq;
        const double* wsum = lds + c * slot + VRX_BULK_Q * K + G;
        part[(((size_t)blockIdx.y * gridDim.x + blockIdx.x) * VRX_BULK_COHORT + c) * nq + q] =
            ((wsum[q] + wsum[VRX_BULK_Q + q]) + wsum[2 * VRX_BULK_Q + q]) + wsum[3 * VRX_BULK_Q + q];
    }
}

// grid: one block per sample; out: [n_sample][n_psi]
__global__ __launch_bounds__(1024) void vrx_bulk_cohort_ll_sum(int n_wg, int n_psi, int q0, int nq,
                                                               const double* __restrict__ part,
                                                               double* __restrict__ out) {
    __shared__ double sums[VRX_BULK_Q];
    const int s = blockIdx.x, chunk = s / VRX_BULK_COHORT, c = s - chunk * VRX_BULK_COHORT;
    vrx_bulk_reduce(n_wg, nq, (size_t)VRX_BULK_COHORT * nq, part + ((size_t)chunk * n_wg * VRX_BULK_COHORT + c) * nq,
                    sums);
    if ((int)threadIdx.x < nq) out[(size_t)s * n_psi + q0 + threadIdx.x] = sums[threadIdx.x];
}
