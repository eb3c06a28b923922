// Ambient-RNA estimation (vrx_problem_elbo_gain, vrx_problem_ambient): the device form of
// predit_ambient (vireoSNP/utils/vireo_doublet.py:213-273) and the per-cell EM it runs,
// _fit_EM_ambient (:139-210), plus the variant selection of variant_ELBO_gain
// (vireoSNP/utils/variant_select.py:66-106).  Included by vrx_engine.hip only.
//
//   vrx_amb_gain     thread per variant: the digamma / logsumexp of variant_ELBO_gain on the
//                    sums AD@ID, DP@ID of one variant pass (the last ID column is all ones: it
//                    carries the row sums of the one-donor model M1)
//   vrx_amb_count    wave per cell: the cell's selected entries with dp > 0 (zero counts add
//                    nothing to any term of the EM)
//   vrx_amb_scatter  wave per cell: those entries, in variant order, as (selected row, a, b)
//   vrx_amb_em       wave per cell: the whole EM of one cell, then its Fisher variance and
//                    likelihood ratio
//
// The EM in factored form: with t1 = theta_e . psi and t0 = (1 - theta_e) . psi per entry e,
//   psi_k <- psi_k r_k / sum_j psi_j r_j,   r_k = sum_e a_e theta_ek / t1_e + b_e (1 - theta_ek) / t0_e
// which is the reference's E step (Z1, Z0 normalised per variant) and M step (AD @ Z1 + BD @ Z0)
// restricted to the entries whose counts are not zero.  The log-likelihood of psi_{p} and the
// r of the update from psi_{p} need the same t1, so one pass over the entries serves both: pass p
// yields logLik[p - 1] and, unless the stop rule ends the loop there, psi_{p + 1}.
//
// Inside a pass the lanes take 64 entries at a time (t1, t0, the log-likelihood terms and the two
// per-entry weights a/t1, b/t0), put the weights in LDS, and then lane k walks those 64 entries in
// order for r_k.  Every sum has a fixed order (lane-sequential chunks, a butterfly over the wave,
// entry order for r), so two runs are bitwise identical; no atomics.  A cell whose entries fit the
// LDS budget keeps their theta rows in LDS (row stride K | 1 doubles: the lane-per-entry reads of
// ds_read_b64 hit 32 distinct bank pairs per half-wave); longer cells read them from the selected
// theta table in global memory (<= n_sel x K doubles, L2 / Infinity Cache resident).
#pragma once

#include "vrx_common.h"
#include "vrx_kernels.h"
#include "vrx_stop.h"

constexpr int VRX_AMB_CELLS = 4;  // cells (waves) per block of the compaction kernels

__device__ __forceinline__ double vrx_amb_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);  // (a + b == b + a: every lane ends equal)
    return v;
}

// S[n][k] = (AD@ID, DP@ID) for k < K1 (variant pass with K1 columns, the last one all ones)
__global__ __launch_bounds__(VRX_BLOCK) void vrx_amb_gain(int64_t n_var, int K1, double pc,
                                                          const double* __restrict__ S,
                                                          double* __restrict__ gain) {
    const int64_t n = (int64_t)blockIdx.x * VRX_BLOCK + threadIdx.x;
    if (n >= n_var) return;
    const double* s = S + n * K1 * 2;
    auto term = [&](double ad, double dp) {
        const double s1 = ad + pc, s2 = (dp - ad) + pc, ss = dp + 2.0 * pc;
        return s1 * vrx_digamma(s1) + s2 * vrx_digamma(s2) - ss * vrx_digamma(ss);
    };
    const int K = K1 - 1;
    double mx = -INFINITY;
    for (int k = 0; k < K; ++k) mx = fmax(mx, term(s[2 * k], s[2 * k + 1]));
    double sum = 0.0;
    for (int k = 0; k < K; ++k) sum += exp(term(s[2 * k], s[2 * k + 1]) - mx);
    // logsumexp over one value is that value: the M1 model's ELBO
    gain[n] = (log(sum) + mx) - term(s[2 * K], s[2 * K + 1]);
}

template <int FMT>
__device__ __forceinline__ bool vrx_amb_entry(const uint32_t* __restrict__ ent, int64_t e,
                                              const int32_t* __restrict__ rank, int32_t& row, int& a,
                                              int& b) {
    const VrxWords<FMT> w = vrx_load_words<FMT>(ent, e, true);
    uint32_t id;
    int ad, dp;
    vrx_unpack<FMT>(w, id, ad, dp);
    row = rank[id];
    a = ad;
    b = dp - ad;
    return row >= 0 && dp > 0;
}

template <int FMT>
__global__ __launch_bounds__(64 * VRX_AMB_CELLS) void vrx_amb_count(
    int64_t n_cell, const int64_t* __restrict__ cptr, const uint32_t* __restrict__ ent,
    const int32_t* __restrict__ rank, int64_t* __restrict__ cnt) {
    const int64_t c = (int64_t)blockIdx.x * VRX_AMB_CELLS + threadIdx.x / 64;
    const int lane = threadIdx.x & 63;
    if (c >= n_cell) return;  // (whole waves)
    const int64_t end = cptr[c + 1];
    int64_t n = 0;
    for (int64_t base = cptr[c]; base < end; base += 64) {
        int32_t row = -1;
        int a = 0, b = 0;
        const bool keep = base + lane < end && vrx_amb_entry<FMT>(ent, base + lane, rank, row, a, b);
        n += __popcll(__ballot(keep));
    }
    if (lane == 0) cnt[c] = n;
}

template <int FMT>
__global__ __launch_bounds__(64 * VRX_AMB_CELLS) void vrx_amb_scatter(
    int64_t n_cell, const int64_t* __restrict__ cptr, const uint32_t* __restrict__ ent,
    const int32_t* __restrict__ rank, const int64_t* __restrict__ sptr, int32_t* __restrict__ ev,
    int32_t* __restrict__ ea, int32_t* __restrict__ eb) {
    const int64_t c = (int64_t)blockIdx.x * VRX_AMB_CELLS + threadIdx.x / 64;
    const int lane = threadIdx.x & 63;
    if (c >= n_cell) return;
    const int64_t end = cptr[c + 1];
    int64_t out = sptr[c];
    for (int64_t base = cptr[c]; base < end; base += 64) {
        int32_t row = -1;
        int a = 0, b = 0;
        const bool keep = base + lane < end && vrx_amb_entry<FMT>(ent, base + lane, rank, row, a, b);
        const uint64_t mask = __ballot(keep);
        const int before = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32),
                                                     __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
        if (keep) {
            ev[out + before] = row;
            ea[out + before] = a;
            eb[out + before] = b;
        }
        out += __popcll(mask);
    }
}

// LDS of one cell (doubles): psi[K] | r[K] | w1[64] | w0[64] | theta cache [cap][K | 1], then the
// chunk's 64 theta row numbers (int32)
__host__ __device__ inline size_t vrx_amb_lds_bytes(int K, int cap) {
    return ((size_t)2 * K + 128 + (size_t)cap * (K | 1)) * sizeof(double) + 64 * sizeof(int32_t);
}

// one pass over the cell's entries with psi as it is in LDS:
//   MODE 0  r_k (LDS) = sum_e theta_ek w1_e + (1 - theta_ek) w0_e, w1 = a / t1, w0 = b / t0;
//           returns sum_e a log t1 + b log(1 - t1)
//   MODE 1  r_k (LDS) = sum_e theta_ek^2 (a / t1^2 + b / (1 - t1)^2)  (Fisher information);
//           returns sum_e a log theta_e,kmax + b log(1 - theta_e,kmax)  (the one-donor null)
template <bool CACHED, int MODE>
__device__ __forceinline__ double vrx_amb_pass(int K, int n, const int32_t* __restrict__ ev,
                                               const int32_t* __restrict__ ea,
                                               const int32_t* __restrict__ eb,
                                               const double* __restrict__ theta, double* psi, double* r,
                                               double* w1, double* w0, const double* th, int32_t* rows,
                                               int kmax) {
    const int lane = threadIdx.x;
    const int S = K | 1;
    for (int k = lane; k < K; k += 64) r[k] = 0.0;
    double ll = 0.0;
    for (int base = 0; base < n; base += 64) {
        const int e = base + lane;
        double x1 = 0.0, x0 = 0.0;
        if (e < n) {
            const int32_t row = ev[e];
            const double* t = CACHED ? th + (size_t)e * S : theta + (size_t)row * K;
            const double a = (double)ea[e], b = (double)eb[e];
            double t1 = 0.0, t0 = 0.0;
            for (int k = 0; k < K; ++k) {
                const double tk = t[k], pk = psi[k];
                t1 = fma(tk, pk, t1);
                t0 = fma(1.0 - tk, pk, t0);
            }
            if (MODE == 0) {
                ll += a * log(t1) + b * log(1.0 - t1);
                x1 = a / t1;
                x0 = b / t0;
            } else {
                const double tm = t[kmax];
                ll += a * log(tm) + b * log(1.0 - tm);
                x1 = a / (t1 * t1) + b / ((1.0 - t1) * (1.0 - t1));
            }
            rows[lane] = row;
        }
        w1[lane] = x1;
        w0[lane] = x0;
        __syncthreads();
        const int m = min(64, n - base);
        for (int k = lane; k < K; k += 64) {
            double acc = r[k];
            for (int j = 0; j < m; ++j) {
                const double tk = CACHED ? th[(size_t)(base + j) * S + k] : theta[(size_t)rows[j] * K + k];
                if (MODE == 0) {
                    acc = fma(tk, w1[j], acc);
                    acc = fma(1.0 - tk, w0[j], acc);
                } else {
                    acc = fma(tk * tk, w1[j], acc);
                }
            }
            r[k] = acc;
        }
        __syncthreads();
    }
    return vrx_amb_wave_sum(ll);
}

template <bool CACHED>
__device__ __forceinline__ void vrx_amb_cell(int K, int n, const int32_t* __restrict__ ev,
                                             const int32_t* __restrict__ ea, const int32_t* __restrict__ eb,
                                             const double* __restrict__ theta, double* psi, double* r,
                                             double* w1, double* w0, const double* th, int32_t* rows,
                                             int min_iter, int max_iter, double eps, double* ll_ret,
                                             int* it_ret) {
    const int lane = threadIdx.x;
    double ll_prev = 0.0;
    for (int p = 0;; ++p) {
        const double ll = vrx_amb_pass<CACHED, 0>(K, n, ev, ea, eb, theta, psi, r, w1, w0, th, rows, 0);
        if (p >= 1) {  // ll = logLik[it] of the reference, it = p - 1 (vireo_doublet.py:170-178)
            const int it = p - 1;
            bool stop = it == max_iter - 1;
            // (it == 0: ll_prev is not the reference's logLik[-1] -- vrx_stop_prev is; min_iter >= 0 never judges it)
            if (vrx_stop_judge(VRX_STOP_EM, it, min_iter, max_iter, eps, vrx_stop_prev(it, max_iter, ll_prev, ll), ll) ==
                VRX_STOP_STOP)
                stop = true;
            if (stop) {  // psi_p is final; the reference returns logLik[it - 1] (logLik_RV = logLik[:it])
                *ll_ret = ll_prev;
                *it_ret = it;
                return;
            }
        }
        ll_prev = ll;
        // M step: psi <- psi * r / sum(psi * r), the sum in index order on every lane
        double sum = 0.0;
        for (int k = 0; k < K; ++k) sum += psi[k] * r[k];
        __syncthreads();
        for (int k = lane; k < K; k += 64) psi[k] = psi[k] * r[k] / sum;
        __syncthreads();
    }
}

// one wave (block of 64) per cell; `cap`: the most entries whose theta rows the LDS holds
__global__ __launch_bounds__(64) void vrx_amb_em(
    int K, const int64_t* __restrict__ sptr, const int32_t* __restrict__ ev_all,
    const int32_t* __restrict__ ea_all, const int32_t* __restrict__ eb_all,
    const double* __restrict__ theta, const double* __restrict__ psi0, int min_iter, int max_iter,
    double eps, int cap, double* __restrict__ psi_out, double* __restrict__ var_out,
    double* __restrict__ llr_out, int32_t* __restrict__ it_out) {
    extern __shared__ double lds[];
    const int lane = threadIdx.x;
    const int64_t c = blockIdx.x;
    double* psi = lds;
    double* r = psi + K;
    double* w1 = r + K;
    double* w0 = w1 + 64;
    double* th = w0 + 64;
    int32_t* rows = reinterpret_cast<int32_t*>(th + (size_t)cap * (K | 1));
    const int64_t beg = sptr[c];
    const int n = (int)(sptr[c + 1] - beg);
    const int32_t* ev = ev_all + beg;
    const int32_t* ea = ea_all + beg;
    const int32_t* eb = eb_all + beg;
    double tot = 0.0;
    for (int e = lane; e < n; e += 64) tot += (double)ea[e] + (double)eb[e];
    tot = vrx_amb_wave_sum(tot);
    if (!(tot > 0.0)) {  // no selected counts: 0 / 0 in the reference, NaN throughout, no break
        for (int k = lane; k < K; k += 64) {
            psi_out[c * K + k] = __builtin_nan("");
            var_out[c * K + k] = __builtin_nan("");
        }
        if (lane == 0) {
            llr_out[c] = __builtin_nan("");
            it_out[c] = max_iter - 1;
        }
        return;
    }
    for (int k = lane; k < K; k += 64) psi[k] = psi0[c * K + k];
    const bool cached = n <= cap;
    if (cached) {
        const int S = K | 1;
        for (int i = lane; i < n * K; i += 64) {
            const int e = i / K, k = i - e * K;
            th[(size_t)e * S + k] = theta[(size_t)ev[e] * K + k];
        }
    }
    __syncthreads();
    double ll_ret = 0.0;
    int it = 0;
    if (cached)
        vrx_amb_cell<true>(K, n, ev, ea, eb, theta, psi, r, w1, w0, th, rows, min_iter, max_iter, eps, &ll_ret, &it);
    else
        vrx_amb_cell<false>(K, n, ev, ea, eb, theta, psi, r, w1, w0, th, rows, min_iter, max_iter, eps, &ll_ret, &it);
    // the first maximum of psi (np.argmax), then the variance bound and the null model
    int kmax = 0;
    for (int k = 1; k < K; ++k)
        if (psi[k] > psi[kmax]) kmax = k;
    const double ll0 = cached
        ? vrx_amb_pass<true, 1>(K, n, ev, ea, eb, theta, psi, r, w1, w0, th, rows, kmax)
        : vrx_amb_pass<false, 1>(K, n, ev, ea, eb, theta, psi, r, w1, w0, th, rows, kmax);
    for (int k = lane; k < K; k += 64) {
        psi_out[c * K + k] = psi[k];
        var_out[c * K + k] = 1.0 / r[k];
    }
    if (lane == 0) {
        llr_out[c] = ll_ret - ll0;
        it_out[c] = it;
    }
}
