// Bulk donor abundance: the vrx_bulk_* entries of include/vireo_hip.h on the kernels of vrx_bulk.h.
// A handle owns its stream, events and buffers; nothing here touches a vrx_problem or a vrx_model.
#include <algorithm>

#include "vrx_handle.h"
#include "vrx_bulk.h"

struct vrx_bulk : VrxQueue {  // ev: 0, 1 bracket the passes of a fit
    int n_cu = 0;
    int64_t N = 0;
    int K = 0, G = 0;
    int T = 0, n_wg = 0;       // the fit pass: variants per tile, workgroups
    int T_ll = 0, n_wg_ll = 0; // the log-likelihood pass
    size_t lds = 0, lds_ll = 0;
    DevBuf<double> P;
    DevBuf<double2> AB;  // (AD, BD) per variant
    DevBuf<double> par;     // psi[K] | theta[G]
    DevBuf<double> part;    // per-workgroup partials of either pass
    DevBuf<double> trace;   // logLik, max_iter of the largest fit so far
    DevBuf<double> psis, out;  // VRX_BULK_Q x K, VRX_BULK_Q
    DevBuf<int32_t> ctl;
    // the cohort (vrx_bulk_set_cohort): n_sample count vectors on the same GT_prob
    int64_t n_sample = 0;
    int T_co = 0, n_wg_co = 0;        // the cohort fit pass; functions of (N, K, G) alone
    int T_co_ll = 0, n_wg_co_ll = 0;  // the cohort log-likelihood pass
    size_t lds_co = 0, lds_co_ll = 0, lds_max = 0;
    DevBuf<double2> AB_co;     // [n_sample][N]
    DevBuf<double> par_co;     // [n_sample][K + G]
    DevBuf<double> part_co;    // [chunk][workgroup][slot][.] of either cohort pass
    DevBuf<double> trace_co;   // [n_sample][max_iter]
    DevBuf<double> psis_co, out_co;  // [n_sample][n_psi][K], [n_sample][n_psi]
    DevBuf<int32_t> ctl_co;    // [n_sample][VRX_BULK_CTL_WORDS]
};

// variants per tile: even, <= 256 (a lane per variant), inside the LDS budget; at least 2
static int bulk_tile(int64_t N, int K, int G, bool fit, bool cohort = false) {
    const VrxBulkShape h0 = vrx_bulk_shape(K, G, 0);
    const size_t fixed = (cohort ? (fit ? vrx_bulk_cohort_lds_doubles(h0) : vrx_bulk_cohort_ll_lds_doubles(h0))
                                 : (fit ? vrx_bulk_lds_doubles(h0) : vrx_bulk_ll_lds_doubles(h0))) *
                         sizeof(double);
    const size_t per = (size_t)(fit ? h0.S + h0.SK + 2 : h0.S) * sizeof(double);
    const size_t budget = cohort ? VRX_BULK_COHORT_LDS : VRX_BULK_LDS_TILE;
    int64_t T = budget > fixed ? (int64_t)((budget - fixed) / per) : 0;
    T = std::min<int64_t>(T, VRX_BULK_BLOCK);
    T = std::min<int64_t>(T, N + (N & 1));
    T &= ~(int64_t)1;
    return (int)std::max<int64_t>(T, 2);
}

static int bulk_upload_counts(vrx_bulk* b, const double* AD, const double* DP) {
    std::vector<double2> ab((size_t)b->N);
    for (int64_t n = 0; n < b->N; ++n) ab[(size_t)n] = make_double2(AD[n], DP[n] - AD[n]);
    VRX_HIP(b->AB.upload(ab.data(), (size_t)b->N, b->stream));
    VRX_HIP(hipStreamSynchronize(b->stream));  // (ab dies at return)
    return VRX_OK;
}

extern "C" void vrx_bulk_destroy(vrx_bulk* b) { vrx_destroy(b); }

extern "C" int vrx_bulk_create(int device, int64_t n_var, int64_t n_donor, int64_t n_gt, const double* GT_prob,
                               const double* AD, const double* DP, vrx_bulk** out) {
    VRX_REQUIRE(GT_prob && AD && DP && out, "vrx_bulk_create: null argument");
    VRX_REQUIRE(n_var >= 1 && n_var < ((int64_t)1 << 31) - 512 && n_donor >= 1 && n_gt >= 2,
                "vrx_bulk_create: 1 <= n_var < 2^31 - 512, n_donor >= 1, n_gt >= 2");
    VRX_REQUIRE(n_donor * n_gt <= (1 << 20), "vrx_bulk_create: n_donor x n_gt too large");
    VrxOwned<vrx_bulk> b(new vrx_bulk());
    VRX_TRY(b->open("vrx_bulk_create", device, 2));
    b->N = n_var;
    b->K = (int)n_donor;
    b->G = (int)n_gt;
    hipDeviceProp_t prop;
    VRX_HIP(hipGetDeviceProperties(&prop, device));
    b->n_cu = prop.multiProcessorCount;
    // what a launch may ask for without the opt-in attribute (the device property may say more)
    const size_t lds_max = std::min<size_t>(prop.sharedMemPerBlock, 64 * 1024);
    b->T = bulk_tile(n_var, b->K, b->G, true);
    b->T_ll = bulk_tile(n_var, b->K, b->G, false);
    b->lds = vrx_bulk_lds_doubles(vrx_bulk_shape(b->K, b->G, b->T)) * sizeof(double);
    b->lds_ll = vrx_bulk_ll_lds_doubles(vrx_bulk_shape(b->K, b->G, b->T_ll)) * sizeof(double);
    VRX_REQUIRE(b->lds <= lds_max && b->lds_ll <= lds_max && (size_t)(b->K + 2 * b->G + 2) * sizeof(double) <= lds_max,
                "vrx_bulk_create: n_donor x n_gt = %lld x %lld needs %zu bytes of LDS per workgroup (limit %zu)",
                (long long)n_donor, (long long)n_gt, std::max(b->lds, b->lds_ll), lds_max);
    // workgroups: as many as stay resident (LDS-bound, at most 4 per CU), each walking tiles grid-stride
    auto grid = [&](int T, size_t lds) {
        const int64_t n_tile = (n_var + T - 1) / T;
        const int per_cu = (int)std::min<size_t>(4, std::max<size_t>(1, (size_t)(160 * 1024) / lds));
        return (int)std::min<int64_t>(n_tile, (int64_t)b->n_cu * per_cu);
    };
    b->n_wg = grid(b->T, b->lds);
    b->n_wg_ll = grid(b->T_ll, b->lds_ll);
    // the cohort passes: shapes now (of N, K, G alone), the LDS check when a cohort is set -- a donor
    // count the single-sample passes take may be too large for VRX_BULK_COHORT sets of accumulators
    b->lds_max = lds_max;
    b->T_co = bulk_tile(n_var, b->K, b->G, true, true);
    b->T_co_ll = bulk_tile(n_var, b->K, b->G, false, true);
    b->lds_co = vrx_bulk_cohort_lds_doubles(vrx_bulk_shape(b->K, b->G, b->T_co)) * sizeof(double);
    b->lds_co_ll = vrx_bulk_cohort_ll_lds_doubles(vrx_bulk_shape(b->K, b->G, b->T_co_ll)) * sizeof(double);
    b->n_wg_co = grid(b->T_co, b->lds_co);
    b->n_wg_co_ll = grid(b->T_co_ll, b->lds_co_ll);
    VRX_HIP(b->P.upload(GT_prob, (size_t)(n_var * n_donor * n_gt), b->stream));
    VRX_TRY(bulk_upload_counts(b.get(), AD, DP));
    VRX_HIP(b->par.alloc((size_t)(b->K + b->G)));
    VRX_HIP(b->part.alloc(std::max((size_t)b->n_wg * (b->K + 2 * b->G + 1), (size_t)b->n_wg_ll * VRX_BULK_Q)));
    VRX_HIP(b->psis.alloc((size_t)VRX_BULK_Q * b->K));
    VRX_HIP(b->out.alloc(VRX_BULK_Q));
    VRX_HIP(b->ctl.alloc(VRX_BULK_CTL_WORDS));
    *out = b.release();
    return VRX_OK;
}

extern "C" int vrx_bulk_set_counts(vrx_bulk* b, const double* AD, const double* DP) {
    VRX_REQUIRE(b && AD && DP, "vrx_bulk_set_counts: null argument");
    VRX_TRY(b->use());
    return bulk_upload_counts(b, AD, DP);
}

// The schedule of both fits.  As in vrx_model_fit: the stop rule runs on the device (the finish kernel
// of a pass); the host enqueues a batch of passes, then reads the n_ctl control words at d_ctl into hctl.
// The first batch reaches the first pass the rule can fire after; a kernel launched behind the stop
// returns at once.  enqueue() launches one pass on the handle's stream; stopped() says after a batch
// whether hctl holds every stop word set, which ends the loop (as does pass max_iter).  The events 0 and 1
// bracket the passes.
template <class Enqueue, class Stopped>
static int bulk_run_passes(vrx_bulk* b, int32_t max_iter, int32_t min_iter, const int32_t* d_ctl, int32_t* hctl,
                           size_t n_ctl, Enqueue enqueue, Stopped stopped) {
    hipStream_t s = b->stream;
    const int batch = VRX_BULK_BATCH;
    const int64_t n_pass = (int64_t)max_iter + 1;  // pass p closes iteration p - 1
    int64_t next = 0;
    bool stop = false;
    VRX_HIP(hipEventRecord(b->ev[0], s));
    while (next < n_pass && !stop) {
        const int64_t first = std::max<int64_t>((int64_t)std::max(min_iter, 0) + 3, batch);
        const int64_t upto = std::min(n_pass, next == 0 ? first : next + batch);
        for (; next < upto; ++next) enqueue();
        VRX_HIP(hipGetLastError());
        VRX_HIP(hipEventRecord(b->ev[1], s));
        VRX_HIP(hipMemcpyAsync(hctl, d_ctl, n_ctl * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        VRX_HIP(hipStreamSynchronize(s));
        stop = stopped();
    }
    return VRX_OK;
}

extern "C" int vrx_bulk_fit(vrx_bulk* b, double* psi_io, double* theta_io, int32_t max_iter, int32_t min_iter,
                            double epsilon, int32_t learn_theta, int32_t delay_fit_theta, double* logLik_trace,
                            int32_t* last_it, double* ms_out) {
    VRX_REQUIRE(b && psi_io && theta_io && logLik_trace && last_it, "vrx_bulk_fit: null argument");
    VRX_REQUIRE(max_iter >= 1, "vrx_bulk_fit: max_iter must be >= 1");
    VRX_TRY(b->use());
    hipStream_t s = b->stream;
    const int K = b->K, G = b->G, W = K + 2 * G + 1;
    if (b->trace.n < (size_t)max_iter) VRX_HIP(b->trace.alloc((size_t)max_iter));
    VRX_HIP(hipMemcpyAsync(b->par.p, psi_io, (size_t)K * sizeof(double), hipMemcpyHostToDevice, s));
    VRX_HIP(hipMemcpyAsync(b->par.p + K, theta_io, (size_t)G * sizeof(double), hipMemcpyHostToDevice, s));
    VRX_HIP(hipMemsetAsync(b->ctl.p, 0, VRX_BULK_CTL_WORDS * sizeof(int32_t), s));
    int32_t hctl[VRX_BULK_CTL_WORDS] = {};
    int rc = bulk_run_passes(
        b, max_iter, min_iter, b->ctl.p, hctl, VRX_BULK_CTL_WORDS,
        [&] {
            if (G == 3)
                vrx_bulk_pass<3><<<b->n_wg, VRX_BULK_BLOCK, b->lds, s>>>((int)b->N, K, G, b->T, b->P.p, b->AB.p,
                                                                         b->par.p, b->ctl.p, b->part.p);
            else
                vrx_bulk_pass<0><<<b->n_wg, VRX_BULK_BLOCK, b->lds, s>>>((int)b->N, K, G, b->T, b->P.p, b->AB.p,
                                                                         b->par.p, b->ctl.p, b->part.p);
            vrx_bulk_finish<<<1, 1024, (size_t)(W + 1) * sizeof(double), s>>>(
                b->n_wg, K, G, b->part.p, b->par.p, b->trace.p, b->ctl.p, min_iter, max_iter, epsilon, learn_theta,
                delay_fit_theta);
        },
        [&] { return hctl[VRX_BULK_STOP] != 0; });
    if (rc) return rc;
    VRX_REQUIRE(hctl[VRX_BULK_STOP], "vrx_bulk_fit: the loop ended without its last iteration");
    const int it = hctl[VRX_BULK_IT];
    *last_it = it;
    VRX_HIP(hipMemcpyAsync(logLik_trace, b->trace.p, (size_t)(it + 1) * sizeof(double), hipMemcpyDeviceToHost, s));
    VRX_HIP(hipMemcpyAsync(psi_io, b->par.p, (size_t)K * sizeof(double), hipMemcpyDeviceToHost, s));
    VRX_HIP(hipMemcpyAsync(theta_io, b->par.p + K, (size_t)G * sizeof(double), hipMemcpyDeviceToHost, s));
    VRX_HIP(hipStreamSynchronize(s));
    return b->ms(0, 1, ms_out);
}

extern "C" int vrx_bulk_loglik(vrx_bulk* b, int64_t n_psi, const double* psi, const double* theta, double* out) {
    VRX_REQUIRE(b && psi && theta && out, "vrx_bulk_loglik: null argument");
    VRX_REQUIRE(n_psi >= 1, "vrx_bulk_loglik: n_psi must be >= 1");
    VRX_TRY(b->use());
    hipStream_t s = b->stream;
    const int K = b->K, G = b->G;
    VRX_HIP(hipMemcpyAsync(b->par.p + K, theta, (size_t)G * sizeof(double), hipMemcpyHostToDevice, s));
    for (int64_t q0 = 0; q0 < n_psi; q0 += VRX_BULK_Q) {
        const int nq = (int)std::min<int64_t>(VRX_BULK_Q, n_psi - q0);
        VRX_HIP(hipMemcpyAsync(b->psis.p, psi + q0 * K, (size_t)nq * K * sizeof(double), hipMemcpyHostToDevice, s));
        if (G == 3)
            vrx_bulk_ll<3><<<b->n_wg_ll, VRX_BULK_BLOCK, b->lds_ll, s>>>((int)b->N, K, G, b->T_ll, nq, b->P.p, b->AB.p,
                                                                         b->psis.p, b->par.p + K, b->part.p);
        else
            vrx_bulk_ll<0><<<b->n_wg_ll, VRX_BULK_BLOCK, b->lds_ll, s>>>((int)b->N, K, G, b->T_ll, nq, b->P.p, b->AB.p,
                                                                         b->psis.p, b->par.p + K, b->part.p);
        vrx_bulk_ll_sum<<<1, 1024, 0, s>>>(b->n_wg_ll, nq, b->part.p, b->out.p);
        VRX_HIP(hipGetLastError());
        VRX_HIP(hipMemcpyAsync(out + q0, b->out.p, (size_t)nq * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    VRX_HIP(hipStreamSynchronize(s));
    return VRX_OK;
}

extern "C" int32_t vrx_bulk_cohort_chunk(void) { return VRX_BULK_COHORT; }

extern "C" int vrx_bulk_info(const vrx_bulk* b, int32_t out[8]) {
    VRX_REQUIRE(b && out, "vrx_bulk_info: null argument");
    const int v[8] = {b->T, b->n_wg, b->T_ll, b->n_wg_ll, b->T_co, b->n_wg_co, b->T_co_ll, b->n_wg_co_ll};
    for (int i = 0; i < 8; ++i) out[i] = v[i];
    return VRX_OK;
}

extern "C" int vrx_bulk_set_cohort(vrx_bulk* b, int64_t n_sample, const double* AD, const double* DP) {
    VRX_REQUIRE(b && AD && DP, "vrx_bulk_set_cohort: null argument");
    VRX_REQUIRE(n_sample >= 1 && n_sample <= (1 << 16), "vrx_bulk_set_cohort: 1 <= n_sample <= 65536");
    VRX_REQUIRE(b->lds_co <= b->lds_max && b->lds_co_ll <= b->lds_max,
                "vrx_bulk_set_cohort: n_donor x n_gt = %d x %d needs %zu bytes of LDS per workgroup for a chunk of "
                "%d samples (limit %zu)",
                b->K, b->G, std::max(b->lds_co, b->lds_co_ll), VRX_BULK_COHORT, b->lds_max);
    VRX_TRY(b->use());
    const size_t S = (size_t)n_sample, N = (size_t)b->N;
    const size_t n_chunk = (S + VRX_BULK_COHORT - 1) / VRX_BULK_COHORT;
    b->n_sample = 0;  // (no cohort while this one is half built)
    {
        std::vector<double2> ab(S * N);
        for (size_t i = 0; i < S * N; ++i) ab[i] = make_double2(AD[i], DP[i] - AD[i]);
        VRX_HIP(b->AB_co.upload(ab.data(), S * N, b->stream));
        VRX_HIP(hipStreamSynchronize(b->stream));  // (ab dies here)
    }
    VRX_HIP(b->par_co.alloc(S * (size_t)(b->K + b->G)));
    VRX_HIP(b->ctl_co.alloc(S * VRX_BULK_CTL_WORDS));
    VRX_HIP(b->part_co.alloc(n_chunk * VRX_BULK_COHORT *
                             std::max((size_t)b->n_wg_co * (b->K + 2 * b->G + 1), (size_t)b->n_wg_co_ll * VRX_BULK_Q)));
    b->n_sample = n_sample;
    return VRX_OK;
}

extern "C" int vrx_bulk_fit_cohort(vrx_bulk* b, double* psi_io, double* theta_io, int32_t max_iter, int32_t min_iter,
                                   double epsilon, int32_t learn_theta, int32_t delay_fit_theta, double* logLik_trace,
                                   int32_t* last_it, double* ms_out) {
    VRX_REQUIRE(b && psi_io && theta_io && logLik_trace && last_it, "vrx_bulk_fit_cohort: null argument");
    VRX_REQUIRE(b->n_sample >= 1, "vrx_bulk_fit_cohort: no cohort set (vrx_bulk_set_cohort)");
    VRX_REQUIRE(max_iter >= 1, "vrx_bulk_fit_cohort: max_iter must be >= 1");
    VRX_TRY(b->use());
    hipStream_t s = b->stream;
    const int K = b->K, G = b->G, S = (int)b->n_sample;
    const int n_chunk = (S + VRX_BULK_COHORT - 1) / VRX_BULK_COHORT;
    const size_t n_trace = (size_t)S * max_iter;
    if (b->trace_co.n < n_trace) VRX_HIP(b->trace_co.alloc(n_trace));
    std::vector<double> par((size_t)S * (K + G));
    for (int i = 0; i < S; ++i) {
        std::copy(psi_io + (size_t)i * K, psi_io + (size_t)(i + 1) * K, par.begin() + (size_t)i * (K + G));
        std::copy(theta_io + (size_t)i * G, theta_io + (size_t)(i + 1) * G, par.begin() + (size_t)i * (K + G) + K);
    }
    VRX_HIP(hipMemcpyAsync(b->par_co.p, par.data(), par.size() * sizeof(double), hipMemcpyHostToDevice, s));
    VRX_HIP(hipMemsetAsync(b->ctl_co.p, 0, (size_t)S * VRX_BULK_CTL_WORDS * sizeof(int32_t), s));
    VRX_HIP(hipMemsetAsync(b->trace_co.p, 0, n_trace * sizeof(double), s));
    // The schedule of vrx_bulk_fit with a stop word per sample: the loop ends when all have stopped.  A
    // stopped sample does no work in the passes behind its stop and its state is not written again.
    std::vector<int32_t> hctl((size_t)S * VRX_BULK_CTL_WORDS, 0);
    auto all_stopped = [&] {
        for (int i = 0; i < S; ++i)
            if (!hctl[(size_t)i * VRX_BULK_CTL_WORDS + VRX_BULK_STOP]) return false;
        return true;
    };
    const dim3 grid((unsigned)b->n_wg_co, (unsigned)n_chunk);
    int rc = bulk_run_passes(
        b, max_iter, min_iter, b->ctl_co.p, hctl.data(), hctl.size(),
        [&] {
            if (G == 3)
                vrx_bulk_cohort_pass<3><<<grid, VRX_BULK_BLOCK, b->lds_co, s>>>(
                    (int)b->N, K, G, b->T_co, S, b->P.p, b->AB_co.p, b->par_co.p, b->ctl_co.p, b->part_co.p);
            else
                vrx_bulk_cohort_pass<0><<<grid, VRX_BULK_BLOCK, b->lds_co, s>>>(
                    (int)b->N, K, G, b->T_co, S, b->P.p, b->AB_co.p, b->par_co.p, b->ctl_co.p, b->part_co.p);
            vrx_bulk_cohort_finish<<<S, 1024, (size_t)(K + 2 * G + 2) * sizeof(double), s>>>(
                b->n_wg_co, K, G, b->part_co.p, b->par_co.p, b->trace_co.p, b->ctl_co.p, min_iter, max_iter, epsilon,
                learn_theta, delay_fit_theta);
        },
        all_stopped);
    if (rc) return rc;
    VRX_REQUIRE(all_stopped(), "vrx_bulk_fit_cohort: the loop ended without every sample's last iteration");
    for (int i = 0; i < S; ++i) last_it[i] = hctl[(size_t)i * VRX_BULK_CTL_WORDS + VRX_BULK_IT];
    // (the whole trace: entries behind a sample's last iteration are the zeros it started with)
    VRX_HIP(hipMemcpyAsync(logLik_trace, b->trace_co.p, n_trace * sizeof(double), hipMemcpyDeviceToHost, s));
    VRX_HIP(hipMemcpyAsync(par.data(), b->par_co.p, par.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    VRX_HIP(hipStreamSynchronize(s));
    for (int i = 0; i < S; ++i) {
        const double* src = par.data() + (size_t)i * (K + G);
        std::copy(src, src + K, psi_io + (size_t)i * K);
        std::copy(src + K, src + K + G, theta_io + (size_t)i * G);
    }
    return b->ms(0, 1, ms_out);
}

extern "C" int vrx_bulk_loglik_cohort(vrx_bulk* b, int64_t n_psi, const double* psi, const double* theta,
                                      double* out) {
    VRX_REQUIRE(b && psi && theta && out, "vrx_bulk_loglik_cohort: null argument");
    VRX_REQUIRE(b->n_sample >= 1, "vrx_bulk_loglik_cohort: no cohort set (vrx_bulk_set_cohort)");
    VRX_REQUIRE(n_psi >= 1 && n_psi <= (1 << 20), "vrx_bulk_loglik_cohort: 1 <= n_psi <= 2^20");
    VRX_TRY(b->use());
    hipStream_t s = b->stream;
    const int K = b->K, G = b->G, S = (int)b->n_sample;
    const int n_chunk = (S + VRX_BULK_COHORT - 1) / VRX_BULK_COHORT;
    const size_t n_in = (size_t)S * n_psi * K, n_out = (size_t)S * n_psi;
    if (b->psis_co.n < n_in) VRX_HIP(b->psis_co.alloc(n_in));
    if (b->out_co.n < n_out) VRX_HIP(b->out_co.alloc(n_out));
    VRX_HIP(hipMemcpyAsync(b->psis_co.p, psi, n_in * sizeof(double), hipMemcpyHostToDevice, s));
    // (theta rides in par_co's first n_sample x G doubles: no fit is in flight on this stream)
    VRX_HIP(hipMemcpyAsync(b->par_co.p, theta, (size_t)S * G * sizeof(double), hipMemcpyHostToDevice, s));
    const dim3 grid((unsigned)b->n_wg_co_ll, (unsigned)n_chunk);
    for (int64_t q0 = 0; q0 < n_psi; q0 += VRX_BULK_Q) {
        const int nq = (int)std::min<int64_t>(VRX_BULK_Q, n_psi - q0);
        if (G == 3)
            vrx_bulk_cohort_ll<3><<<grid, VRX_BULK_BLOCK, b->lds_co_ll, s>>>((int)b->N, K, G, b->T_co_ll, S, (int)n_psi,
                                                                             (int)q0, nq, b->P.p, b->AB_co.p,
                                                                             b->psis_co.p, b->par_co.p, b->part_co.p);
        else
            vrx_bulk_cohort_ll<0><<<grid, VRX_BULK_BLOCK, b->lds_co_ll, s>>>((int)b->N, K, G, b->T_co_ll, S, (int)n_psi,
                                                                             (int)q0, nq, b->P.p, b->AB_co.p,
                                                                             b->psis_co.p, b->par_co.p, b->part_co.p);
        vrx_bulk_cohort_ll_sum<<<S, 1024, 0, s>>>(b->n_wg_co_ll, (int)n_psi, (int)q0, nq, b->part_co.p, b->out_co.p);
        VRX_HIP(hipGetLastError());
    }
    VRX_HIP(hipMemcpyAsync(out, b->out_co.p, n_out * sizeof(double), hipMemcpyDeviceToHost, s));
    VRX_HIP(hipStreamSynchronize(s));
    return VRX_OK;
}
