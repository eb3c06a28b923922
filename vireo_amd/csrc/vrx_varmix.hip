// Per-variant clone mixtures: the vrx_varmix_* entries of include/vireo_hip.h on the kernel of vrx_varmix.h.
// A handle owns its stream, events and buffers; nothing here touches a vrx_problem or a vrx_model.
#include <algorithm>
#include <numeric>

#include "vrx_handle.h"
#include "vrx_varmix.h"

struct vrx_varmix : VrxQueue {  // ev: 0, 1 bracket the fit kernel
    int64_t n_var = 0, nnz = 0, n_long = 0;
    DevBuf<int32_t> perm, len, pairs, n_iter, warn;
    DevBuf<int64_t> start;
    DevBuf<double> elbo, mu, sum, size, trace;  // elbo: K components | one component
    DevBuf<VrxVmArgs> args;
};

extern "C" int32_t vrx_varmix_wave_rows(void) { return VRX_VM_WAVE_ROWS; }

extern "C" void vrx_varmix_destroy(vrx_varmix* h) { vrx_destroy(h); }

extern "C" int vrx_varmix_create(int device, int64_t n_var, int64_t nnz, const int64_t* rowptr, const int32_t* ad,
                                 const int32_t* dp, vrx_varmix** out) {
    VRX_REQUIRE(rowptr && out, "vrx_varmix_create: null argument");
    VRX_REQUIRE(n_var >= 0 && n_var < ((int64_t)1 << 31) - 4, "vrx_varmix_create: 0 <= n_var < 2^31 - 4");
    VRX_REQUIRE(nnz >= 0 && (nnz == 0 || (ad && dp)), "vrx_varmix_create: nnz entries need ad and dp");
    VRX_REQUIRE(rowptr[0] == 0 && rowptr[n_var] == nnz, "vrx_varmix_create: rowptr must run from 0 to nnz");
    for (int64_t v = 0; v < n_var; ++v) {
        VRX_REQUIRE(rowptr[v] <= rowptr[v + 1], "vrx_varmix_create: rowptr decreases at row %lld", (long long)v);
        VRX_REQUIRE(rowptr[v + 1] - rowptr[v] < ((int64_t)1 << 31) - 4,
                    "vrx_varmix_create: row %lld has 2^31 entries or more", (long long)v);
    }
    for (int64_t e = 0; e < nnz; ++e)
        VRX_REQUIRE(dp[e] > 0 && ad[e] >= 0 && ad[e] <= dp[e],
                    "vrx_varmix_create: entry %lld has ad = %d, dp = %d (need 0 <= ad <= dp, dp > 0)", (long long)e,
                    (int)ad[e], (int)dp[e]);
    VrxOwned<vrx_varmix> h(new vrx_varmix());
    VRX_TRY(h->open("vrx_varmix_create", device, 2));
    h->n_var = n_var;
    h->nnz = nnz;
    // rows longest first (equal lengths in input order), each padded to whole pairs of entries
    const size_t N = (size_t)n_var;
    std::vector<int32_t> perm(N), len(N);
    std::vector<int64_t> start(N);
    int64_t total = 0;
    for (size_t v = 0; v < N; ++v) {
        len[v] = (int32_t)(rowptr[v + 1] - rowptr[v]);
        start[v] = total;
        total += (len[v] + 1) & ~(int64_t)1;
        if (len[v] > VRX_VM_WAVE_ROWS) ++h->n_long;
    }
    std::iota(perm.begin(), perm.end(), 0);
    std::stable_sort(perm.begin(), perm.end(), [&](int32_t a, int32_t b) { return len[a] > len[b]; });
    std::vector<int32_t> pairs((size_t)total * 2, 0);
    for (size_t v = 0; v < N; ++v)
        for (int64_t e = 0; e < len[v]; ++e) {
            pairs[(size_t)(start[v] + e) * 2] = ad[rowptr[v] + e];
            pairs[(size_t)(start[v] + e) * 2 + 1] = dp[rowptr[v] + e];
        }
    hipStream_t s = h->stream;
    VRX_HIP(h->perm.upload(perm.data(), N, s));
    VRX_HIP(h->len.upload(len.data(), N, s));
    VRX_HIP(h->start.upload(start.data(), N, s));
    VRX_HIP(h->pairs.upload(pairs.data(), pairs.size(), s));
    VRX_HIP(h->elbo.alloc(2 * N));
    VRX_HIP(h->n_iter.alloc(N));
    VRX_HIP(h->warn.alloc(N));
    VRX_HIP(h->mu.alloc(N * VRX_VM_MAX_K));
    VRX_HIP(h->sum.alloc(N * VRX_VM_MAX_K));
    VRX_HIP(h->size.alloc(N * VRX_VM_MAX_K));
    VRX_HIP(h->args.alloc(1));
    VRX_HIP(hipStreamSynchronize(s));  // (the host vectors die at return)
    *out = h.release();
    return VRX_OK;
}

template <int K>
static void vrx_varmix_launch(const VrxVmArgs* g, unsigned n_blk, hipStream_t s) {
    vrx_varmix_fit_k<K><<<n_blk, VRX_VM_BLOCK, 0, s>>>(g);
}

extern "C" int vrx_varmix_fit(vrx_varmix* h, int32_t n_clone, int32_t max_iter, int32_t min_iter, double epsilon_conv,
                              double* elbo_k, double* elbo_one, double* beta_mu, double* beta_sum, double* size,
                              int32_t* n_iter, int32_t* warn, double* trace, double* ms) {
    VRX_REQUIRE(h, "vrx_varmix_fit: null handle");
    if (n_clone < VRX_VM_MIN_K || n_clone > VRX_VM_MAX_K) {
        vrx_set_error("vrx_varmix_fit: n_clone = %d, built for %d ... %d components", (int)n_clone, VRX_VM_MIN_K,
                      VRX_VM_MAX_K);
        return VRX_ERR_UNSUPPORTED;
    }
    if (max_iter < 2) {
        vrx_set_error("vrx_varmix_fit: max_iter = %d, the bound returned is ELBO[it - 1] and needs max_iter >= 2",
                      (int)max_iter);
        return VRX_ERR_UNSUPPORTED;
    }
    VRX_REQUIRE(min_iter >= 0, "vrx_varmix_fit: min_iter must not be negative");
    VRX_REQUIRE(epsilon_conv == epsilon_conv, "vrx_varmix_fit: epsilon_conv is NaN");
    const size_t N = (size_t)h->n_var;
    VRX_REQUIRE(N == 0 || (elbo_k && elbo_one && n_iter && warn), "vrx_varmix_fit: null output");
    if (ms) *ms = 0.0;
    if (N == 0) return VRX_OK;
    VRX_TRY(h->use());
    hipStream_t s = h->stream;
    const size_t n_trace = trace ? N * (size_t)max_iter : 0;
    if (trace) {
        if (h->trace.n < n_trace) VRX_HIP(h->trace.alloc(n_trace));
        VRX_HIP(hipMemsetAsync(h->trace.p, 0, n_trace * sizeof(double), s));
    }
    VrxVmArgs g;
    g.n_var = h->n_var;
    g.n_long = h->n_long;
    g.perm = h->perm.p;
    g.start = h->start.p;
    g.len = h->len.p;
    g.pairs = reinterpret_cast<const int4*>(h->pairs.p);
    g.max_iter = max_iter;
    g.min_iter = min_iter;
    g.eps = epsilon_conv;
    g.elbo_k = h->elbo.p;
    g.elbo_one = h->elbo.p + N;
    g.mu = h->mu.p;
    g.sum = h->sum.p;
    g.size = h->size.p;
    g.n_iter = h->n_iter.p;
    g.warn = h->warn.p;
    g.trace = trace ? h->trace.p : nullptr;
    const int64_t n_short = h->n_var - h->n_long;
    const unsigned n_blk = (unsigned)(h->n_long + (n_short + VRX_VM_WAVES - 1) / VRX_VM_WAVES);
    VRX_HIP(hipMemcpyAsync(h->args.p, &g, sizeof g, hipMemcpyHostToDevice, s));
    VRX_HIP(hipStreamSynchronize(s));  // (g is a local)
    VRX_HIP(hipEventRecord(h->ev[0], s));
    switch (n_clone) {
        case 2: vrx_varmix_launch<2>(h->args.p, n_blk, s); break;
        case 3: vrx_varmix_launch<3>(h->args.p, n_blk, s); break;
        case 4: vrx_varmix_launch<4>(h->args.p, n_blk, s); break;
        case 5: vrx_varmix_launch<5>(h->args.p, n_blk, s); break;
        case 6: vrx_varmix_launch<6>(h->args.p, n_blk, s); break;
        case 7: vrx_varmix_launch<7>(h->args.p, n_blk, s); break;
        default: vrx_varmix_launch<8>(h->args.p, n_blk, s); break;
    }
    VRX_HIP(hipGetLastError());
    VRX_HIP(hipEventRecord(h->ev[1], s));
    const size_t NK = N * (size_t)n_clone;
    VRX_HIP(hipMemcpyAsync(elbo_k, g.elbo_k, N * sizeof(double), hipMemcpyDeviceToHost, s));
    VRX_HIP(hipMemcpyAsync(elbo_one, g.elbo_one, N * sizeof(double), hipMemcpyDeviceToHost, s));
    VRX_HIP(hipMemcpyAsync(n_iter, g.n_iter, N * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    VRX_HIP(hipMemcpyAsync(warn, g.warn, N * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (beta_mu) VRX_HIP(hipMemcpyAsync(beta_mu, g.mu, NK * sizeof(double), hipMemcpyDeviceToHost, s));
    if (beta_sum) VRX_HIP(hipMemcpyAsync(beta_sum, g.sum, NK * sizeof(double), hipMemcpyDeviceToHost, s));
    if (size) VRX_HIP(hipMemcpyAsync(size, g.size, NK * sizeof(double), hipMemcpyDeviceToHost, s));
    if (trace) VRX_HIP(hipMemcpyAsync(trace, g.trace, n_trace * sizeof(double), hipMemcpyDeviceToHost, s));
    VRX_HIP(hipStreamSynchronize(s));
    return h->ms(0, 1, ms);
}
