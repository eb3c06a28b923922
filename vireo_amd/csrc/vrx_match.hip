// Donor matching: vrx_geno_dist of include/vireo_hip.h on the kernels of vrx_match.h.  A call owns its
// stream, events and buffers; nothing here touches a vrx_problem or a vrx_model.
#include <algorithm>

#include "vrx_handle.h"
#include "vrx_match.h"

// the stream and the two events of one vrx_geno_dist call (released on every return path)
using GenoCall = VrxQueue;

extern "C" int vrx_geno_dist(int device, int64_t n_var, int64_t k1, int64_t k2, int64_t n_gt, const double* X,
                             const double* Z, int64_t block_vars, double* D, double* ms_out) {
    VRX_REQUIRE(X && D, "vrx_geno_dist: null argument");
    if (!Z) VRX_REQUIRE(k2 == k1, "vrx_geno_dist: Z = NULL compares X with itself, k2 must equal k1");
    VRX_REQUIRE(n_var >= 1 && k1 >= 1 && k2 >= 1 && n_gt >= 1 && block_vars >= 0,
                "vrx_geno_dist: n_var >= 1, k1 >= 1, k2 >= 1, n_gt >= 1, block_vars >= 0");
    const int64_t kmax = std::max(k1, k2);
    if (n_gt > (1 << 20) || kmax > (1 << 20) || kmax * n_gt >= ((int64_t)1 << 28)) {
        vrx_set_error("vrx_geno_dist: %lld x %lld donors x %lld genotypes: a variant's row is too long",
                      (long long)k1, (long long)k2, (long long)n_gt);
        return VRX_ERR_UNSUPPORTED;
    }
    const int G = (int)n_gt;
    const VrxGenoShape h = vrx_geno_shape(k1, k2, G);
    const size_t lds = vrx_geno_lds_doubles(h) * sizeof(double);
    const int64_t n_ij = ((k1 + h.TI - 1) / h.TI) * ((k2 + h.TJ - 1) / h.TJ);
    if (h.T < 1 || lds > (size_t)VRX_GENO_LDS || n_ij > 65535) {
        vrx_set_error("vrx_geno_dist: %lld x %lld donors x %lld genotypes unsupported (one variant of a tile must "
                      "fit %d bytes of LDS, at most 65535 output tiles)",
                      (long long)k1, (long long)k2, (long long)n_gt, VRX_GENO_LDS);
        return VRX_ERR_UNSUPPORTED;
    }
    GenoCall c;
    VRX_TRY(c.open("vrx_geno_dist", device, 2));
    hipDeviceProp_t prop;
    VRX_HIP(hipGetDeviceProperties(&prop, device));
    // variants per slab: each operand's slab at most 256 MiB by default, and below 2^31 - 1 variants
    const int64_t row_bytes = kmax * n_gt * (int64_t)sizeof(double);
    int64_t bv = block_vars > 0 ? block_vars : std::max<int64_t>(1, ((int64_t)256 << 20) / row_bytes);
    bv = std::min(std::min(bv, n_var), (int64_t)0x7fffffff - VRX_GENO_MAX_T);
    // workgroups of a slab: the output tiles times as many chunks of variant tiles as stay resident
    const int64_t n_vt = (bv + h.T - 1) / h.T;
    const int64_t resident = (int64_t)prop.multiProcessorCount * 4;
    // (at least 4 variant tiles per chunk where the slab has them: fewer partials to add)
    const int n_chunk = (int)std::max<int64_t>(1, std::min<int64_t>((n_vt + 3) / 4, resident / n_ij));
    const int64_t n_cell = k1 * k2;
    DevBuf<double> dX, dZ, part, acc;
    VRX_HIP(dX.alloc((size_t)(bv * k1 * n_gt)));
    if (Z) VRX_HIP(dZ.alloc((size_t)(bv * k2 * n_gt)));
    VRX_HIP(part.alloc((size_t)n_chunk * (size_t)n_cell));
    VRX_HIP(acc.alloc((size_t)n_cell));
    const double* pZ = Z ? dZ.p : dX.p;
    hipStream_t s = c.stream;
    double ms = 0.0, t = 0.0;
    for (int64_t n0 = 0; n0 < n_var; n0 += bv) {
        const int64_t nv = std::min(bv, n_var - n0);
        const bool last = n0 + nv == n_var;
        VRX_HIP(hipMemcpyAsync(dX.p, X + n0 * k1 * n_gt, (size_t)(nv * k1 * n_gt) * sizeof(double),
                               hipMemcpyHostToDevice, s));
        if (Z)
            VRX_HIP(hipMemcpyAsync(dZ.p, Z + n0 * k2 * n_gt, (size_t)(nv * k2 * n_gt) * sizeof(double),
                                   hipMemcpyHostToDevice, s));
        // (a short last slab keeps the grid: a chunk without variant tiles writes zeros)
        const dim3 grid((unsigned)n_chunk, (unsigned)n_ij);
        VRX_HIP(hipEventRecord(c.ev[0], s));
        if (G == 3)
            vrx_geno_pass<3><<<grid, VRX_GENO_BLOCK, lds, s>>>((int)nv, (int)k1, (int)k2, h, dX.p, pZ, part.p);
        else
            vrx_geno_pass<0><<<grid, VRX_GENO_BLOCK, lds, s>>>((int)nv, (int)k1, (int)k2, h, dX.p, pZ, part.p);
        vrx_geno_sum<<<(unsigned)((n_cell + 63) / 64), 64 * VRX_GENO_SUM_RUNS, 0, s>>>(
            n_chunk, n_cell, part.p, acc.p, n0 == 0, last ? (double)n_var * (double)n_gt : 0.0);
        VRX_HIP(hipGetLastError());
        VRX_HIP(hipEventRecord(c.ev[1], s));
        VRX_HIP(hipStreamSynchronize(s));  // (the next upload overwrites the slab)
        VRX_TRY(c.ms(0, 1, &t));
        ms += t;
    }
    VRX_HIP(hipMemcpyAsync(D, acc.p, (size_t)n_cell * sizeof(double), hipMemcpyDeviceToHost, s));
    VRX_HIP(hipStreamSynchronize(s));
    if (ms_out) *ms_out = ms;
    return VRX_OK;
}
