// Barcode selection: the vrx_barcode_* entries of include/vireo_hip.h on the kernels of vrx_barcode.h and
// hipCUB.  A handle owns its stream, events and buffers; nothing here touches a vrx_problem or a vrx_model.
#include <algorithm>

#include "vrx_handle.h"
#include "vrx_barcode.h"

struct vrx_barcode : VrxQueue {  // ev: 0, 1, 2 around the entropy pass and the ties, 3, 4 around the median
    int64_t N = 0;      // variants
    size_t stride = 0;  // bytes between the donors' rows of GT
    int K = 0, NC = 0;
    bool has_vc = false, have_round = false;
    int64_t n_kept = 0;
    DevBuf<uint8_t> GT, flag, flag2, tmp;
    DevBuf<double> vc, ent, keys, sorted, table, part, scal;
    DevBuf<int32_t> state, tidx, kidx, ctl;  // state: order [K] | bnd [K + 1]
};

// The three hipCUB calls of a round over n items, on b->tmp, which vrx_barcode_create sizes for n_var items.
static hipError_t bc_select_tied(vrx_barcode* b, int n, VrxCub mode = VRX_CUB_RUN) {
    return vrx_cub(b->tmp,
                   VRX_CUB_CALL(DeviceSelect::Flagged, hipcub::CountingInputIterator<int32_t>(0), b->flag.p, b->tidx.p,
                                b->ctl.p + VRX_BC_TIED, n, b->stream),
                   mode);
}
static hipError_t bc_sort_keys(vrx_barcode* b, int n, VrxCub mode = VRX_CUB_RUN) {
    return vrx_cub(b->tmp, VRX_CUB_CALL(DeviceRadixSort::SortKeys, b->keys.p, b->sorted.p, n, 0, 64, b->stream),
                   mode);
}
static hipError_t bc_select_kept(vrx_barcode* b, int n, VrxCub mode = VRX_CUB_RUN) {
    return vrx_cub(b->tmp,
                   VRX_CUB_CALL(DeviceSelect::Flagged, b->tidx.p, b->flag2.p, b->kidx.p, b->ctl.p + VRX_BC_KEPT, n,
                                b->stream),
                   mode);
}

extern "C" void vrx_barcode_destroy(vrx_barcode* b) { vrx_destroy(b); }

extern "C" int vrx_barcode_create(int device, int64_t n_var, int64_t n_donor, int64_t n_cat, const uint8_t* GT,
                                  const double* var_count, vrx_barcode** out) {
    VRX_REQUIRE(GT && out, "vrx_barcode_create: null argument");
    VRX_REQUIRE(n_var >= 1 && n_var < ((int64_t)1 << 31) - 4096, "vrx_barcode_create: 1 <= n_var < 2^31 - 4096");
    VRX_REQUIRE(n_donor >= 1 && n_donor <= VRX_BC_MAX_DONORS, "vrx_barcode_create: 1 <= n_donor <= %d",
                VRX_BC_MAX_DONORS);
    VRX_REQUIRE(n_cat >= 1 && n_cat <= VRX_BC_MAX_CAT, "vrx_barcode_create: 1 <= categories <= %d", VRX_BC_MAX_CAT);
    VrxOwned<vrx_barcode> b(new vrx_barcode());
    VRX_TRY(b->open("vrx_barcode_create", device, 5));
    b->N = n_var;
    b->K = (int)n_donor;
    b->NC = n_cat <= 3 ? 3 : VRX_BC_MAX_CAT;
    b->stride = ((size_t)n_var + 255) & ~(size_t)255;
    b->has_vc = var_count != nullptr;
    const size_t N = (size_t)n_var;
    hipStream_t s = b->stream;
    VRX_HIP(b->GT.alloc(b->stride * (size_t)b->K));
    VRX_HIP(hipMemsetAsync(b->GT.p, 0, b->stride * (size_t)b->K, s));
    VRX_HIP(hipMemcpy2DAsync(b->GT.p, b->stride, GT, N, N, (size_t)b->K, hipMemcpyHostToDevice, s));
    if (var_count) VRX_HIP(b->vc.upload(var_count, N, s));
    VRX_HIP(b->ent.alloc(N));
    VRX_HIP(b->flag.alloc(N));
    VRX_HIP(b->tidx.alloc(N));
    if (var_count) {
        VRX_HIP(b->flag2.alloc(N));
        VRX_HIP(b->kidx.alloc(N));
        VRX_HIP(b->keys.alloc(N));
        VRX_HIP(b->sorted.alloc(N));
    }
    VRX_HIP(b->part.alloc(VRX_BC_MAX_BLOCKS));
    VRX_HIP(b->scal.alloc(VRX_BC_SCALARS));
    VRX_HIP(b->ctl.alloc(VRX_BC_CTL_WORDS));
    VRX_HIP(b->state.alloc((size_t)(2 * b->K + 1)));
    // the temporary storage of the largest of the three hipCUB calls of a round (a round over fewer items that
    // should ever ask for more grows it)
    VRX_HIP(bc_select_tied(b.get(), (int)n_var, VRX_CUB_SIZE));
    if (var_count) {
        VRX_HIP(bc_sort_keys(b.get(), (int)n_var, VRX_CUB_SIZE));
        VRX_HIP(bc_select_kept(b.get(), (int)n_var, VRX_CUB_SIZE));
    }
    VRX_HIP(hipStreamSynchronize(s));  // (the caller's arrays may die at return)
    *out = b.release();
    return VRX_OK;
}

extern "C" int vrx_barcode_round(vrx_barcode* b, const int32_t* order, const int32_t* bnd, int32_t n_class,
                                 const double* table, int32_t half_width, double log2, double* max_out,
                                 int64_t* counts3, double* ms2) {
    VRX_REQUIRE(b && order && bnd && table && max_out && counts3, "vrx_barcode_round: null argument");
    const int K = b->K;
    VRX_REQUIRE(n_class >= 1 && n_class <= K, "vrx_barcode_round: 1 <= n_class <= n_donor");
    VRX_REQUIRE(half_width >= 0 && half_width <= VRX_BC_MAX_H, "vrx_barcode_round: 0 <= table half-width <= %d",
                VRX_BC_MAX_H);
    VRX_REQUIRE(log2 > 0.0, "vrx_barcode_round: log(2) must be positive");
    // the state indexes GT and the table: every donor once, the classes non-empty and covering [0, K)
    {
        bool seen[VRX_BC_MAX_DONORS] = {};
        for (int k = 0; k < K; ++k) {
            VRX_REQUIRE(order[k] >= 0 && order[k] < K && !seen[order[k]],
                        "vrx_barcode_round: order is not a permutation of the donors");
            seen[order[k]] = true;
        }
        VRX_REQUIRE(bnd[0] == 0 && bnd[n_class] == K, "vrx_barcode_round: class boundaries must run from 0 to n_donor");
        for (int c = 0; c < n_class; ++c)
            VRX_REQUIRE(bnd[c] < bnd[c + 1], "vrx_barcode_round: class boundaries must increase");
    }
    VRX_TRY(b->use());
    hipStream_t s = b->stream;
    b->have_round = false;
    const size_t n_tab = (size_t)(2 * half_width + 1) * (size_t)(K + 1);
    if (b->table.n < n_tab) VRX_HIP(b->table.alloc(n_tab));
    VRX_HIP(hipMemcpyAsync(b->table.p, table, n_tab * sizeof(double), hipMemcpyHostToDevice, s));
    VRX_HIP(hipMemcpyAsync(b->state.p, order, (size_t)K * sizeof(int32_t), hipMemcpyHostToDevice, s));
    VRX_HIP(hipMemcpyAsync(b->state.p + K, bnd, (size_t)(n_class + 1) * sizeof(int32_t), hipMemcpyHostToDevice, s));
    VRX_HIP(hipMemsetAsync(b->ctl.p, 0, VRX_BC_CTL_WORDS * sizeof(int32_t), s));
    const int64_t N = b->N;
    const unsigned n_blk = (unsigned)((N + VRX_BC_BLOCK - 1) / VRX_BC_BLOCK);
    const int n_part = (int)std::min<int64_t>(n_blk, VRX_BC_MAX_BLOCKS);
    VRX_HIP(hipEventRecord(b->ev[0], s));
    if (b->NC == 3)
        vrx_barcode_entropy<3><<<n_blk, VRX_BC_BLOCK, 0, s>>>(N, b->stride, K, n_class, b->GT.p, b->state.p,
                                                              b->state.p + K, b->table.p, half_width, log2, b->ent.p,
                                                              b->ctl.p);
    else
        vrx_barcode_entropy<VRX_BC_MAX_CAT><<<n_blk, VRX_BC_BLOCK, 0, s>>>(N, b->stride, K, n_class, b->GT.p,
                                                                           b->state.p, b->state.p + K, b->table.p,
                                                                           half_width, log2, b->ent.p, b->ctl.p);
    VRX_HIP(hipEventRecord(b->ev[1], s));
    vrx_barcode_max<<<n_part, VRX_BC_BLOCK, 0, s>>>(N, b->ent.p, b->part.p);
    vrx_barcode_max2<<<1, VRX_BC_BLOCK, 0, s>>>(n_part, b->part.p, b->scal.p);
    vrx_barcode_flag<<<n_blk, VRX_BC_BLOCK, 0, s>>>(N, b->ent.p, b->scal.p, b->flag.p);
    VRX_HIP(hipGetLastError());
    VRX_HIP(bc_select_tied(b, (int)N, VRX_CUB_SIZED));  // (n_var items, as sized)
    VRX_HIP(hipEventRecord(b->ev[2], s));
    int32_t hctl[VRX_BC_CTL_WORDS] = {};
    double hmax = 0.0;
    VRX_HIP(hipMemcpyAsync(hctl, b->ctl.p, sizeof hctl, hipMemcpyDeviceToHost, s));
    VRX_HIP(hipMemcpyAsync(&hmax, b->scal.p + VRX_BC_MAX, sizeof(double), hipMemcpyDeviceToHost, s));
    VRX_HIP(hipStreamSynchronize(s));
    double ms_ent = 0.0, ms_rest = 0.0, t = 0.0;
    VRX_TRY(b->ms(0, 1, &ms_ent));
    VRX_TRY(b->ms(1, 2, &ms_rest));
    counts3[0] = hctl[VRX_BC_TIED];
    counts3[1] = 0;
    counts3[2] = hctl[VRX_BC_OUTSIDE];
    *max_out = hmax;
    if (ms2) {
        ms2[0] = ms_ent;
        ms2[1] = ms_rest;
    }
    if (hctl[VRX_BC_OUTSIDE] > 0) {
        vrx_set_error("vrx_barcode_round: %d variants have a normalising sum more than %d ulp from 1, outside the "
                      "entropy table (nothing is evaluated approximately: pass a wider table)",
                      hctl[VRX_BC_OUTSIDE], half_width);
        return VRX_ERR_UNSUPPORTED;
    }
    const int n_tied = hctl[VRX_BC_TIED];
    int64_t n_kept = n_tied;
    if (b->has_vc && n_tied > 0) {
        const unsigned t_blk = (unsigned)((n_tied + VRX_BC_BLOCK - 1) / VRX_BC_BLOCK);
        VRX_HIP(hipEventRecord(b->ev[3], s));
        vrx_barcode_gather<<<t_blk, VRX_BC_BLOCK, 0, s>>>(b->ctl.p, b->tidx.p, b->vc.p, b->keys.p);
        VRX_HIP(hipGetLastError());
        VRX_HIP(bc_sort_keys(b, n_tied));
        vrx_barcode_median<<<1, 1, 0, s>>>(b->ctl.p, b->sorted.p, b->scal.p);
        vrx_barcode_flag_ge<<<t_blk, VRX_BC_BLOCK, 0, s>>>(b->ctl.p, b->keys.p, b->scal.p, b->flag2.p);
        VRX_HIP(hipGetLastError());
        VRX_HIP(bc_select_kept(b, n_tied));
        VRX_HIP(hipEventRecord(b->ev[4], s));
        int32_t kept = 0;
        VRX_HIP(hipMemcpyAsync(&kept, b->ctl.p + VRX_BC_KEPT, sizeof kept, hipMemcpyDeviceToHost, s));
        VRX_HIP(hipStreamSynchronize(s));
        VRX_TRY(b->ms(3, 4, &t));
        if (ms2) ms2[1] = ms_rest + t;
        n_kept = kept;
    }
    counts3[1] = n_kept;
    b->n_kept = n_kept;
    b->have_round = true;
    return VRX_OK;
}

extern "C" int vrx_barcode_pick(vrx_barcode* b, int64_t r, int64_t* index_out, double* entropy_out) {
    VRX_REQUIRE(b && index_out && entropy_out, "vrx_barcode_pick: null argument");
    VRX_REQUIRE(b->have_round, "vrx_barcode_pick: no finished round");
    VRX_REQUIRE(r >= 0 && r < b->n_kept, "vrx_barcode_pick: r = %lld is not one of the %lld survivors", (long long)r,
                (long long)b->n_kept);
    VRX_TRY(b->use());
    hipStream_t s = b->stream;
    int32_t idx = -1;
    VRX_HIP(hipMemcpyAsync(&idx, (b->has_vc ? b->kidx.p : b->tidx.p) + r, sizeof idx, hipMemcpyDeviceToHost, s));
    VRX_HIP(hipStreamSynchronize(s));
    VRX_REQUIRE(idx >= 0 && idx < b->N, "vrx_barcode_pick: the survivor list is corrupt");
    VRX_HIP(hipMemcpyAsync(entropy_out, b->ent.p + idx, sizeof(double), hipMemcpyDeviceToHost, s));
    VRX_HIP(hipStreamSynchronize(s));
    *index_out = idx;
    return VRX_OK;
}

extern "C" int vrx_barcode_entropies(vrx_barcode* b, double* out) {
    VRX_REQUIRE(b && out, "vrx_barcode_entropies: null argument");
    VRX_REQUIRE(b->have_round, "vrx_barcode_entropies: no finished round");
    VRX_TRY(b->use());
    VRX_HIP(hipMemcpyAsync(out, b->ent.p, (size_t)b->N * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    VRX_HIP(hipStreamSynchronize(b->stream));
    return VRX_OK;
}
