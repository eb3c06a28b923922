// Pooling cell columns: the vrx_pool_* entries of include/vireo_hip.h on the kernels of vrx_pool.h.  A handle owns
// its stream, events and buffers and keeps the source columns resident, so several plans can run on one upload;
// nothing here touches a vrx_problem or a vrx_model.
#include <algorithm>
#include <climits>

#include "vrx_handle.h"
#include "vrx_pool.h"

struct vrx_pool : VrxQueue {  // ev: 0, 1 bracket the count pass and its scan, 2, 3 the emit pass
    int64_t n_var = 0, n_src = 0, n_pool = -1, total = 0;
    std::vector<int64_t> colptr;  // host copy: the lengths order the columns of a plan
    DevBuf<int64_t> d_colptr, len, out, blk;
    DevBuf<int32_t> row, ad, dp, cols, src0, src1, orow, oad, odp, bad;
};

extern "C" int32_t vrx_pool_wave_limit(void) { return VRX_POOL_WAVE_LIMIT; }
extern "C" int32_t vrx_pool_scan_block(void) { return VRX_POOL_SCAN_BLOCK; }

extern "C" void vrx_pool_destroy(vrx_pool* h) { vrx_destroy(h); }

static const int64_t VRX_POOL_MAX = ((int64_t)1 << 31) - 1024;

extern "C" int vrx_pool_create(int device, int64_t n_var, int64_t n_src, const int64_t* colptr, const int32_t* rowidx,
                               const int32_t* ad, const int32_t* dp, vrx_pool** out) {
    VRX_REQUIRE(colptr && out, "vrx_pool_create: null argument");
    VRX_REQUIRE(n_var >= 0 && n_var < VRX_POOL_MAX && n_src >= 0 && n_src < VRX_POOL_MAX,
                "vrx_pool_create: n_var and n_src must lie in [0, 2^31 - 1024)");
    const int64_t nnz = colptr[n_src];
    VRX_REQUIRE(colptr[0] == 0 && nnz >= 0, "vrx_pool_create: colptr must start at 0");
    VRX_REQUIRE(nnz == 0 || (rowidx && ad && dp), "vrx_pool_create: entries need rowidx, ad and dp");
    for (int64_t c = 0; c < n_src; ++c) {
        VRX_REQUIRE(colptr[c] <= colptr[c + 1] && colptr[c + 1] <= nnz,
                    "vrx_pool_create: colptr not monotone at column %lld", (long long)c);
        int64_t prev = -1;
        for (int64_t e = colptr[c]; e < colptr[c + 1]; ++e) {
            VRX_REQUIRE(rowidx[e] > prev && rowidx[e] < n_var,
                        "vrx_pool_create: row indices of column %lld not strictly increasing / out of range",
                        (long long)c);
            VRX_REQUIRE(ad[e] >= 0 && dp[e] >= 0, "vrx_pool_create: negative count in column %lld", (long long)c);
            prev = rowidx[e];
        }
    }
    VrxOwned<vrx_pool> h(new vrx_pool());
    VRX_TRY(h->open("vrx_pool_create", device, 4));
    h->n_var = n_var;
    h->n_src = n_src;
    h->colptr.assign(colptr, colptr + n_src + 1);
    hipStream_t s = h->stream;
    VRX_HIP(h->d_colptr.upload(colptr, (size_t)n_src + 1, s));
    VRX_HIP(h->row.upload(rowidx, (size_t)nnz, s));
    VRX_HIP(h->ad.upload(ad, (size_t)nnz, s));
    VRX_HIP(h->dp.upload(dp, (size_t)nnz, s));
    VRX_HIP(h->bad.alloc(1));
    VRX_HIP(hipStreamSynchronize(s));  // (the caller's arrays may die at return)
    *out = h.release();
    return VRX_OK;
}

extern "C" int vrx_pool_run(vrx_pool* h, int64_t n_pool, const int32_t* src0, const int32_t* src1, int64_t* colptr_out,
                            int64_t* bad, double* ms) {
    VRX_REQUIRE(h && colptr_out && bad, "vrx_pool_run: null argument");
    VRX_REQUIRE(n_pool >= 0 && n_pool < VRX_POOL_MAX, "vrx_pool_run: 0 <= n_pool < 2^31 - 1024");
    VRX_REQUIRE(n_pool == 0 || (src0 && src1), "vrx_pool_run: pooled columns need src0 and src1");
    h->n_pool = -1;
    h->total = 0;
    *bad = -1;
    if (ms) *ms = 0.0;
    // workgroup columns first, then wavefront columns, each in plan order
    const size_t P = (size_t)n_pool;
    std::vector<int32_t> cols(P);
    int64_t n_long = 0;
    for (int64_t j = 0; j < n_pool; ++j) {
        VRX_REQUIRE(src0[j] >= 0 && src0[j] < h->n_src && src1[j] >= -1 && src1[j] < h->n_src,
                    "vrx_pool_run: pooled column %lld names sources %d and %d of %lld", (long long)j, (int)src0[j],
                    (int)src1[j], (long long)h->n_src);
        int64_t work = h->colptr[src0[j] + 1] - h->colptr[src0[j]];
        if (src1[j] >= 0) work += h->colptr[src1[j] + 1] - h->colptr[src1[j]];
        if (work > VRX_POOL_WAVE_LIMIT) cols[(size_t)n_long++] = (int32_t)j;
    }
    {
        int64_t at = n_long;
        for (int64_t j = 0, k = 0; j < n_pool; ++j) {
            if (k < n_long && cols[(size_t)k] == j)
                ++k;
            else
                cols[(size_t)at++] = (int32_t)j;
        }
    }
    // a launch holds fewer than 2^32 threads: 2^24 - 1 workgroups of 256, one per long column or four short ones
    const int64_t n_wg = n_long + (n_pool - n_long + VRX_POOL_WAVES - 1) / VRX_POOL_WAVES;
    VRX_REQUIRE(n_wg < ((int64_t)1 << 32) / VRX_POOL_BLOCK,
                "vrx_pool_run: %lld pooled columns (%lld above the wavefront limit) need %lld workgroups, "
                "a launch takes fewer than %lld",
                (long long)n_pool, (long long)n_long, (long long)n_wg, (long long)(((int64_t)1 << 32) / VRX_POOL_BLOCK));
    colptr_out[0] = 0;
    if (n_pool == 0) {
        h->n_pool = 0;
        return VRX_OK;
    }
    VRX_TRY(h->use());
    hipStream_t s = h->stream;
    VRX_HIP(h->cols.upload(cols.data(), P, s));
    VRX_HIP(h->src0.upload(src0, P, s));
    VRX_HIP(h->src1.upload(src1, P, s));
    VRX_HIP(h->len.alloc(P));
    VRX_HIP(h->out.alloc(P + 1));
    const int64_t n_blk = (n_pool + VRX_POOL_SCAN_BLOCK - 1) / VRX_POOL_SCAN_BLOCK;
    VRX_HIP(h->blk.alloc((size_t)n_blk));
    const int32_t none = INT32_MAX;
    VRX_HIP(hipMemcpyAsync(h->bad.p, &none, sizeof none, hipMemcpyHostToDevice, s));
    VrxPoolArgs g;
    g.n_long = n_long;
    g.n_short = n_pool - n_long;
    g.cols = h->cols.p;
    g.src0 = h->src0.p;
    g.src1 = h->src1.p;
    g.colptr = h->d_colptr.p;
    g.row = h->row.p;
    g.ad = h->ad.p;
    g.dp = h->dp.p;
    g.len = h->len.p;
    g.out = h->out.p;
    g.orow = g.oad = g.odp = nullptr;
    g.bad = h->bad.p;
    const unsigned grid = (unsigned)n_wg;
    VRX_HIP(hipEventRecord(h->ev[0], s));
    vrx_pool_pass<false><<<grid, VRX_POOL_BLOCK, 0, s>>>(g);
    VRX_HIP(hipGetLastError());
    vrx_pool_scan_local<<<(unsigned)n_blk, VRX_POOL_BLOCK, 0, s>>>(n_pool, h->len.p, h->out.p, h->blk.p);
    VRX_HIP(hipGetLastError());
    vrx_pool_scan_blocks<<<1, VRX_POOL_BLOCK, 0, s>>>(n_blk, h->blk.p, h->out.p + n_pool);
    VRX_HIP(hipGetLastError());
    vrx_pool_scan_add<<<(unsigned)((n_pool + VRX_POOL_BLOCK - 1) / VRX_POOL_BLOCK), VRX_POOL_BLOCK, 0, s>>>(
        n_pool, h->out.p, h->blk.p);
    VRX_HIP(hipGetLastError());
    VRX_HIP(hipEventRecord(h->ev[1], s));
    VRX_HIP(hipMemcpyAsync(colptr_out, h->out.p, (P + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    VRX_HIP(hipStreamSynchronize(s));
    const int64_t total = colptr_out[n_pool];
    {   // what the emit pass will index by: checked before anything is written through it
        int64_t most = 0;
        for (int64_t j = 0; j < n_pool; ++j) {
            int64_t work = h->colptr[src0[j] + 1] - h->colptr[src0[j]];
            if (src1[j] >= 0) work += h->colptr[src1[j] + 1] - h->colptr[src1[j]];
            const int64_t len = colptr_out[j + 1] - colptr_out[j];
            VRX_REQUIRE(len >= 0 && len <= work && (src1[j] >= 0 || len == work),
                        "vrx_pool_run: pooled column %lld came out with %lld entries of %lld", (long long)j,
                        (long long)len, (long long)work);
            most += work;
        }
        VRX_REQUIRE(total >= 0 && total <= most, "vrx_pool_run: %lld entries from %lld", (long long)total,
                    (long long)most);
    }
    VRX_HIP(h->orow.alloc((size_t)total));
    VRX_HIP(h->oad.alloc((size_t)total));
    VRX_HIP(h->odp.alloc((size_t)total));
    double t0 = 0.0, t1 = 0.0;
    if (total > 0) {
        g.orow = h->orow.p;
        g.oad = h->oad.p;
        g.odp = h->odp.p;
        VRX_HIP(hipEventRecord(h->ev[2], s));
        vrx_pool_pass<true><<<grid, VRX_POOL_BLOCK, 0, s>>>(g);
        VRX_HIP(hipGetLastError());
        VRX_HIP(hipEventRecord(h->ev[3], s));
    }
    int32_t first = INT32_MAX;
    VRX_HIP(hipMemcpyAsync(&first, h->bad.p, sizeof first, hipMemcpyDeviceToHost, s));
    VRX_HIP(hipStreamSynchronize(s));
    VRX_TRY(h->ms(0, 1, &t0));
    if (total > 0) VRX_TRY(h->ms(2, 3, &t1));
    if (ms) *ms = t0 + t1;
    if (first != INT32_MAX) *bad = first;
    h->n_pool = n_pool;
    h->total = total;
    return VRX_OK;
}

extern "C" int vrx_pool_read(vrx_pool* h, int32_t* rowidx, int32_t* ad, int32_t* dp) {
    VRX_REQUIRE(h, "vrx_pool_read: null handle");
    VRX_REQUIRE(h->n_pool >= 0, "vrx_pool_read: no vrx_pool_run before it");
    if (h->total == 0) return VRX_OK;
    VRX_REQUIRE(rowidx && ad && dp, "vrx_pool_read: null output");
    VRX_TRY(h->use());
    const size_t n = (size_t)h->total * sizeof(int32_t);
    VRX_HIP(hipMemcpyAsync(rowidx, h->orow.p, n, hipMemcpyDeviceToHost, h->stream));
    VRX_HIP(hipMemcpyAsync(ad, h->oad.p, n, hipMemcpyDeviceToHost, h->stream));
    VRX_HIP(hipMemcpyAsync(dp, h->odp.p, n, hipMemcpyDeviceToHost, h->stream));
    VRX_HIP(hipStreamSynchronize(h->stream));
    return VRX_OK;
}
