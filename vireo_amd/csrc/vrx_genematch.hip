// SNP-to-gene matching and gene-level counts: the vrx_genematch_* and vrx_genecount_* entries of
// include/vireo_hip.h on the kernels of vrx_genematch.h.  A handle owns its stream, events and buffers; nothing
// here touches a vrx_problem or a vrx_model.
#include <algorithm>

#include <hipcub/hipcub.hpp>

#include "vrx_handle.h"
#include "vrx_genematch.h"

struct vrx_genematch : VrxQueue {  // ev: 0, 1 bracket the kernels of a call
    int64_t n_chrom = 0, n_gene = 0, n_snp = 0, total = -1;
    DevBuf<int32_t> chrom_ptr, gene, grow;  // gene: (start, stop) pairs
    DevBuf<int32_t> code, pos, perm, gap_m1, flag, thr, first, rows;
    DevBuf<uint8_t> single, multi, tmp;
    DevBuf<int64_t> count, offset;
    VrxGmArgs args;
};

extern "C" int32_t vrx_genematch_tile(void) { return VRX_GM_TILE; }
extern "C" int32_t vrx_genematch_block(void) { return VRX_GM_BLOCK; }

extern "C" void vrx_genematch_destroy(vrx_genematch* h) { vrx_destroy(h); }

static const int64_t VRX_GM_MAX = ((int64_t)1 << 31) - 1024;

extern "C" int vrx_genematch_create(int device, int64_t n_chrom, int64_t n_gene, const int64_t* chrom_ptr,
                                    const int32_t* start, const int32_t* stop, const int32_t* row,
                                    vrx_genematch** out) {
    VRX_REQUIRE(chrom_ptr && out, "vrx_genematch_create: null argument");
    VRX_REQUIRE(n_chrom >= 0 && n_chrom < VRX_GM_MAX, "vrx_genematch_create: 0 <= n_chrom < 2^31 - 1024");
    VRX_REQUIRE(n_gene >= 0 && n_gene < VRX_GM_MAX, "vrx_genematch_create: 0 <= n_gene < 2^31 - 1024");
    VRX_REQUIRE(n_gene == 0 || (start && stop && row), "vrx_genematch_create: genes need start, stop and row");
    VRX_REQUIRE(chrom_ptr[0] == 0 && chrom_ptr[n_chrom] == n_gene,
                "vrx_genematch_create: chrom_ptr must run from 0 to n_gene");
    for (int64_t c = 0; c < n_chrom; ++c)
        VRX_REQUIRE(chrom_ptr[c] <= chrom_ptr[c + 1], "vrx_genematch_create: chrom_ptr decreases at code %lld",
                    (long long)c);
    for (int64_t i = 0; i < n_gene; ++i)
        VRX_REQUIRE(start[i] >= 0 && stop[i] >= 0 && row[i] >= 0,
                    "vrx_genematch_create: gene %lld has a negative start, stop or row", (long long)i);
    VrxOwned<vrx_genematch> h(new vrx_genematch());
    VRX_TRY(h->open("vrx_genematch_create", device, 2));
    h->n_chrom = n_chrom;
    h->n_gene = n_gene;
    std::vector<int32_t> cp((size_t)n_chrom + 1), pairs((size_t)n_gene * 2);
    for (int64_t c = 0; c <= n_chrom; ++c) cp[(size_t)c] = (int32_t)chrom_ptr[c];
    for (int64_t i = 0; i < n_gene; ++i) {
        pairs[(size_t)i * 2] = start[i];
        pairs[(size_t)i * 2 + 1] = stop[i];
    }
    hipStream_t s = h->stream;
    VRX_HIP(h->chrom_ptr.upload(cp.data(), cp.size(), s));
    VRX_HIP(h->gene.upload(pairs.data(), pairs.size(), s));
    VRX_HIP(h->grow.upload(row, (size_t)n_gene, s));
    VRX_HIP(hipStreamSynchronize(s));  // (the host vectors die at return)
    *out = h.release();
    return VRX_OK;
}

extern "C" int vrx_genematch_match(vrx_genematch* h, int64_t n_snp, const int32_t* code, const int32_t* pos,
                                   const int32_t* perm, int32_t n_gap, const int32_t* gap_m1, const uint8_t* single,
                                   int32_t* flag, int64_t* count, double* ms) {
    VRX_REQUIRE(h, "vrx_genematch_match: null handle");
    VRX_REQUIRE(n_snp >= 0 && n_snp < VRX_GM_MAX, "vrx_genematch_match: 0 <= n_snp < 2^31 - 1024");
    VRX_REQUIRE(n_gap >= 1 && gap_m1 && single, "vrx_genematch_match: at least one gap");
    VRX_REQUIRE(n_snp == 0 || (code && pos && perm && flag && count), "vrx_genematch_match: null argument");
    h->total = -1;
    h->n_snp = 0;
    if (ms) *ms = 0.0;
    {   // sorted codes inside the table, positions non-negative, perm a permutation
        std::vector<uint8_t> seen((size_t)n_snp, 0);
        for (int64_t j = 0; j < n_snp; ++j) {
            VRX_REQUIRE(code[j] >= 0 && code[j] < h->n_chrom, "vrx_genematch_match: SNP %lld has code %d of %lld",
                        (long long)j, (int)code[j], (long long)h->n_chrom);
            VRX_REQUIRE(j == 0 || code[j - 1] <= code[j], "vrx_genematch_match: codes not sorted at %lld", (long long)j);
            VRX_REQUIRE(pos[j] >= 0, "vrx_genematch_match: SNP %lld has a negative position", (long long)j);
            VRX_REQUIRE(perm[j] >= 0 && perm[j] < n_snp && !seen[(size_t)perm[j]],
                        "vrx_genematch_match: perm is not a permutation at %lld", (long long)j);
            seen[(size_t)perm[j]] = 1;
        }
    }
    h->n_snp = n_snp;
    if (n_snp == 0) {
        h->total = 0;
        return VRX_OK;
    }
    VRX_TRY(h->use());
    hipStream_t s = h->stream;
    const size_t N = (size_t)n_snp;
    VRX_HIP(h->code.upload(code, N, s));
    VRX_HIP(h->pos.upload(pos, N, s));
    VRX_HIP(h->perm.upload(perm, N, s));
    VRX_HIP(h->gap_m1.upload(gap_m1, (size_t)n_gap, s));
    VRX_HIP(h->single.upload(single, (size_t)n_gap, s));
    VRX_HIP(h->flag.alloc(N));
    VRX_HIP(h->count.alloc(N));
    VRX_HIP(h->offset.alloc(N));
    VRX_HIP(h->thr.alloc(N));
    VRX_HIP(h->first.alloc(N));
    VRX_HIP(h->multi.alloc(N));
    auto scan_counts = VRX_CUB_CALL(DeviceScan::ExclusiveSum, h->count.p, h->offset.p, N, s);
    VRX_HIP(vrx_cub(h->tmp, scan_counts, VRX_CUB_SIZE));  // (ahead of the timed region)
    VrxGmArgs& g = h->args;
    g.n_snp = n_snp;
    g.code = h->code.p;
    g.pos = h->pos.p;
    g.perm = h->perm.p;
    g.chrom_ptr = h->chrom_ptr.p;
    g.gene = reinterpret_cast<const int2*>(h->gene.p);
    g.grow = h->grow.p;
    g.n_gap = n_gap;
    g.gap_m1 = h->gap_m1.p;
    g.single = h->single.p;
    g.flag = h->flag.p;
    g.count = h->count.p;
    g.offset = h->offset.p;
    g.thr = h->thr.p;
    g.first = h->first.p;
    g.multi = h->multi.p;
    g.rows = nullptr;
    const unsigned n_blk = (unsigned)((n_snp + VRX_GM_BLOCK - 1) / VRX_GM_BLOCK);
    VRX_HIP(hipEventRecord(h->ev[0], s));
    vrx_gm_pass1<<<n_blk, VRX_GM_BLOCK, 0, s>>>(g);
    VRX_HIP(hipGetLastError());
    VRX_HIP(vrx_cub(h->tmp, scan_counts, VRX_CUB_SIZED));
    VRX_HIP(hipEventRecord(h->ev[1], s));
    VRX_HIP(hipMemcpyAsync(flag, h->flag.p, N * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    VRX_HIP(hipMemcpyAsync(count, h->count.p, N * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    VRX_HIP(hipStreamSynchronize(s));
    int64_t total = 0;
    for (size_t i = 0; i < N; ++i) total += count[i];
    h->total = total;
    return h->ms(0, 1, ms);
}

extern "C" int vrx_genematch_lists(vrx_genematch* h, int64_t total, int32_t* rows, double* ms) {
    VRX_REQUIRE(h, "vrx_genematch_lists: null handle");
    VRX_REQUIRE(h->total >= 0, "vrx_genematch_lists: no vrx_genematch_match before it");
    VRX_REQUIRE(total == h->total, "vrx_genematch_lists: total = %lld, the match counted %lld", (long long)total,
                (long long)h->total);
    VRX_REQUIRE(total == 0 || rows, "vrx_genematch_lists: null output");
    if (ms) *ms = 0.0;
    if (total == 0) return VRX_OK;
    VRX_TRY(h->use());
    hipStream_t s = h->stream;
    VRX_HIP(h->rows.alloc((size_t)total));
    h->args.rows = h->rows.p;
    const unsigned n_blk = (unsigned)((h->n_snp + VRX_GM_BLOCK - 1) / VRX_GM_BLOCK);
    VRX_HIP(hipEventRecord(h->ev[0], s));
    vrx_gm_pass2<<<n_blk, VRX_GM_BLOCK, 0, s>>>(h->args);
    VRX_HIP(hipGetLastError());
    VRX_HIP(hipEventRecord(h->ev[1], s));
    VRX_HIP(hipMemcpyAsync(rows, h->rows.p, (size_t)total * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    VRX_HIP(hipStreamSynchronize(s));
    return h->ms(0, 1, ms);
}

// ---- gene counts ----------------------------------------------------------------------------------

struct vrx_genecount : VrxQueue {  // ev: 0, 1 bracket the kernels of create
    int64_t n_out = 0;
    DevBuf<uint64_t> out_key;
    DevBuf<int64_t> out_ad, out_dp;
};

extern "C" void vrx_genecount_destroy(vrx_genecount* h) { vrx_destroy(h); }

static unsigned vrx_gc_blocks(int64_t n) { return (unsigned)((n + VRX_GC_BLOCK - 1) / VRX_GC_BLOCK); }

extern "C" int vrx_genecount_create(int device, int64_t n_var, int64_t n_cell, int64_t n_gene, const int64_t* colptr,
                                    const int32_t* rowidx, const int32_t* ad, const int32_t* dp, const int64_t* gptr,
                                    const int32_t* gid, vrx_genecount** out, int64_t* n_out, double* ms) {
    VRX_REQUIRE(colptr && gptr && out && n_out, "vrx_genecount_create: null argument");
    VRX_REQUIRE(n_var >= 0 && n_var < VRX_GM_MAX && n_cell >= 0 && n_cell < VRX_GM_MAX && n_gene >= 0 &&
                    n_gene < VRX_GM_MAX,
                "vrx_genecount_create: n_var, n_cell and n_gene must lie in [0, 2^31 - 1024)");
    const int64_t nnz = colptr[n_cell], n_map = gptr[n_var];
    VRX_REQUIRE(colptr[0] == 0 && nnz >= 0 && gptr[0] == 0 && n_map >= 0,
                "vrx_genecount_create: colptr and gptr must start at 0");
    VRX_REQUIRE(nnz == 0 || (rowidx && ad && dp), "vrx_genecount_create: entries need rowidx, ad and dp");
    VRX_REQUIRE(n_map == 0 || gid, "vrx_genecount_create: the map needs gid");
    for (int64_t c = 0; c < n_cell; ++c)
        VRX_REQUIRE(colptr[c] <= colptr[c + 1], "vrx_genecount_create: colptr decreases at column %lld", (long long)c);
    for (int64_t v = 0; v < n_var; ++v)
        VRX_REQUIRE(gptr[v] <= gptr[v + 1], "vrx_genecount_create: gptr decreases at variant %lld", (long long)v);
    for (int64_t q = 0; q < n_map; ++q)
        VRX_REQUIRE(gid[q] >= 0 && gid[q] < n_gene, "vrx_genecount_create: gid[%lld] = %d of %lld genes", (long long)q,
                    (int)gid[q], (long long)n_gene);
    int64_t total = 0;
    for (int64_t e = 0; e < nnz; ++e) {
        VRX_REQUIRE(rowidx[e] >= 0 && rowidx[e] < n_var && ad[e] >= 0 && dp[e] >= 0,
                    "vrx_genecount_create: entry %lld has row %d, ad %d, dp %d", (long long)e, (int)rowidx[e],
                    (int)ad[e], (int)dp[e]);
        total += gptr[rowidx[e] + 1] - gptr[rowidx[e]];
        VRX_REQUIRE(total < VRX_GM_MAX, "vrx_genecount_create: 2^31 - 1024 (entry, gene) pairs or more");
    }
    if (int e = vrx_use_device("vrx_genecount_create", device)) return e;
    VrxOwned<vrx_genecount> h(new vrx_genecount());
    *n_out = 0;
    if (ms) *ms = 0.0;
    if (total == 0) {  // nothing to count: a handle without a stream
        *out = h.release();
        return VRX_OK;
    }
    VRX_TRY(h->open("vrx_genecount_create", device, 2));
    hipStream_t s = h->stream;
    const size_t E = (size_t)nnz, T = (size_t)total;
    DevBuf<int64_t> d_colptr, d_gptr, cnt, off;
    DevBuf<int32_t> d_row, d_ad, d_dp, d_gid, head, seg;
    DevBuf<uint64_t> key, val, key2, val2;
    DevBuf<uint8_t> tmp;
    VRX_HIP(d_colptr.upload(colptr, (size_t)n_cell + 1, s));
    VRX_HIP(d_gptr.upload(gptr, (size_t)n_var + 1, s));
    VRX_HIP(d_row.upload(rowidx, E, s));
    VRX_HIP(d_ad.upload(ad, E, s));
    VRX_HIP(d_dp.upload(dp, E, s));
    VRX_HIP(d_gid.upload(gid, (size_t)n_map, s));
    VRX_HIP(cnt.alloc(E));
    VRX_HIP(off.alloc(E));
    VRX_HIP(key.alloc(T));
    VRX_HIP(val.alloc(T));
    VRX_HIP(key2.alloc(T));
    VRX_HIP(val2.alloc(T));
    VRX_HIP(head.alloc(T));
    VRX_HIP(seg.alloc(T));
    int bits = 1;  // of the largest key, n_cell n_gene - 1 < 2^62
    while (bits < 64 && ((uint64_t)n_cell * (uint64_t)n_gene - 1) >> bits) ++bits;
    auto scan_counts = VRX_CUB_CALL(DeviceScan::ExclusiveSum, cnt.p, off.p, E, s);
    auto sort_pairs = VRX_CUB_CALL(DeviceRadixSort::SortPairs, key.p, key2.p, val.p, val2.p, T, 0, bits, s);
    auto scan_heads = VRX_CUB_CALL(DeviceScan::ExclusiveSum, head.p, seg.p, T, s);
    VRX_HIP(vrx_cub(tmp, scan_counts, VRX_CUB_SIZE));  // (all three ahead of the timed region)
    VRX_HIP(vrx_cub(tmp, sort_pairs, VRX_CUB_SIZE));
    VRX_HIP(vrx_cub(tmp, scan_heads, VRX_CUB_SIZE));
    VRX_HIP(hipEventRecord(h->ev[0], s));
    vrx_gc_count<<<vrx_gc_blocks(nnz), VRX_GC_BLOCK, 0, s>>>(nnz, d_row.p, d_gptr.p, cnt.p);
    VRX_HIP(hipGetLastError());
    VRX_HIP(vrx_cub(tmp, scan_counts, VRX_CUB_SIZED));
    vrx_gc_emit<<<vrx_gc_blocks(nnz), VRX_GC_BLOCK, 0, s>>>(nnz, n_cell, n_gene, d_colptr.p, d_row.p, d_ad.p, d_dp.p,
                                                            d_gptr.p, d_gid.p, off.p, key.p, val.p);
    VRX_HIP(hipGetLastError());
    VRX_HIP(vrx_cub(tmp, sort_pairs, VRX_CUB_SIZED));
    vrx_gc_heads<<<vrx_gc_blocks(total), VRX_GC_BLOCK, 0, s>>>(total, key2.p, head.p);
    VRX_HIP(hipGetLastError());
    VRX_HIP(vrx_cub(tmp, scan_heads, VRX_CUB_SIZED));
    int32_t last[2] = {0, 0};
    VRX_HIP(hipMemcpyAsync(&last[0], seg.p + (T - 1), sizeof(int32_t), hipMemcpyDeviceToHost, s));
    VRX_HIP(hipMemcpyAsync(&last[1], head.p + (T - 1), sizeof(int32_t), hipMemcpyDeviceToHost, s));
    VRX_HIP(hipStreamSynchronize(s));
    const int64_t n_seg = (int64_t)last[0] + last[1];
    VRX_REQUIRE(n_seg >= 1 && n_seg <= total, "vrx_genecount_create: %lld runs of %lld pairs", (long long)n_seg,
                (long long)total);
    VRX_HIP(h->out_key.alloc((size_t)n_seg));
    VRX_HIP(h->out_ad.alloc((size_t)n_seg));
    VRX_HIP(h->out_dp.alloc((size_t)n_seg));
    vrx_gc_reduce<<<vrx_gc_blocks(total), VRX_GC_BLOCK, 0, s>>>(total, key2.p, val2.p, head.p, seg.p, h->out_key.p,
                                                                h->out_ad.p, h->out_dp.p);
    VRX_HIP(hipGetLastError());
    VRX_HIP(hipEventRecord(h->ev[1], s));
    VRX_HIP(hipStreamSynchronize(s));
    VRX_TRY(h->ms(0, 1, ms));
    h->n_out = n_seg;
    *n_out = n_seg;
    *out = h.release();
    return VRX_OK;
}

extern "C" int vrx_genecount_read(vrx_genecount* h, int64_t* key, int64_t* ad, int64_t* dp) {
    VRX_REQUIRE(h, "vrx_genecount_read: null handle");
    if (h->n_out == 0) return VRX_OK;
    VRX_REQUIRE(key && ad && dp, "vrx_genecount_read: null output");
    VRX_TRY(h->use());
    const size_t n = (size_t)h->n_out;
    VRX_HIP(hipMemcpyAsync(key, h->out_key.p, n * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    VRX_HIP(hipMemcpyAsync(ad, h->out_ad.p, n * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    VRX_HIP(hipMemcpyAsync(dp, h->out_dp.p, n * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    VRX_HIP(hipStreamSynchronize(h->stream));
    return VRX_OK;
}
