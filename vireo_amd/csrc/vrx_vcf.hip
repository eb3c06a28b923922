// VCF text on the device: the vrx_vcf_* entries of include/vireo_hip.h on the kernels of vrx_vcf.h (donor VCFs) and
// the vrx_cellvcf_* entries on those of vrx_cellvcf.h (cell VCFs); in front of both, the vrx_bgzf_* entries inflate the
// file's BGZF members with the decoder of vrx_bgzf.h.
// A handle owns its stream and buffers; nothing here touches a vrx_problem or a vrx_model.
#include <algorithm>
#include <chrono>

#include <hipcub/hipcub.hpp>

#include "vrx_handle.h"
#include "vrx_bgzf.h"
#include "vrx_cellvcf.h"
#include "vrx_vcf.h"

namespace {
constexpr size_t kRowBatchBytes = (size_t)128 << 20;  // rows of one vrx_vcf_rows launch (device staging)

double seconds_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}
}  // namespace

// The text front end of both readers: a slab of VCF text on the device and where its lines start.
struct VcfText {
    DevBuf<uint8_t> text, flag, tmp;  // tmp: the temporary storage of every hipCUB call of the handle
    DevBuf<uint32_t> lstart, ctl;     // ctl: 0 lines of the slab, 1 status, 2 and 3 the reader's own counts
    int create(hipStream_t s) {
        VRX_HIP(ctl.alloc(4));
        VRX_HIP(hipMemsetAsync(ctl.p, 0, 4 * sizeof(uint32_t), s));
        return VRX_OK;
    }
    int lines(hipStream_t s, const char* host, size_t n, uint32_t status, uint32_t out_ctl[4], double* seconds,
              std::chrono::steady_clock::time_point* t0);
};

struct vrx_vcf : VrxQueue {
    int32_t tag = 0, n_sample = 0, biallelic_only = 1, mode = -1;
    bool matching = false;
    int64_t n_ids = 0;
    uint32_t table_status = 0;
    // cell table
    DevBuf<uint8_t> id_bytes;
    DevBuf<int64_t> id_off;
    DevBuf<uint64_t> hash;
    DevBuf<int32_t> idx, claim;
    DevBuf<double> pl_table;
    // slab
    uint32_t n = 0, n_lines = 0;
    int64_t n_matched = 0, line_base = 0, kept_total = 0;
    VcfText in;  // its ctl: 2 matched, 3 tagged
    DevBuf<uint8_t> match;
    DevBuf<int32_t> kept, tagged, ord, mlist;
    DevBuf<VrxVcfLine> rec;
    // rows
    DevBuf<double> gpb;
    DevBuf<int64_t> slot, ordinal, span;
    DevBuf<int32_t> rflag;
};

extern "C" int32_t vrx_vcf_chunk(void) { return VRX_VCF_CHUNK; }

extern "C" void vrx_vcf_destroy(vrx_vcf* h) { vrx_destroy(h); }

extern "C" int vrx_vcf_create(int device, int32_t tag, int32_t n_sample, int32_t biallelic_only, int64_t n_ids,
                              const char* id_bytes, const int64_t* id_off, const double* pl_table, vrx_vcf** out) {
    VRX_REQUIRE(out, "vrx_vcf_create: null argument");
    VRX_REQUIRE(tag == VRX_VCF_GT || tag == VRX_VCF_PL || tag == VRX_VCF_GP, "vrx_vcf_create: tag must be 0 (GT), 1 (PL) or 2 (GP)");
    VRX_REQUIRE(n_sample >= 1 && n_sample < (1 << 24), "vrx_vcf_create: 1 <= n_sample < 2^24");
    VRX_REQUIRE(tag != VRX_VCF_PL || pl_table, "vrx_vcf_create: PL needs its table");
    VRX_REQUIRE(n_ids < ((int64_t)1 << 31) - 4, "vrx_vcf_create: n_ids < 2^31 - 4");
    if (n_ids >= 0) {
        VRX_REQUIRE(id_off && id_off[0] == 0, "vrx_vcf_create: id_off must start at 0");
        for (int64_t i = 0; i < n_ids; ++i)
            VRX_REQUIRE(id_off[i] <= id_off[i + 1], "vrx_vcf_create: id_off decreases at id %lld", (long long)i);
        VRX_REQUIRE(id_off[n_ids] == 0 || id_bytes, "vrx_vcf_create: ids need their bytes");
    }
    VrxOwned<vrx_vcf> h(new vrx_vcf());
    VRX_TRY(h->open("vrx_vcf_create", device, 0));
    h->tag = tag;
    h->n_sample = n_sample;
    h->biallelic_only = biallelic_only != 0;
    h->matching = n_ids >= 0;
    h->n_ids = std::max<int64_t>(n_ids, 0);
    hipStream_t s = h->stream;
    VRX_TRY(h->in.create(s));
    if (pl_table) VRX_HIP(h->pl_table.upload(pl_table, VRX_VCF_PL_MAX + 1, s));
    const size_t N = (size_t)h->n_ids;
    if (N > 0) {
        DevBuf<uint64_t> hash_in;
        DevBuf<int32_t> idx_in;
        VRX_HIP(h->id_bytes.upload(reinterpret_cast<const uint8_t*>(id_bytes), (size_t)id_off[N], s));
        VRX_HIP(h->id_off.upload(id_off, N + 1, s));
        VRX_HIP(hash_in.alloc(N));
        VRX_HIP(idx_in.alloc(N));
        VRX_HIP(h->hash.alloc(N));
        VRX_HIP(h->idx.alloc(N));
        VRX_HIP(h->claim.alloc(N));
        const unsigned n_blk = (unsigned)((N + VRX_VCF_BLOCK - 1) / VRX_VCF_BLOCK);
        vrx_vcf_hash_ids<<<n_blk, VRX_VCF_BLOCK, 0, s>>>(h->id_bytes.p, h->id_off.p, (int64_t)N, hash_in.p, idx_in.p);
        VRX_HIP(hipGetLastError());
        VRX_HIP(vrx_cub(h->in.tmp, VRX_CUB_CALL(DeviceRadixSort::SortPairs, hash_in.p, h->hash.p, idx_in.p, h->idx.p,
                                                (int)N, 0, 64, s)));
        vrx_vcf_table_check<<<n_blk, VRX_VCF_BLOCK, 0, s>>>(h->id_bytes.p, h->id_off.p, (int64_t)N, h->hash.p, h->idx.p,
                                                            h->in.ctl.p + 1);
        VRX_HIP(hipGetLastError());
        VRX_HIP(hipMemcpyAsync(&h->table_status, h->in.ctl.p + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        VRX_HIP(hipStreamSynchronize(s));  // (the staging buffers die at return)
    }
    VRX_HIP(hipStreamSynchronize(s));
    *out = h.release();
    return VRX_OK;
}

extern "C" int vrx_vcf_begin(vrx_vcf* h, int32_t mode, int32_t* status) {
    VRX_REQUIRE(h && status, "vrx_vcf_begin: null argument");
    VRX_REQUIRE(h->matching ? (mode >= 0 && mode <= 2) : mode == -1,
                "vrx_vcf_begin: mode is 0, 1 or 2 with a cell table and -1 without");
    VRX_TRY(h->use());
    h->mode = mode;
    h->n = h->n_lines = 0;
    h->n_matched = h->line_base = h->kept_total = 0;
    if (h->n_ids > 0) VRX_HIP(hipMemsetAsync(h->claim.p, 0, (size_t)h->n_ids * sizeof(int32_t), h->stream));
    VRX_HIP(hipStreamSynchronize(h->stream));
    *status = (int32_t)h->table_status;
    return VRX_OK;
}

// Uploads the n > 0 bytes (seconds[0]), marks the line starts with the status word seeded by `status`, reads
// the control words back into ctl and, if the status is still 0, compacts the ctl[0] line starts into lstart.
// With a status set nothing more is done and seconds[1] is closed; otherwise *t0 is where seconds[1] began.
int VcfText::lines(hipStream_t s, const char* host, size_t n, uint32_t status, uint32_t out_ctl[4], double* seconds,
                   std::chrono::steady_clock::time_point* t0) {
    const size_t n_pad = (n + VRX_VCF_MARK_BYTES - 1) / VRX_VCF_MARK_BYTES * VRX_VCF_MARK_BYTES;
    *t0 = std::chrono::steady_clock::now();
    VRX_HIP(vrx_reserve(text, n_pad + 2 * VRX_VCF_MARK_BYTES));
    VRX_HIP(vrx_reserve(flag, n_pad + VRX_VCF_MARK_BYTES));
    VRX_HIP(hipMemcpyAsync(text.p, host, n, hipMemcpyHostToDevice, s));
    VRX_HIP(hipStreamSynchronize(s));
    if (seconds) seconds[0] = seconds_since(*t0);
    *t0 = std::chrono::steady_clock::now();
    const uint32_t seed[4] = {0, status, 0, 0};
    VRX_HIP(hipMemcpyAsync(ctl.p, seed, sizeof seed, hipMemcpyHostToDevice, s));
    const size_t per_block = (size_t)VRX_VCF_BLOCK * VRX_VCF_MARK_BYTES;
    vrx_vcf_mark<<<(unsigned)((n + per_block - 1) / per_block), VRX_VCF_BLOCK, 0, s>>>(text.p, (uint32_t)n, flag.p,
                                                                                        ctl.p, ctl.p + 1);
    VRX_HIP(hipGetLastError());
    VRX_HIP(hipMemcpyAsync(out_ctl, ctl.p, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    VRX_HIP(hipStreamSynchronize(s));
    const size_t L = out_ctl[0];
    // a line that load_VCF can index has 8 tabs and a line end, the last one may lack the line end
    if (L * 9 > n + 1) out_ctl[1] |= VRX_VCF_ST_SHORT;
    if (out_ctl[1]) {
        if (seconds) seconds[1] = seconds_since(*t0);
        return VRX_OK;
    }
    VRX_HIP(vrx_reserve(lstart, L));
    VRX_HIP(vrx_cub(tmp, VRX_CUB_CALL(DeviceSelect::Flagged, hipcub::CountingInputIterator<uint32_t>(0), flag.p,
                                      lstart.p, ctl.p + 2, (int)n, s)));
    return VRX_OK;
}

extern "C" int vrx_vcf_slab(vrx_vcf* h, const char* text, int64_t n_bytes, int64_t* info, double* seconds) {
    VRX_REQUIRE(h && info, "vrx_vcf_slab: null argument");
    VRX_REQUIRE(h->mode >= -1 && (h->mode >= 0) == h->matching, "vrx_vcf_slab: vrx_vcf_begin first");
    VRX_REQUIRE(n_bytes >= 0 && n_bytes < ((int64_t)1 << 31) - 64, "vrx_vcf_slab: a slab holds fewer than 2^31 - 64 bytes");
    VRX_REQUIRE(n_bytes == 0 || text, "vrx_vcf_slab: null text");
    VRX_TRY(h->use());
    hipStream_t s = h->stream;
    info[0] = info[1] = info[2] = 0;
    info[3] = (int64_t)h->table_status;
    if (seconds) seconds[0] = seconds[1] = 0.0;
    h->line_base = h->kept_total;
    h->n = (uint32_t)n_bytes;
    h->n_lines = 0;
    h->n_matched = 0;
    if (n_bytes == 0) return VRX_OK;
    const size_t n = (size_t)n_bytes;
    uint32_t ctl[4];
    std::chrono::steady_clock::time_point t0;
    VRX_TRY(h->in.lines(s, text, n, h->table_status, ctl, seconds, &t0));
    if (ctl[1]) {  // the caller takes the host path: nothing more to do here
        info[3] = ctl[1];
        return VRX_OK;
    }
    const size_t L = ctl[0];
    h->n_lines = (uint32_t)L;
    VRX_HIP(vrx_reserve(h->kept, L));
    VRX_HIP(vrx_reserve(h->tagged, L));
    VRX_HIP(vrx_reserve(h->ord, L));
    VRX_HIP(vrx_reserve(h->mlist, L));
    VRX_HIP(vrx_reserve(h->match, L));
    VRX_HIP(vrx_reserve(h->rec, L));
    VrxVcfLinesArgs g;
    g.text = h->in.text.p;
    g.n = (uint32_t)n;
    g.lstart = h->in.lstart.p;
    g.n_lines = (uint32_t)L;
    g.tag = h->tag;
    g.biallelic_only = h->biallelic_only;
    g.mode = h->mode;
    g.n_ids = h->n_ids;
    g.id_bytes = h->id_bytes.p;
    g.id_off = h->id_off.p;
    g.hash = h->hash.p;
    g.idx = h->idx.p;
    g.claim = h->claim.p;
    g.kept = h->kept.p;
    g.tagged = h->tagged.p;
    g.match = h->match.p;
    g.rec = h->rec.p;
    g.status = h->in.ctl.p + 1;
    vrx_vcf_lines<<<(unsigned)((L + VRX_VCF_WAVES - 1) / VRX_VCF_WAVES), VRX_VCF_BLOCK, 0, s>>>(g);
    VRX_HIP(hipGetLastError());
    VRX_HIP(vrx_cub(h->in.tmp, VRX_CUB_CALL(DeviceScan::InclusiveSum, h->kept.p, h->ord.p, (int)L, s)));
    VRX_HIP(vrx_cub(h->in.tmp, VRX_CUB_CALL(DeviceSelect::Flagged, hipcub::CountingInputIterator<int32_t>(0), h->match.p,
                                            h->mlist.p, h->in.ctl.p + 2, (int)L, s)));
    VRX_HIP(vrx_cub(h->in.tmp, VRX_CUB_CALL(DeviceReduce::Sum, h->tagged.p, reinterpret_cast<int32_t*>(h->in.ctl.p + 3),
                                            (int)L, s)));
    int32_t n_kept = 0;
    VRX_HIP(hipMemcpyAsync(ctl, h->in.ctl.p, sizeof ctl, hipMemcpyDeviceToHost, s));
    VRX_HIP(hipMemcpyAsync(&n_kept, h->ord.p + (L - 1), sizeof n_kept, hipMemcpyDeviceToHost, s));
    VRX_HIP(hipStreamSynchronize(s));
    if (seconds) seconds[1] = seconds_since(t0);
    h->n_matched = ctl[2];
    h->kept_total += n_kept;
    info[0] = n_kept;
    info[1] = ctl[3];
    info[2] = ctl[2];
    info[3] = ctl[1];
    return VRX_OK;
}

extern "C" int vrx_vcf_rows(vrx_vcf* h, double* gpb, int64_t* slot, int64_t* line, int32_t* flag, int64_t* span,
                            double* seconds) {
    VRX_REQUIRE(h, "vrx_vcf_rows: null handle");
    if (seconds) seconds[0] = seconds[1] = 0.0;
    const int64_t M = h->n_matched;
    if (M == 0) return VRX_OK;
    VRX_REQUIRE(gpb && slot && line && flag && span, "vrx_vcf_rows: null output");
    VRX_TRY(h->use());
    hipStream_t s = h->stream;
    const size_t row = (size_t)h->n_sample * 3;
    const int64_t cap = std::min<int64_t>(M, std::max<size_t>(1, kRowBatchBytes / (row * sizeof(double))));
    VRX_HIP(vrx_reserve(h->gpb, (size_t)cap * row));
    VRX_HIP(vrx_reserve(h->slot, (size_t)cap));
    VRX_HIP(vrx_reserve(h->ordinal, (size_t)cap));
    VRX_HIP(vrx_reserve(h->rflag, (size_t)cap));
    VRX_HIP(vrx_reserve(h->span, (size_t)cap * 2));
    VrxVcfRowsArgs g;
    g.text = h->in.text.p;
    g.n = h->n;
    g.n_lines = h->n_lines;
    g.lstart = h->in.lstart.p;
    g.rec = h->rec.p;
    g.ord = h->ord.p;
    g.mlist = h->mlist.p;
    g.line_base = h->line_base;
    g.tag = h->tag;
    g.n_sample = h->n_sample;
    g.matching = h->matching;
    g.pl_table = h->pl_table.p;
    g.gpb = h->gpb.p;
    g.slot = h->slot.p;
    g.ordinal = h->ordinal.p;
    g.flag = h->rflag.p;
    g.span = h->span.p;
    for (int64_t first = 0; first < M; first += cap) {
        const int64_t count = std::min(cap, M - first);
        g.first = first;
        g.count = count;
        auto t0 = std::chrono::steady_clock::now();
        vrx_vcf_rows<<<(unsigned)((count + VRX_VCF_WAVES - 1) / VRX_VCF_WAVES), VRX_VCF_BLOCK, 0, s>>>(g);
        VRX_HIP(hipGetLastError());
        VRX_HIP(hipStreamSynchronize(s));
        if (seconds) seconds[0] += seconds_since(t0);
        t0 = std::chrono::steady_clock::now();
        const size_t c = (size_t)count;
        VRX_HIP(hipMemcpyAsync(gpb + (size_t)first * row, g.gpb, c * row * sizeof(double), hipMemcpyDeviceToHost, s));
        VRX_HIP(hipMemcpyAsync(slot + first, g.slot, c * sizeof(int64_t), hipMemcpyDeviceToHost, s));
        VRX_HIP(hipMemcpyAsync(line + first, g.ordinal, c * sizeof(int64_t), hipMemcpyDeviceToHost, s));
        VRX_HIP(hipMemcpyAsync(flag + first, g.flag, c * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        VRX_HIP(hipMemcpyAsync(span + first * 2, g.span, c * 2 * sizeof(int64_t), hipMemcpyDeviceToHost, s));
        VRX_HIP(hipStreamSynchronize(s));
        if (seconds) seconds[1] += seconds_since(t0);
    }
    return VRX_OK;
}

// ---- cell VCF text: the vrx_cellvcf_* entries on the kernels of vrx_cellvcf.h ------------------------------------
struct vrx_cellvcf : VrxQueue {
    int32_t n_sample = 0, biallelic_only = 1;
    int32_t n_fmt = 0, key0 = 0, key1 = 0;
    uint32_t fmt_len = 0;
    DevBuf<uint8_t> fmt;
    // slab
    uint32_t n = 0, n_lines = 0;
    int64_t n_rows = 0, n_entries = 0;
    VcfText in;  // its ctl: 2 (select count), 3 flagged lines
    DevBuf<uint32_t> off;
    DevBuf<int32_t> kept, ord, nseg, segbase, seg_tabs, seg_entries, tab0, ent0, lineflag;
    // rows
    DevBuf<int32_t> cell, v0, v1, rflag, roff;
    DevBuf<int64_t> indptr, span;
};

extern "C" int32_t vrx_cellvcf_segment(void) { return VRX_CELLVCF_SEGMENT; }

extern "C" void vrx_cellvcf_destroy(vrx_cellvcf* h) { vrx_destroy(h); }

extern "C" int vrx_cellvcf_create(int device, int32_t n_sample, int32_t biallelic_only, vrx_cellvcf** out) {
    VRX_REQUIRE(out, "vrx_cellvcf_create: null argument");
    VRX_REQUIRE(n_sample >= 1, "vrx_cellvcf_create: n_sample >= 1");
    VrxOwned<vrx_cellvcf> h(new vrx_cellvcf());
    VRX_TRY(h->open("vrx_cellvcf_create", device, 0));
    h->n_sample = n_sample;
    h->biallelic_only = biallelic_only != 0;
    VRX_TRY(h->in.create(h->stream));
    VRX_HIP(h->fmt.alloc(VRX_CELLVCF_FORMAT_MAX + 1));
    VRX_HIP(hipStreamSynchronize(h->stream));
    *out = h.release();
    return VRX_OK;
}

extern "C" int vrx_cellvcf_format(vrx_cellvcf* h, const char* fmt, int32_t fmt_len, int32_t key0, int32_t key1) {
    VRX_REQUIRE(h && fmt, "vrx_cellvcf_format: null argument");
    VRX_REQUIRE(fmt_len >= 1 && fmt_len <= VRX_CELLVCF_FORMAT_MAX, "vrx_cellvcf_format: FORMAT has 1 ... %d bytes",
                VRX_CELLVCF_FORMAT_MAX);
    int32_t n_fmt = 1;
    for (int32_t k = 0; k < fmt_len; ++k) n_fmt += fmt[k] == ':';
    VRX_REQUIRE(key0 >= 0 && key0 < n_fmt && key1 >= 0 && key1 < n_fmt, "vrx_cellvcf_format: a key outside FORMAT's %d names",
                n_fmt);
    VRX_TRY(h->use());
    VRX_HIP(hipMemcpyAsync(h->fmt.p, fmt, (size_t)fmt_len, hipMemcpyHostToDevice, h->stream));
    VRX_HIP(hipStreamSynchronize(h->stream));
    h->fmt_len = (uint32_t)fmt_len;
    h->n_fmt = n_fmt;
    h->key0 = key0;
    h->key1 = key1;
    return VRX_OK;
}

extern "C" int vrx_cellvcf_slab(vrx_cellvcf* h, const char* text, int64_t n_bytes, int64_t* info, double* seconds) {
    VRX_REQUIRE(h && info, "vrx_cellvcf_slab: null argument");
    VRX_REQUIRE(n_bytes >= 0 && n_bytes < ((int64_t)1 << 31) - 64, "vrx_cellvcf_slab: a slab holds fewer than 2^31 - 64 bytes");
    VRX_REQUIRE(n_bytes == 0 || text, "vrx_cellvcf_slab: null text");
    VRX_TRY(h->use());
    hipStream_t s = h->stream;
    info[0] = info[1] = info[2] = info[3] = 0;
    if (seconds) seconds[0] = seconds[1] = 0.0;
    h->n = (uint32_t)n_bytes;
    h->n_lines = 0;
    h->n_rows = h->n_entries = 0;
    if (n_bytes == 0) return VRX_OK;
    // 1. line starts
    const size_t n = (size_t)n_bytes;
    uint32_t ctl[4];
    std::chrono::steady_clock::time_point t0;
    VRX_TRY(h->in.lines(s, text, n, 0, ctl, seconds, &t0));
    if (ctl[1]) {
        info[3] = ctl[1];
        return VRX_OK;
    }
    const size_t L = ctl[0];
    h->n_lines = (uint32_t)L;
    VRX_HIP(vrx_reserve(h->kept, L));
    VRX_HIP(vrx_reserve(h->ord, L));
    VRX_HIP(vrx_reserve(h->nseg, L + 1));
    VRX_HIP(vrx_reserve(h->segbase, L + 1));
    VRX_HIP(vrx_reserve(h->lineflag, L));
    VRX_HIP(vrx_reserve(h->off, L * VRX_CELLVCF_OFFS));
    // 2. per line
    VrxCellLinesArgs gl;
    gl.text = h->in.text.p;
    gl.n = (uint32_t)n;
    gl.lstart = h->in.lstart.p;
    gl.n_lines = (uint32_t)L;
    gl.biallelic_only = h->biallelic_only;
    gl.fmt = h->fmt.p;
    gl.fmt_len = h->fmt_len;
    gl.kept = h->kept.p;
    gl.nseg = h->nseg.p;
    gl.off = h->off.p;
    gl.status = h->in.ctl.p + 1;
    VRX_HIP(hipMemsetAsync(h->nseg.p + L, 0, sizeof(int32_t), s));
    VRX_HIP(hipMemsetAsync(h->lineflag.p, 0, L * sizeof(int32_t), s));
    vrx_cellvcf_lines<<<(unsigned)((L + VRX_VCF_WAVES - 1) / VRX_VCF_WAVES), VRX_VCF_BLOCK, 0, s>>>(gl);
    VRX_HIP(hipGetLastError());
    VRX_HIP(vrx_cub(h->in.tmp, VRX_CUB_CALL(DeviceScan::InclusiveSum, h->kept.p, h->ord.p, (int)L, s)));
    VRX_HIP(vrx_cub(h->in.tmp, VRX_CUB_CALL(DeviceScan::ExclusiveSum, h->nseg.p, h->segbase.p, (int)(L + 1), s)));
    int32_t n_kept = 0, n_seg = 0;
    VRX_HIP(hipMemcpyAsync(ctl, h->in.ctl.p, sizeof ctl, hipMemcpyDeviceToHost, s));
    VRX_HIP(hipMemcpyAsync(&n_kept, h->ord.p + (L - 1), sizeof n_kept, hipMemcpyDeviceToHost, s));
    VRX_HIP(hipMemcpyAsync(&n_seg, h->segbase.p + L, sizeof n_seg, hipMemcpyDeviceToHost, s));
    VRX_HIP(hipStreamSynchronize(s));
    if (ctl[1]) {
        h->n_lines = 0;  // (nothing for vrx_cellvcf_rows)
        info[3] = ctl[1];
        if (seconds) seconds[1] = seconds_since(t0);
        return VRX_OK;
    }
    // 3. count pass over the segments, 4. scans
    const size_t G = (size_t)n_seg;
    VRX_HIP(vrx_reserve(h->seg_tabs, G + 1));
    VRX_HIP(vrx_reserve(h->seg_entries, G + 1));
    VRX_HIP(vrx_reserve(h->tab0, G + 1));
    VRX_HIP(vrx_reserve(h->ent0, G + 1));
    VrxCellSegArgs gs;
    gs.text = h->in.text.p;
    gs.off = h->off.p;
    gs.segbase = h->segbase.p;
    gs.n_lines = (uint32_t)L;
    gs.n_seg = (uint32_t)G;
    gs.n_fmt = (uint32_t)h->n_fmt;
    gs.key0 = h->key0;
    gs.key1 = h->key1;
    gs.seg_tabs = h->seg_tabs.p;
    gs.seg_entries = h->seg_entries.p;
    gs.tab0 = h->tab0.p;
    gs.ent0 = h->ent0.p;
    gs.cell = gs.v0 = gs.v1 = nullptr;
    gs.lineflag = h->lineflag.p;
    gs.status = h->in.ctl.p + 1;
    const unsigned seg_blocks = (unsigned)((G + VRX_VCF_WAVES - 1) / VRX_VCF_WAVES);
    VRX_HIP(hipMemsetAsync(h->seg_tabs.p + G, 0, sizeof(int32_t), s));
    VRX_HIP(hipMemsetAsync(h->seg_entries.p + G, 0, sizeof(int32_t), s));
    if (G > 0) {
        vrx_cellvcf_count<<<seg_blocks, VRX_VCF_BLOCK, 0, s>>>(gs);
        VRX_HIP(hipGetLastError());
    }
    VRX_HIP(vrx_cub(h->in.tmp, VRX_CUB_CALL(DeviceScan::ExclusiveSum, h->seg_tabs.p, h->tab0.p, (int)(G + 1), s)));
    VRX_HIP(vrx_cub(h->in.tmp, VRX_CUB_CALL(DeviceScan::ExclusiveSum, h->seg_entries.p, h->ent0.p, (int)(G + 1), s)));
    int32_t n_ent = 0;
    VRX_HIP(hipMemcpyAsync(&n_ent, h->ent0.p + G, sizeof n_ent, hipMemcpyDeviceToHost, s));
    VRX_HIP(hipStreamSynchronize(s));
    // 5. emit pass, then the kept lines as rows
    const size_t E = (size_t)n_ent, R = (size_t)n_kept;
    VRX_HIP(vrx_reserve(h->cell, E + 1));
    VRX_HIP(vrx_reserve(h->v0, E + 1));
    VRX_HIP(vrx_reserve(h->v1, E + 1));
    VRX_HIP(vrx_reserve(h->indptr, R + 1));
    VRX_HIP(vrx_reserve(h->rflag, R + 1));
    VRX_HIP(vrx_reserve(h->span, (R + 1) * 2));
    VRX_HIP(vrx_reserve(h->roff, (R + 1) * VRX_CELLVCF_OFFS));
    gs.cell = h->cell.p;
    gs.v0 = h->v0.p;
    gs.v1 = h->v1.p;
    if (G > 0 && E > 0) {
        vrx_cellvcf_emit<<<seg_blocks, VRX_VCF_BLOCK, 0, s>>>(gs);
        VRX_HIP(hipGetLastError());
    }
    VrxCellRowsArgs gr;
    gr.n = (uint32_t)n;
    gr.n_lines = (uint32_t)L;
    gr.n_seg = (uint32_t)G;
    gr.n_sample = h->n_sample;
    gr.lstart = h->in.lstart.p;
    gr.kept = h->kept.p;
    gr.ord = h->ord.p;
    gr.segbase = h->segbase.p;
    gr.tab0 = h->tab0.p;
    gr.ent0 = h->ent0.p;
    gr.off = h->off.p;
    gr.lineflag = h->lineflag.p;
    gr.indptr = h->indptr.p;
    gr.flag = h->rflag.p;
    gr.span = h->span.p;
    gr.roff = h->roff.p;
    gr.status = h->in.ctl.p + 1;
    gr.n_flagged = h->in.ctl.p + 3;
    vrx_cellvcf_rows<<<(unsigned)((L + VRX_VCF_BLOCK - 1) / VRX_VCF_BLOCK), VRX_VCF_BLOCK, 0, s>>>(gr);
    VRX_HIP(hipGetLastError());
    VRX_HIP(hipMemcpyAsync(ctl, h->in.ctl.p, sizeof ctl, hipMemcpyDeviceToHost, s));
    VRX_HIP(hipStreamSynchronize(s));
    if (seconds) seconds[1] = seconds_since(t0);
    h->n_rows = n_kept;
    h->n_entries = n_ent;
    info[0] = n_kept;
    info[1] = n_ent;
    info[2] = ctl[3];
    info[3] = ctl[1];
    return VRX_OK;
}

extern "C" int vrx_cellvcf_rows(vrx_cellvcf* h, int64_t* indptr, int32_t* cell, int32_t* v0, int32_t* v1, int32_t* flag,
                                int64_t* span, int32_t* off, double* seconds) {
    VRX_REQUIRE(h, "vrx_cellvcf_rows: null handle");
    if (seconds) seconds[0] = 0.0;
    VRX_REQUIRE(indptr, "vrx_cellvcf_rows: null output");
    const size_t R = (size_t)h->n_rows, E = (size_t)h->n_entries;
    VRX_REQUIRE(R == 0 || (flag && span && off), "vrx_cellvcf_rows: null output");
    VRX_REQUIRE(E == 0 || (cell && v0 && v1), "vrx_cellvcf_rows: null output");
    if (h->n_lines == 0) {  // an empty slab, or one that ended with a status
        indptr[0] = 0;
        return VRX_OK;
    }
    VRX_TRY(h->use());
    hipStream_t s = h->stream;
    auto t0 = std::chrono::steady_clock::now();
    VRX_HIP(hipMemcpyAsync(indptr, h->indptr.p, (R + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    if (E > 0) {
        VRX_HIP(hipMemcpyAsync(cell, h->cell.p, E * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        VRX_HIP(hipMemcpyAsync(v0, h->v0.p, E * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        VRX_HIP(hipMemcpyAsync(v1, h->v1.p, E * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    }
    if (R > 0) {
        VRX_HIP(hipMemcpyAsync(flag, h->rflag.p, R * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        VRX_HIP(hipMemcpyAsync(span, h->span.p, R * 2 * sizeof(int64_t), hipMemcpyDeviceToHost, s));
        VRX_HIP(hipMemcpyAsync(off, h->roff.p, R * VRX_CELLVCF_OFFS * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    }
    VRX_HIP(hipStreamSynchronize(s));
    if (seconds) seconds[0] = seconds_since(t0);
    return VRX_OK;
}

// ---- BGZF inflation: the vrx_bgzf_* entries on the decoder of vrx_bgzf.h -----------------------------------------
namespace {
constexpr int64_t kBgzfTextDefault = (int64_t)256 << 20, kBgzfTextMax = (int64_t)1 << 30;

// One wavefront, one workgroup, one member; the working memory of vrx_bgzf.h is the launch's dynamic LDS.
__global__ __launch_bounds__(VRX_BGZF_LANES) void vrx_bgzf_members(const uint8_t* __restrict__ comp,
                                                                   const uint32_t* __restrict__ payload_off,
                                                                   const uint32_t* __restrict__ payload_len,
                                                                   const uint32_t* __restrict__ out_off, uint32_t n_members,
                                                                   const VrxBgzfCrc* __restrict__ crc,
                                                                   uint8_t* __restrict__ text, int32_t* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) uint8_t vrx_bgzf_lds[];
    VrxBgzfWork& w = *reinterpret_cast<VrxBgzfWork*>(vrx_bgzf_lds);
    const uint32_t m = blockIdx.x, lane = threadIdx.x;
    if (m >= n_members) return;
    {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(crc);
        uint32_t* dst = reinterpret_cast<uint32_t*>(&w.crc);
        for (uint32_t i = lane; i < sizeof(VrxBgzfCrc) / sizeof(uint32_t); i += VRX_BGZF_LANES) dst[i] = src[i];
    }
    __syncthreads();
    const uint8_t* payload = comp + payload_off[m];
    const uint32_t n = payload_len[m], room = out_off[m + 1] - out_off[m];
    const uint32_t want_crc = vrx_bgzf_le32(payload + n), isize = vrx_bgzf_le32(payload + n + 4);
    uint32_t st = VRX_BGZF_ST_ISIZE;
    if (isize == room) st = vrx_bgzf_member(w, payload, n, isize, want_crc, w.window);
    if (st == 0) {
        uint8_t* dst = text + out_off[m];
        for (uint32_t i = lane; i < isize; i += VRX_BGZF_LANES) dst[i] = w.window[i];
    }
    if (lane == 0) status[m] = (int32_t)st;
}

struct PinnedBytes {
    uint8_t* p = nullptr;
    size_t n = 0;
    PinnedBytes() = default;
    PinnedBytes(const PinnedBytes&) = delete;
    PinnedBytes& operator=(const PinnedBytes&) = delete;
    ~PinnedBytes() {
        if (p) (void)hipHostFree(p);
    }
    hipError_t reserve(size_t count) {
        if (n >= count) return hipSuccess;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        n = 0;
        hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&p), count + count / 8, hipHostMallocDefault);
        if (e == hipSuccess) n = count + count / 8;
        return e;
    }
};
}  // namespace

struct vrx_bgzf : VrxQueue {
    int64_t max_text = 0;
    PinnedBytes pin;  // the compressed bytes on their way up, then the text on its way down
    DevBuf<uint8_t> comp, text;
    DevBuf<uint32_t> meta;  // payload_off, payload_len (n each), out_off (n + 1)
    DevBuf<int32_t> status;
    DevBuf<VrxBgzfCrc> crc;
};

extern "C" int vrx_bgzf_scan(const uint8_t* file, int64_t n_bytes, int64_t room, int64_t* n_members, int64_t* payload_off,
                             int32_t* payload_len, int32_t* isize, int64_t* out_off, int32_t* status) {
    VRX_REQUIRE(n_members && status, "vrx_bgzf_scan: null argument");
    VRX_REQUIRE(n_bytes >= 0 && (n_bytes == 0 || file), "vrx_bgzf_scan: null file");
    VRX_REQUIRE(room >= 0 && (room == 0 || (payload_off && payload_len && isize && out_off)), "vrx_bgzf_scan: null output");
    *status = vrx_bgzf_scan_image(file, n_bytes, room, n_members, payload_off, payload_len, isize, out_off);
    return VRX_OK;
}

extern "C" void vrx_bgzf_destroy(vrx_bgzf* h) { vrx_destroy(h); }

extern "C" int vrx_bgzf_create(int device, int64_t max_text, vrx_bgzf** out) {
    VRX_REQUIRE(out, "vrx_bgzf_create: null argument");
    if (max_text == 0) max_text = kBgzfTextDefault;
    VRX_REQUIRE(max_text >= VRX_BGZF_TEXT_MAX && max_text <= kBgzfTextMax, "vrx_bgzf_create: max_text is 64 KiB ... 1 GiB");
    VrxOwned<vrx_bgzf> h(new vrx_bgzf());
    VRX_TRY(h->open("vrx_bgzf_create", device, 0));
    h->max_text = max_text;
    VrxBgzfCrc tables;
    vrx_bgzf_crc_init(tables);
    VRX_HIP(h->crc.upload(&tables, 1, h->stream));
    VRX_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(vrx_bgzf_members), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)sizeof(VrxBgzfWork)));
    VRX_HIP(hipStreamSynchronize(h->stream));  // (the tables die at return)
    *out = h.release();
    return VRX_OK;
}

extern "C" int vrx_bgzf_inflate(vrx_bgzf* h, const uint8_t* comp, int64_t n_comp, int64_t n_members,
                                const int64_t* payload_off, const int32_t* payload_len, const int64_t* out_off, uint8_t* text,
                                int32_t* status, double* seconds) {
    VRX_REQUIRE(h && comp && payload_off && payload_len && out_off && status, "vrx_bgzf_inflate: null argument");
    VRX_REQUIRE(n_members >= 1 && n_members < ((int64_t)1 << 31) - 1, "vrx_bgzf_inflate: 1 <= n_members < 2^31 - 1");
    VRX_REQUIRE(n_comp >= 1 && n_comp < ((int64_t)1 << 31), "vrx_bgzf_inflate: 1 <= n_comp < 2^31");
    VRX_REQUIRE(out_off[0] == 0, "vrx_bgzf_inflate: out_off starts at 0");
    for (int64_t i = 0; i < n_members; ++i) {
        VRX_REQUIRE(payload_len[i] >= 0 && payload_off[i] >= 0 &&
                        payload_off[i] <= n_comp - VRX_BGZF_FOOTER - (int64_t)payload_len[i],
                    "vrx_bgzf_inflate: member %lld lies outside the compressed bytes", (long long)i);
        VRX_REQUIRE(out_off[i + 1] >= out_off[i] && out_off[i + 1] - out_off[i] <= VRX_BGZF_TEXT_MAX,
                    "vrx_bgzf_inflate: member %lld has 0 ... 65536 bytes of text", (long long)i);
    }
    const int64_t n_text = out_off[n_members];
    VRX_REQUIRE(n_text <= h->max_text, "vrx_bgzf_inflate: %lld bytes of text in a batch of at most %lld", (long long)n_text,
                (long long)h->max_text);
    VRX_REQUIRE(n_text == 0 || text, "vrx_bgzf_inflate: null text");
    if (seconds) seconds[0] = seconds[1] = seconds[2] = 0.0;
    VRX_TRY(h->use());
    hipStream_t s = h->stream;
    const size_t M = (size_t)n_members, meta_bytes = (3 * M + 1) * sizeof(uint32_t);
    // upload: the members and where they lie, through the pinned buffer
    auto t0 = std::chrono::steady_clock::now();
    VRX_HIP(h->pin.reserve(std::max((size_t)n_comp + meta_bytes, (size_t)n_text)));
    VRX_HIP(vrx_reserve(h->comp, (size_t)n_comp));
    VRX_HIP(vrx_reserve(h->meta, 3 * M + 1));
    VRX_HIP(vrx_reserve(h->status, M));
    VRX_HIP(vrx_reserve(h->text, std::max<size_t>((size_t)n_text, 1)));
    uint32_t* meta = reinterpret_cast<uint32_t*>(h->pin.p);
    for (size_t i = 0; i < M; ++i) {
        meta[i] = (uint32_t)payload_off[i];
        meta[M + i] = (uint32_t)payload_len[i];
        meta[2 * M + i] = (uint32_t)out_off[i];
    }
    meta[3 * M] = (uint32_t)n_text;
    std::copy(comp, comp + n_comp, h->pin.p + meta_bytes);
    VRX_HIP(hipMemcpyAsync(h->meta.p, meta, meta_bytes, hipMemcpyHostToDevice, s));
    VRX_HIP(hipMemcpyAsync(h->comp.p, h->pin.p + meta_bytes, (size_t)n_comp, hipMemcpyHostToDevice, s));
    VRX_HIP(hipStreamSynchronize(s));
    if (seconds) seconds[0] = seconds_since(t0);
    t0 = std::chrono::steady_clock::now();
    vrx_bgzf_members<<<(unsigned)M, VRX_BGZF_LANES, sizeof(VrxBgzfWork), s>>>(h->comp.p, h->meta.p, h->meta.p + M,
                                                                              h->meta.p + 2 * M, (uint32_t)M, h->crc.p,
                                                                              h->text.p, h->status.p);
    VRX_HIP(hipGetLastError());
    VRX_HIP(hipStreamSynchronize(s));
    if (seconds) seconds[1] = seconds_since(t0);
    t0 = std::chrono::steady_clock::now();
    VRX_HIP(hipMemcpyAsync(status, h->status.p, M * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (n_text > 0) VRX_HIP(hipMemcpyAsync(h->pin.p, h->text.p, (size_t)n_text, hipMemcpyDeviceToHost, s));
    VRX_HIP(hipStreamSynchronize(s));
    if (n_text > 0) std::copy(h->pin.p, h->pin.p + n_text, text);
    if (seconds) seconds[2] = seconds_since(t0);
    return VRX_OK;
}
