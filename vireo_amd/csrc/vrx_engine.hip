// Host side of libvireo_hip.so: the C ABI of include/vireo_hip.h.
// Owns the device state, schedules the kernels of vrx_kernels.h on one HIP stream per
// problem and runs the coordinate-ascent loop of the reference
// (vireoSNP/utils/vireo_model.py:251-276, vireoSNP/utils/bmm_model.py:178-201).
#include <algorithm>
#include <atomic>
#include <chrono>
#include <thread>
#include <cmath>
#include <cstdarg>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "vrx_handle.h"
#include "vrx_kernels.h"
#include "vrx_build.h"
#include "vrx_ambient.h"

// (vrx_set_error / vrx_last_error: vrx_host.cpp, so that the host-only translation unit links on
//  its own for the sanitizer build of tests/test_host_sanitizers_cpu.py)

extern "C" int vrx_device_count(int* n) {
    VRX_REQUIRE(n, "vrx_device_count: null output");
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        c = 0;
    }
    *n = c;
    return VRX_OK;
}

int vrx_use_device(const char* who, int device) {
    int ndev = 0;
    vrx_device_count(&ndev);
    if (device < 0 || device >= ndev) {
        vrx_set_error("%s: device %d not available (%d HIP devices visible)", who, device, ndev);
        return VRX_ERR_HIP;
    }
    VRX_HIP(hipSetDevice(device));
    return VRX_OK;
}

extern "C" int vrx_device_info(int device, char* name, int name_len, int* n_cu,
                               int64_t* hbm_bytes) {
    hipDeviceProp_t prop;
    VRX_HIP(hipGetDeviceProperties(&prop, device));
    if (name && name_len > 0) {
        // (some boxes report an empty marketing name: say what the arch is then)
        snprintf(name, name_len, "%s (%s)", prop.name[0] ? prop.name : "AMD GPU",
                 prop.gcnArchName);
    }
    if (n_cu) *n_cu = prop.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = (int64_t)prop.totalGlobalMem;
    return VRX_OK;
}

// "0000:c1:00.0" of a device: which physical GPU a rank of the restart shard sits on
// (bench.py's `comm` block lists it per rank)
extern "C" int vrx_device_pci_bus_id(int device, char* out, int out_len) {
    VRX_REQUIRE(out && out_len >= 16, "vrx_device_pci_bus_id: buffer of >= 16 bytes needed");
    VRX_HIP(hipDeviceGetPCIBusId(out, out_len, device));
    return VRX_OK;
}

// ------------------------------------------------------------------------------------
// problem
// ------------------------------------------------------------------------------------
static constexpr int kSegCap = 4096;     // entries per segment (one wavefront each)
static constexpr int kXcd = 8;           // XCDs per MI355X; workgroup b is observed on XCD b % 8
static constexpr double kSlabBytes = 1.6e6;  // dense-operand slab per tile (fits a 4 MiB L2)

// Host-side build of a problem (validation, transposition, packing, tiling) is plain loops
// over the non-zeros; they are spread over host threads (VIREO_HOST_THREADS, default <= 64).
static int host_threads() {
    static const int n = [] {
        const char* v = getenv("VIREO_HOST_THREADS");
        int t = v && *v ? atoi(v) : (int)std::min(64u, std::max(1u, std::thread::hardware_concurrency()));
        return std::max(1, t);
    }();
    return n;
}

// the per-tile greedy of the balanced-slab build is compute in a core's own L2: it takes more threads
static int balance_threads() {
    const char* v = getenv("VIREO_HOST_THREADS");
    if (v && *v) return host_threads();
    return (int)std::min(128u, std::max(1u, std::thread::hardware_concurrency()));
}

// uninitialised host array (a std::vector would zero hundreds of MB on one thread first)
template <class T>
struct RawArray {
    T* p = nullptr;
    explicit RawArray(size_t n) : p(static_cast<T*>(std::malloc(std::max<size_t>(n, 1) * sizeof(T)))) {}
    RawArray(const RawArray&) = delete;
    RawArray& operator=(const RawArray&) = delete;
    ~RawArray() { std::free(p); }
    T* data() { return p; }
    T& operator[](size_t i) { return p[i]; }
};

// f(begin, end, tid) over [0, n) cut into contiguous chunks, one per thread
template <class F>
static void parallel_chunks(int64_t n, int n_threads, F&& f) {
    n_threads = (int)std::max<int64_t>(1, std::min<int64_t>(n_threads, n));
    if (n_threads == 1) {
        f((int64_t)0, n, 0);
        return;
    }
    std::vector<std::thread> pool;
    pool.reserve((size_t)n_threads);
    for (int t = 0; t < n_threads; ++t) {
        const int64_t b = n * t / n_threads, e = n * (t + 1) / n_threads;
        pool.emplace_back([&f, b, e, t] { f(b, e, t); });
    }
    for (auto& th : pool) th.join();
}

static int env_int(const char* name, int dflt) {
    const char* v = getenv(name);
    return v && *v ? atoi(v) : dflt;
}

// number of tiles over the contracted dimension for a dense operand of `row_bytes` per
// contracted index (nominal K = 16): 1, 2, 4, 8 or a multiple of 8
static int pick_tiles(int64_t n_contract, double row_bytes, const char* env) {
    int t = env_int(env, 0);
    // (an operand of up to two slabs still sits in one XCD's 4 MiB L2: one tile, and no rows
    //  split over tiles whose slots need a second kernel to sum -- c2: 45.1 -> 42.7 us)
    if (t <= 0) t = n_contract * row_bytes <= 2.0 * kSlabBytes ? 1 : (int)std::lround(n_contract * row_bytes / kSlabBytes);
    if (t <= 1) return 1;
    if (t <= kXcd) {
        int p = 1;
        while (p < t) p <<= 1;
        return p;
    }
    return (t + kXcd - 1) / kXcd * kXcd;
}

// Pack the entries of one orientation, build its tiled / XCD-ordered segment table, upload.
//   contract_count[i] = number of entries with contracted index i (for equal-nnz tiles)
static int build_orient(Orient& o, int64_t n_rows, int64_t n_contract, const int64_t* ptr,
                        const int32_t* idx, const int2* val, const int64_t* contract_ptr,
                        int n_tiles, int fmt, hipStream_t s) {
    o.n_rows = n_rows;
    o.n_contract = n_contract;
    o.nnz = ptr[n_rows];
    o.fmt = fmt;
    o.n_tiles = n_tiles;
    // ---- entries ------------------------------------------------------------------
    const int ew = fmt + 1;
    RawArray<uint32_t> ent((size_t)o.nnz * ew);
    VRX_REQUIRE(ent.p, "out of host memory");
    parallel_chunks(o.nnz, host_threads(), [&](int64_t b, int64_t e_end, int) {
        for (int64_t e = b; e < e_end; ++e) {
            const uint32_t id = (uint32_t)idx[e], ad = (uint32_t)val[e].x, dp = (uint32_t)val[e].y;
            if (fmt == VRX_FMT_P32) {
                ent[(size_t)e] = (id << 12) | (ad << 6) | dp;
            } else if (fmt == VRX_FMT_P64) {
                ent[(size_t)e * 2] = id;
                ent[(size_t)e * 2 + 1] = ad | (dp << 16);
            } else {
                ent[(size_t)e * 3] = id;
                ent[(size_t)e * 3 + 1] = ad;
                ent[(size_t)e * 3 + 2] = dp;
            }
        }
    });
    // ---- tile boundaries: equal entry counts ------------------------------------------
    std::vector<int64_t> bound((size_t)n_tiles + 1, n_contract);
    bound[0] = 0;
    for (int t = 1; t < n_tiles; ++t) {
        const int64_t want = o.nnz * t / n_tiles;
        bound[(size_t)t] = std::lower_bound(contract_ptr, contract_ptr + n_contract + 1, want) -
                           contract_ptr;
        if (bound[(size_t)t] > n_contract) bound[(size_t)t] = n_contract;
        if (bound[(size_t)t] < bound[(size_t)t - 1]) bound[(size_t)t] = bound[(size_t)t - 1];
    }
    // ---- segments, grouped per tile -----------------------------------------------------
    struct Seg {
        int64_t begin;
        int32_t len, dst;
    };
    std::vector<std::vector<Seg>> per_tile((size_t)n_tiles);
    std::vector<int32_t> multi_row, multi_ptr;
    multi_ptr.push_back(0);
    int64_t slots = 0;
    std::vector<Seg> row_segs;
    std::vector<int> row_tile;
    for (int64_t r = 0; r < n_rows; ++r) {
        const int64_t lo = ptr[r], hi = ptr[r + 1];
        if (hi <= lo) {  // empty row: its output stays 0 (buffers are zero-filled)
            ++o.n_empty;
            continue;
        }
        row_segs.clear();
        row_tile.clear();
        int64_t at = lo;
        for (int t = 0; t < n_tiles && at < hi; ++t) {
            const int64_t end = n_tiles == 1 ? hi
                                             : std::lower_bound(idx + at, idx + hi,
                                                                (int32_t)std::min<int64_t>(bound[(size_t)t + 1], INT32_MAX)) - idx;
            int64_t len = end - at;
            if (len <= 0) continue;
            const int64_t parts = (len + kSegCap - 1) / kSegCap;
            int64_t chunk = (len + parts - 1) / parts;
            if (parts > 1) chunk = (chunk + 63) / 64 * 64;
            for (int64_t b = 0; b < len; b += chunk) {
                row_segs.push_back({at + b, (int32_t)std::min(chunk, len - b), 0});
                row_tile.push_back(t);
            }
            at = end;
        }
        if (row_segs.size() == 1) {
            row_segs[0].dst = (int32_t)r;
        } else {
            for (auto& sg : row_segs) sg.dst = (int32_t)(-(++slots));
            multi_row.push_back((int32_t)r);
            multi_ptr.push_back((int32_t)slots);
        }
        for (size_t i = 0; i < row_segs.size(); ++i) per_tile[(size_t)row_tile[i]].push_back(row_segs[i]);
    }
    if (slots >= INT32_MAX) {
        vrx_set_error("too many segments");
        return VRX_ERR_UNSUPPORTED;
    }
    // ---- launch order: tile t -> XCD t % 8 (tiles < 8: each tile shared by 8/n_tiles XCDs)
    std::vector<std::vector<Seg>> per_xcd(kXcd);
    if (n_tiles >= kXcd) {
        for (int t = 0; t < n_tiles; ++t) {
            auto& dst = per_xcd[(size_t)(t % kXcd)];
            dst.insert(dst.end(), per_tile[(size_t)t].begin(), per_tile[(size_t)t].end());
        }
    } else {
        const int share = kXcd / n_tiles;  // XCDs per tile
        for (int t = 0; t < n_tiles; ++t) {
            const auto& src = per_tile[(size_t)t];
            for (size_t i = 0; i < src.size(); ++i) {
                const int x = t + n_tiles * (int)((i / VRX_WAVES) % share);
                per_xcd[(size_t)x].push_back(src[i]);
            }
        }
    }
    size_t longest = 0;
    for (auto& v : per_xcd) longest = std::max(longest, v.size());
    const size_t blocks_per_xcd = (longest + VRX_WAVES - 1) / VRX_WAVES;
    const size_t total = blocks_per_xcd * kXcd * VRX_WAVES;
    std::vector<int64_t> seg_begin(total, 0);
    std::vector<int32_t> seg_len(total, -1), seg_dst(total, 0);
    for (int x = 0; x < kXcd; ++x)
        for (size_t i = 0; i < per_xcd[(size_t)x].size(); ++i) {
            const size_t pos = ((i / VRX_WAVES) * kXcd + (size_t)x) * VRX_WAVES + i % VRX_WAVES;
            seg_begin[pos] = per_xcd[(size_t)x][i].begin;
            seg_len[pos] = per_xcd[(size_t)x][i].len;
            seg_dst[pos] = per_xcd[(size_t)x][i].dst;
        }
    if (total >= (size_t)INT32_MAX) {
        vrx_set_error("too many segments");
        return VRX_ERR_UNSUPPORTED;
    }
    o.n_seg = (int64_t)total;
    o.n_multi = (int64_t)multi_row.size();
    o.n_slots = slots;
    VRX_HIP(o.ent.upload(ent.data(), (size_t)o.nnz * ew, s));
    VRX_HIP(o.seg_begin.upload(seg_begin.data(), seg_begin.size(), s));
    VRX_HIP(o.seg_len.upload(seg_len.data(), seg_len.size(), s));
    VRX_HIP(o.seg_dst.upload(seg_dst.data(), seg_dst.size(), s));
    VRX_HIP(o.multi_row.upload(multi_row.data(), multi_row.size(), s));
    VRX_HIP(o.multi_ptr.upload(multi_ptr.data(), multi_ptr.size(), s));
    VRX_HIP(hipStreamSynchronize(s));  // the host vectors die at return
    return VRX_OK;
}

// Tiled entry stream for vrx_spmm_lds (see vrx_kernels.h): RW rows per wave handled
// 16 at a time (a round), 16 waves per tile, slabs of slab_rows contracted indices; inside a
// round the words are trip-major and zero-padded to the round's longest row.
//
// Ragged data (heavy-tailed coverage / depth): a round costs its LONGEST row and a workgroup
// its slowest wave, so (1) a row much longer than the mean is cut into P interleaved PIECES
// (entry j of a slab segment -> piece (j + slab) % P) that accumulate separately and are
// summed afterwards in piece order (vrx_sum_pieces), (2) pieces are sorted by length so that
// a round holds 16 similar ones, (3) the sorted rounds are dealt to the waves in snake order
// so that every wave (and tile) carries about the same number of entries.
//
// form 1 (cell pass): every (ad, dp) entry becomes single-valued entries of AD and of
// BD = DP - AD (none for a zero, several for a value outside 15 signed bits), see FORM 1 in
// vrx_kernels.h.  Word = value:15 | (2 * slab-local index + half) * 128.
struct DevRows {
    const int64_t* ptr;
    const int32_t* idx;
    const int2* val;
};
// The rows a stream is built from: the row pointer on the host, the entries on the host (idx / val: the host
// builder) or on the device (dev.ptr != nullptr: the device builder, vrx_build.h).  virt: the VIRTUAL rows of
// the variant pass (vrx_build.h).
struct TileRows {
    const int64_t* ptr;
    const int32_t* idx;
    const int2* val;
    DevRows dev;
    int64_t n_rows, n_contract, nnz;
    bool virt;
};
// The stream asked for: rows per wave, slab height, word form (0 pairs, 1 AD / BD words),
// pass (0 variant, 1 cell), the padding guard (VIREO_LDS_MAX_PAD), balanced slabs (TiledStream::perm).
struct TileShape {
    int RW, slab_rows, form, mode;
    bool guard, balance;
};

// Work list of an LDS-resident pass (TiledStream::items).  The (tile, slab) visits, tile-major,
// are cut into n_wg contiguous runs of equal cost -- cost of a visit = the longest wave's trips in
// that slab + the staging of the slab, in trips -- so that every CU is busy for the whole launch
// and a tile is cut into few pieces (tiles + n_wg pieces at most: the partial outputs the
// consumers add up).  bnd = the per-wave (slab, round) offsets on the host.
static int plan_items(TiledStream& t, const int32_t* bnd, int n_cu, const int32_t* rowmap, hipStream_t s) {
    constexpr int G = 64 / VRX_LDS_LPE, UG = VRX_LDS_U * G;
    constexpr double stage = 10.0;  // staging a slab, in trips
    const int nr = t.rw / G;
    const int64_t per_wave = (int64_t)t.n_slab * nr + 1, visits = (int64_t)t.n_tile * t.n_slab;
    const int n_wg = (int)std::max<int64_t>(1, std::min<int64_t>(env_int("VIREO_LDS_BLOCKS", std::max(1, n_cu)), visits));
    std::vector<double> cost((size_t)visits);
    parallel_chunks(t.n_tile, host_threads(), [&](int64_t t0, int64_t t1, int) {
        for (int64_t tl = t0; tl < t1; ++tl)
            for (int sl = 0; sl < t.n_slab; ++sl) {
                int32_t longest = 0;
                for (int w = 0; w < VRX_LDS_WAVES; ++w) {
                    const int32_t* bw = bnd + (tl * VRX_LDS_WAVES + w) * per_wave;
                    longest = std::max(longest, (bw[(int64_t)(sl + 1) * nr] & ~(UG - 1)) -
                                                    (bw[(int64_t)sl * nr] & ~(UG - 1)));
                }
                cost[(size_t)(tl * t.n_slab + sl)] = (double)longest / UG + stage;
            }
    });
    double total = 0.0;
    for (double c : cost) total += c;
    std::vector<int32_t> items, first((size_t)n_wg + 1, 0), pieces((size_t)t.n_tile, 0);
    double acc = 0.0;
    int64_t u = 0;
    for (int b = 0; b < n_wg; ++b) {
        first[(size_t)b] = (int32_t)(items.size() / 4);
        // run b ends at the visit where the accumulated cost passes (b + 1) / n_wg of the total
        // (every run gets at least one visit while visits remain for the runs behind it)
        const double goal = total * (double)(b + 1) / (double)n_wg;
        int64_t end = u;
        while (end < visits && (end == u || acc + cost[(size_t)end] * 0.5 <= goal) &&
               visits - (end + 1) >= n_wg - 1 - b)
            acc += cost[(size_t)end++];
        if (b == n_wg - 1)
            while (end < visits) acc += cost[(size_t)end++];
        while (u < end) {  // cut the run at tile boundaries
            const int64_t tl = u / t.n_slab, s0 = u % t.n_slab;
            const int64_t s1 = std::min<int64_t>(t.n_slab, s0 + (end - u));
            items.insert(items.end(), {(int32_t)tl, (int32_t)s0, (int32_t)s1, pieces[(size_t)tl]++});
            u += s1 - s0;
        }
    }
    first[(size_t)n_wg] = (int32_t)(items.size() / 4);
    // Which workgroup walks which run.  The runs start at every phase of the slab cycle, so in
    // launch order the workgroups of one XCD would stage different slabs at any time and share
    // nothing in their L2 (measured: the passes' L2-miss traffic 1.1 -> 1.6 GB per launch).
    // Workgroup b runs on XCD b % 8 (observed dispatch rule; used for speed only): the runs are
    // sorted by the slab they start at and dealt XCD by XCD, so that the ~32 workgroups of an
    // XCD walk neighbouring slabs together and every slab is fetched into that L2 about once.
    if (n_wg > kXcd) {
        std::vector<int> run((size_t)n_wg);
        for (int b = 0; b < n_wg; ++b) run[(size_t)b] = b;
        auto phase = [&](int b) {
            return first[(size_t)b] < first[(size_t)b + 1] ? items[(size_t)(4 * first[(size_t)b] + 1)] : INT32_MAX;
        };
        std::stable_sort(run.begin(), run.end(), [&](int a, int b) { return phase(a) < phase(b); });
        std::vector<int> run_of_wg((size_t)n_wg, -1);
        int next = 0;
        for (int x = 0; x < kXcd; ++x)
            for (int b = x; b < n_wg; b += kXcd) run_of_wg[(size_t)b] = run[(size_t)next++];
        std::vector<int32_t> it2, f2((size_t)n_wg + 1, 0);
        for (int b = 0; b < n_wg; ++b) {
            const int r = run_of_wg[(size_t)b];
            f2[(size_t)b] = (int32_t)(it2.size() / 4);
            it2.insert(it2.end(), items.begin() + 4 * first[(size_t)r], items.begin() + 4 * first[(size_t)r + 1]);
        }
        f2[(size_t)n_wg] = (int32_t)(it2.size() / 4);
        items.swap(it2);
        first.swap(f2);
    }
    t.n_wg = n_wg;
    t.n_range = 1;
    for (int32_t c : pieces) t.n_range = std::max(t.n_range, (int)c);
    VRX_REQUIRE(t.n_range < 65536, "tiled stream: a tile is cut into too many pieces");
    std::vector<uint16_t> npiece((size_t)t.n_vrows, 0);
    const int64_t tile_pos = (int64_t)VRX_LDS_WAVES * t.rw;
    for (int64_t pos = 0; pos < (int64_t)t.n_tile * tile_pos; ++pos)
        if (rowmap[(size_t)pos] >= 0) npiece[(size_t)rowmap[(size_t)pos]] = (uint16_t)pieces[(size_t)(pos / tile_pos)];
    VRX_HIP(t.items.upload(items.data(), items.size(), s));
    VRX_HIP(t.wg_first.upload(first.data(), first.size(), s));
    VRX_HIP(t.npiece.upload(npiece.data(), npiece.size(), s));
    VRX_HIP(hipStreamSynchronize(s));
    return VRX_OK;
}

// the virtual rows of the variant pass on the host (vrx_build.h: vrx_virt_count / vrx_virt_fill
// are the same derivation on the device)
static void derive_virtual_rows(int64_t n_var, const int64_t* rptr, const int32_t* ridx, const int2* rval,
                                std::vector<int64_t>& vptr2, std::vector<int32_t>& vidx, std::vector<int2>& vval) {
    vptr2.assign((size_t)(2 * n_var + 1), 0);
    parallel_chunks(n_var, host_threads(), [&](int64_t n0, int64_t n1, int) {
        for (int64_t n = n0; n < n1; ++n) {
            int64_t ca = 0, cb = 0;
            int32_t ja = -1, jb = -1;
            for (int64_t e = rptr[n]; e < rptr[n + 1]; ++e) {
                const int32_t j = ridx[e] >> 1;
                if (rval[e].x != 0 && j != ja) ++ca, ja = j;
                if (rval[e].y - rval[e].x != 0 && j != jb) ++cb, jb = j;
            }
            vptr2[(size_t)(2 * n + 1)] = ca;   // (counts: scanned below)
            vptr2[(size_t)(2 * n + 2)] = cb;
        }
    });
    for (int64_t r = 0; r < 2 * n_var; ++r) vptr2[(size_t)r + 1] += vptr2[(size_t)r];
    vidx.resize((size_t)vptr2[(size_t)(2 * n_var)]);
    vval.resize(vidx.size());
    parallel_chunks(n_var, host_threads(), [&](int64_t n0, int64_t n1, int) {
        for (int64_t n = n0; n < n1; ++n) {
            int64_t oa = vptr2[(size_t)(2 * n)] - 1, ob = vptr2[(size_t)(2 * n + 1)] - 1;
            int32_t ja = -1, jb = -1;
            for (int64_t e = rptr[n]; e < rptr[n + 1]; ++e) {
                const int32_t c = ridx[e], j = c >> 1;
                const int a = rval[e].x, b = rval[e].y - rval[e].x;
                if (a != 0) {
                    if (j != ja) ++oa, ja = j, vidx[(size_t)oa] = j, vval[(size_t)oa] = make_int2(0, 0);
                    if (c & 1) vval[(size_t)oa].y += a; else vval[(size_t)oa] = make_int2(a, vval[(size_t)oa].y + a);
                }
                if (b != 0) {
                    if (j != jb) ++ob, jb = j, vidx[(size_t)ob] = j, vval[(size_t)ob] = make_int2(0, 0);
                    if (c & 1) vval[(size_t)ob].y += b; else vval[(size_t)ob] = make_int2(b, vval[(size_t)ob].y + b);
                }
            }
        }
    });
}

// smallest b >= 1 with 2^b >= n: the key bits of a radix sort over n values
static int bits_for(int64_t n) {
    int b = 1;
    while (((int64_t)1 << b) < n) ++b;
    return b;
}

// VIREO_BUILD_TIMING=1: where a build spends its wall clock, lap by lap (a lap waits for the stream first)
struct LapTimer {
    hipStream_t s;
    std::string label;
    int width;
    bool on = env_int("VIREO_BUILD_TIMING", 0) != 0;
    double begin = now(), last = begin;
    static double now() {
        return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
    }
    void operator()(const char* what) {
        if (!on) return;
        (void)hipStreamSynchronize(s);
        const double t1 = now();
        fprintf(stderr, "[vrx build] %s %-*s %.3f s\n", label.c_str(), width, what, t1 - last);
        last = t1;
    }
};

// ---- balanced slabs (r6; TiledStream::perm) -------------------------------------------------------
// The padding of a round is the maximum over its 16 rows of their words in ONE slab; which contracted
// rows share a slab is free per tile.  Greedy, per tile: the contracted rows ("columns" of the tile's
// sub-matrix) most-covered first, each to the slab -- among those with room -- where the sum of the
// present loads of the rows it touches is smallest (ties: the lowest slab); columns without an entry in
// the tile fill what is left.  Counted on the c3 matrix: 1.62 -> 1.17 executed slots per word.
// Deterministic (the result is part of the stream both greedy routes must agree on).

// (the greedy itself: vrx_host.cpp, vrx_balance_tile -- host only, built with AVX2 clones of its inner loops)
void vrx_balance_tile(const int32_t* rows, int64_t n_rows_tile, const int64_t* ptr, const int32_t* idx,
                      const uint8_t* words, int64_t n_contract, int n_slab, int slab_rows, int max_block,
                      int32_t* posmap, int32_t* perm);

// Stage (a), the host half of a tiled stream that needs nothing but the row pointer: the pieces long rows are
// cut into, the tile / slab geometry, and which piece sits at which tile position.
struct TileLayout {
    std::vector<int32_t> vptr, vrow_row, split_rows, rowmap;
    int64_t n_vrows = 0;
    bool split = false;
    int n_tile = 0, n_slab = 0, slab_rows = 0;
};

static int tile_layout(TileLayout& L, const TileRows& R, const TileShape& S, int n_cu) {
    constexpr int G = 64 / VRX_LDS_LPE;
    const int64_t* ptr = R.ptr;
    const int RW = S.RW;
    int slab_rows = S.slab_rows;
    L.slab_rows = slab_rows;
    L.n_slab = (int)((R.n_contract + slab_rows - 1) / slab_rows);
    // ---- pieces ------------------------------------------------------------------------
    const double mean = (double)R.nnz / (double)std::max<int64_t>(R.n_rows, 1);
    const int64_t cap = std::max<int64_t>(
        64, (int64_t)(mean * (double)env_int("VIREO_LDS_SPLIT_X10", 20) / 10.0 + 0.5));
    const bool reorder = env_int("VIREO_LDS_SORT", 1) != 0;
    std::vector<int32_t>& vptr = L.vptr;
    vptr.assign((size_t)R.n_rows + 1, 0);
    for (int64_t r = 0; r < R.n_rows; ++r) {
        const int64_t len = ptr[r + 1] - ptr[r];
        const int64_t P = reorder ? std::max<int64_t>(1, (len + cap - 1) / cap) : 1;
        if ((int64_t)vptr[(size_t)r] + P >= INT32_MAX) {
            vrx_set_error("tiled stream: too many row pieces");
            return VRX_ERR_UNSUPPORTED;
        }
        vptr[(size_t)r + 1] = vptr[(size_t)r] + (int32_t)P;
    }
    const int64_t n_vrows = vptr[(size_t)R.n_rows];
    L.n_vrows = n_vrows;
    L.split = n_vrows != R.n_rows;
    std::vector<int32_t>& split_rows = L.split_rows;  // rows cut into several pieces: folded by vrx_fold_split
    split_rows.clear();
    for (int64_t r = 0; r < R.n_rows; ++r)
        if (vptr[(size_t)r + 1] - vptr[(size_t)r] > 1) split_rows.push_back((int32_t)r);
    std::vector<int32_t>& vrow_row = L.vrow_row;
    vrow_row.assign((size_t)n_vrows, 0);
    for (int64_t r = 0; r < R.n_rows; ++r)
        for (int32_t v = vptr[(size_t)r]; v < vptr[(size_t)r + 1]; ++v) vrow_row[(size_t)v] = (int32_t)r;
    const int64_t tile_rows = VRX_LDS_WAVES * (int64_t)RW;
    L.n_tile = (int)((n_vrows + tile_rows - 1) / tile_rows);
    // Coarse shapes (clone mode: a few hundred variants, 10^5 cells): the (tile, slab) visits
    // are what the work list deals to the CUs, and a visit is not divisible.
    //  * fewer visits than CUs: shorter slabs, until every CU has one (c5 variant pass: ONE tile
    //    of 200 variants x 196 slabs of 1024 cells left 60 CUs idle -> 256 slabs of 784);
    //  * one or two slabs: the rows are spread over as many tiles as make whole rounds of CUs --
    //    the pieces are dealt round-robin to the waves anyway, only the number of tiles changes
    //    (c5 cell pass: 196 full tiles of 1024 cells -> 256 tiles of 782).
    if (n_cu > 0 && env_int("VIREO_LDS_FILL_CUS", 1) != 0) {
        auto spread_tiles = [&]() {  // (tiles must keep >= 4 rows per wave on average)
            const int64_t visits = (int64_t)L.n_tile * L.n_slab, rounds = (visits + n_cu - 1) / n_cu;
            const int64_t nt = rounds * n_cu / L.n_slab;
            if (nt > L.n_tile && nt * VRX_LDS_WAVES * G <= std::max<int64_t>(n_vrows, 1) * 4) L.n_tile = (int)nt;
        };
        if (L.n_slab <= 2) spread_tiles();
        if ((int64_t)L.n_tile * L.n_slab < n_cu) {
            const int64_t want = (n_cu + L.n_tile - 1) / L.n_tile;
            const int64_t sr = std::min<int64_t>(slab_rows, std::max<int64_t>(64, ((R.n_contract + want - 1) / want + 15) / 16 * 16));
            slab_rows = (int)sr;
            L.slab_rows = slab_rows;
            L.n_slab = (int)((R.n_contract + slab_rows - 1) / slab_rows);
            if ((int64_t)L.n_tile * L.n_slab < n_cu) spread_tiles();
        }
    }
    const int64_t n_wave = (int64_t)L.n_tile * VRX_LDS_WAVES;
    // ---- tile position -> piece (-1 = padding position) ---------------------------------
    std::vector<int32_t>& rowmap = L.rowmap;
    rowmap.assign((size_t)(n_wave * RW), -1);
    std::vector<int32_t> order((size_t)n_vrows);
    for (int64_t v = 0; v < n_vrows; ++v) order[(size_t)v] = (int32_t)v;
    if (reorder) {
        auto piece_len = [&](int32_t v) {
            const int32_t r = vrow_row[(size_t)v];
            return (ptr[r + 1] - ptr[r]) / (vptr[(size_t)r + 1] - vptr[(size_t)r]);
        };
        std::stable_sort(order.begin(), order.end(),
                         [&](int32_t a, int32_t b) { return piece_len(a) > piece_len(b); });
    }
    const int64_t n_unit = (n_vrows + G - 1) / G;
    for (int64_t u = 0; u < n_unit; ++u) {
        const int64_t j = u / n_wave, i = u % n_wave;  // stratum j -> round j of the wave
        const int64_t w = reorder && (j & 1) ? n_wave - 1 - i : i;
        for (int g = 0; g < G && u * G + g < n_vrows; ++g)
            rowmap[(size_t)(w * RW + j * G + g)] = order[(size_t)(u * G + g)];
    }
    return VRX_OK;
}

// The word geometry of a stream, as the device builder's kernels take it; the host walk reads the same
// fields (the device pointers are set by the device builder).
static VrxTileArgs tile_args(const TileRows& R, const TileShape& S, const TileLayout& L) {
    constexpr int G = 64 / VRX_LDS_LPE;
    VrxTileArgs A{};
    A.ptr = R.dev.ptr;
    A.idx = R.dev.idx;
    A.val = R.dev.val;
    A.RW = S.RW;
    A.NR = S.RW / G;
    A.G = G;
    A.U = VRX_LDS_U;
    A.n_slab = L.n_slab;
    A.slab_rows = L.slab_rows;
    A.form = S.form;
    // the entry bit that selects the LDS bank half of a 128-B dense row: half (form 1), parity
    // of the slab-local index (variant pass); none for the 256-B rows of the (ad, dp) cell pass
    A.bit_shift = S.form != 0 ? 7 : (S.mode == 0 ? 22 : -1);
    A.xor_partner = 24 / VRX_LDS_LPE;
    // form 1 words carry the LDS address of their half row: the slab starts behind the rings
    A.f1_base = (uint32_t)VRX_LDS_WAVES * VRX_RING * 4u;
    A.pad_word = S.form != 0 ? A.f1_base : 0u;
    A.n_wave = (int64_t)L.n_tile * VRX_LDS_WAVES;
    return A;
}

// Balanced slabs apply to AD/BD words (form 1) of several slabs.  The kernel stages a balanced slab through the
// gather of its precise instances only, and its perm path hard-codes the lane mapping of 16 waves loading at
// most 8 registers each (lane 32 + 4 i + q <- slab-local row 4 * wave + 64 i + q).
static_assert(VRX_LDS_WAVES == 16 && VRX_LDS_PF <= 8,
              "balanced slabs: the perm path of vrx_spmm_lds assumes 16 waves and at most 8 prefetch registers");
static bool balance_applies(const TileRows& R, const TileShape& S, const TileLayout& L) {
    return S.balance && S.form == 1 && L.n_slab > 1 && R.n_contract < ((int64_t)1 << 24) &&
           L.n_vrows < ((int64_t)1 << 31) && (!L.split || env_int("VIREO_BALANCE_SPLIT", 1) != 0);
}

// The rows the greedy and the relabel work on: the stream's rows, or -- rows cut into pieces (heavy-tailed
// data) -- the PIECES, whose entries are copied out as rows of their own (entry k of a row -> piece k % P), so
// that every unit belongs to exactly one tile and is relabelled by that tile's permutation.
struct BalanceUnits {
    const int64_t* ptr;  // row pointer on the host
    DevRows dev;         // the same rows on the device
    int64_t n, nnz, n_contract;
    std::vector<int32_t> tile, tpos;  // tile and tile position of every unit (-1: none)
};

// The greedy of every tile (vrx_balance_tile) on host threads, tiles in parallel: posmap / perm per tile.
static void greedy_tiles(const TileLayout& L, int RW, bool pieces, const BalanceUnits& U, const int32_t* idx,
                         const uint8_t* words, std::vector<int32_t>& posmap, std::vector<int32_t>& perm) {
    const int64_t tile_pos = (int64_t)VRX_LDS_WAVES * RW, slots = (int64_t)L.n_slab * L.slab_rows;
    const int max_block = env_int("VIREO_BALANCE_BLOCK", 64);
    posmap.resize((size_t)(L.n_tile * U.n_contract));
    perm.resize((size_t)(L.n_tile * slots));
    auto unit_of = [&](int32_t v) { return pieces ? v : L.vrow_row[(size_t)v]; };
    std::atomic<int64_t> next_tile{0};  // (tiles cost about the same: first come, first served)
    parallel_chunks(std::min<int64_t>(L.n_tile, balance_threads()), balance_threads(), [&](int64_t, int64_t, int) {
        std::vector<int32_t> rows;
        for (int64_t tl = next_tile++; tl < L.n_tile; tl = next_tile++) {
            rows.clear();
            for (int64_t pos = tl * tile_pos; pos < (tl + 1) * tile_pos; ++pos)
                if (L.rowmap[(size_t)pos] >= 0) rows.push_back(unit_of(L.rowmap[(size_t)pos]));
            vrx_balance_tile(rows.data(), (int64_t)rows.size(), U.ptr, idx, words, U.n_contract, L.n_slab,
                             L.slab_rows, max_block, posmap.data() + tl * U.n_contract, perm.data() + tl * slots);
        }
    });
}

// The greedy on the device (vrx_build.h, vrx_balance_greedy): no entry leaves the GPU.  Prepared by two radix
// sorts and a scan whose key / value buffers (k_*, v_*) the relabel uses afterwards.  *declined: a column deeper
// than 4095 tile rows or a block without room -- the host greedy takes over.
static int greedy_device(const BalanceUnits& U, const TileLayout& L, int RW, VrxBalBlocks blocks, DevBuf<uint64_t>& k_in,
                         DevBuf<uint64_t>& k_out, DevBuf<uint32_t>& v_in, DevBuf<uint32_t>& v_out,
                         DevBuf<int32_t>& d_posmap, DevBuf<int32_t>& perm, hipStream_t s, LapTimer& lap, bool* declined) {
    const int64_t tile_pos = (int64_t)VRX_LDS_WAVES * RW, slots = (int64_t)L.n_slab * L.slab_rows;
    const int64_t nnz = U.nnz, n_contract = U.n_contract;
    const int64_t n_cols_all = (int64_t)L.n_tile * n_contract, n_groups = (int64_t)L.n_tile * blocks.nb;
    DevBuf<int32_t> d_tpos, d_flags;
    DevBuf<uint64_t> ok_in, ok_out;
    DevBuf<uint32_t> d_cptr, d_deg, d_ostart, d_ovals;
    DevBuf<int64_t> d_seg;
    DevBuf<char> tmp;
    const int cbits = bits_for(n_contract), tbits = bits_for((int64_t)L.n_tile + 1), gbits = bits_for(n_groups);
    const unsigned nbe = (unsigned)((nnz + VRX_BLOCK - 1) / VRX_BLOCK);
    const unsigned nbc = (unsigned)((n_cols_all + 1 + VRX_BLOCK - 1) / VRX_BLOCK);
    VRX_HIP(d_tpos.upload(U.tpos.data(), U.tpos.size(), s));
    const int32_t zero2[2] = {0, 0};
    VRX_HIP(d_flags.upload(zero2, 2, s));
    vrx_bal_keys<<<nbe, VRX_BLOCK, 0, s>>>(nnz, U.n, U.dev.ptr, U.dev.idx, U.dev.val, d_tpos.p, (int)tile_pos,
                                           L.n_tile, cbits, k_in.p, v_in.p);
    VRX_HIP(hipGetLastError());
    size_t tmp_bytes = 0, tmp2 = 0, tmp3 = 0;
    VRX_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, k_in.p, k_out.p, v_in.p, v_out.p,
                                               (size_t)nnz, 0, cbits + tbits, s));
    VRX_HIP(ok_in.alloc((size_t)n_cols_all));
    VRX_HIP(ok_out.alloc((size_t)n_cols_all));
    VRX_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, tmp2, ok_in.p, ok_out.p, (size_t)n_cols_all, 0,
                                              cbits + 12 + gbits, s));
    VRX_HIP(d_deg.alloc((size_t)n_cols_all));
    VRX_HIP(d_ostart.alloc((size_t)n_cols_all));
    VRX_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp3, d_deg.p, d_ostart.p, (size_t)n_cols_all, s));
    VRX_HIP(tmp.alloc(std::max(tmp_bytes, std::max(tmp2, tmp3))));
    VRX_HIP(hipcub::DeviceRadixSort::SortPairs(tmp.p, tmp_bytes, k_in.p, k_out.p, v_in.p, v_out.p,
                                               (size_t)nnz, 0, cbits + tbits, s));
    VRX_HIP(d_cptr.alloc((size_t)n_cols_all + 1));
    vrx_bal_cptr<<<nbc, VRX_BLOCK, 0, s>>>(n_cols_all, n_contract, nnz, k_out.p, cbits, d_cptr.p);
    VRX_HIP(hipGetLastError());
    vrx_bal_order_keys<<<nbc, VRX_BLOCK, 0, s>>>(n_cols_all, n_contract, d_cptr.p, L.slab_rows, blocks.bs,
                                                 blocks.nb, cbits, ok_in.p, d_flags.p);
    VRX_HIP(hipGetLastError());
    VRX_HIP(hipcub::DeviceRadixSort::SortKeys(tmp.p, tmp2, ok_in.p, ok_out.p, (size_t)n_cols_all, 0,
                                              cbits + 12 + gbits, s));
    VRX_HIP(d_seg.alloc((size_t)n_groups + 1));
    vrx_bal_groups<<<(unsigned)((n_groups + 1 + VRX_BLOCK - 1) / VRX_BLOCK), VRX_BLOCK, 0, s>>>(
        n_groups, n_cols_all, ok_out.p, 12 + cbits, d_seg.p);
    VRX_HIP(hipGetLastError());
    vrx_bal_degrees<<<nbc, VRX_BLOCK, 0, s>>>(n_cols_all, ok_out.p, cbits, d_deg.p);
    VRX_HIP(hipGetLastError());
    VRX_HIP(hipcub::DeviceScan::ExclusiveSum(tmp.p, tmp3, d_deg.p, d_ostart.p, (size_t)n_cols_all, s));
    uint32_t n_stream = 0;  // the entries that count = first entry of the column behind the last one
    VRX_HIP(hipMemcpyAsync(&n_stream, d_cptr.p + n_cols_all, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    VRX_HIP(d_ovals.alloc((size_t)nnz));
    vrx_bal_stream<<<nbc, VRX_BLOCK, 0, s>>>(n_cols_all, n_contract, ok_out.p, cbits, blocks.nb, d_cptr.p,
                                             v_out.p, d_ostart.p, d_ovals.p);
    VRX_HIP(hipGetLastError());
    VRX_HIP(d_posmap.alloc((size_t)n_cols_all));
    VRX_HIP(perm.alloc((size_t)(L.n_tile * slots)));
    VRX_HIP(hipMemsetAsync(perm.p, 0, (size_t)(L.n_tile * slots) * sizeof(int32_t), s));
    VRX_HIP(hipStreamSynchronize(s));  // (n_stream)
    const size_t lds = (size_t)(tile_pos + 1) * 64 + 2 * VRX_BAL_BATCH * sizeof(uint32_t);
    VRX_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(vrx_balance_greedy),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    vrx_balance_greedy<<<(unsigned)n_groups, 64, lds, s>>>(ok_out.p, d_seg.p, d_ostart.p, d_ovals.p,
                                                          (int64_t)n_stream, n_contract, cbits, L.n_slab,
                                                          L.slab_rows, blocks.bs, blocks.nb, (int)tile_pos,
                                                          d_posmap.p, perm.p, d_flags.p + 1);
    VRX_HIP(hipGetLastError());
    int32_t flags[2] = {0, 0};
    VRX_HIP(hipMemcpyAsync(flags, d_flags.p, sizeof flags, hipMemcpyDeviceToHost, s));
    VRX_HIP(hipStreamSynchronize(s));
    lap("greedy on the device");
    *declined = flags[0] || flags[1];
    if (*declined && lap.on)
        fprintf(stderr, "[vrx build] balanced slabs: device greedy declined (%d, %d)\n", flags[0], flags[1]);
    return VRX_OK;
}

// The greedy on host threads (the specification): the units' indices and one byte of FORM 1 words per entry
// (vrx_build_words) come back from the device.
static int greedy_host(const BalanceUnits& U, const TileLayout& L, int RW, bool pieces, hipStream_t s, LapTimer& lap,
                       std::vector<int32_t>& posmap, std::vector<int32_t>& perm) {
    std::vector<int32_t> h_idx((size_t)U.nnz);
    std::vector<uint8_t> h_words((size_t)U.nnz);
    {
        DevBuf<uint8_t> d_words;
        VRX_HIP(d_words.alloc((size_t)U.nnz));
        vrx_build_words<<<(unsigned)((U.nnz + VRX_BLOCK - 1) / VRX_BLOCK), VRX_BLOCK, 0, s>>>(U.nnz, U.dev.val, d_words.p);
        VRX_HIP(hipGetLastError());
        VRX_HIP(hipMemcpyAsync(h_idx.data(), U.dev.idx, (size_t)U.nnz * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        VRX_HIP(hipMemcpyAsync(h_words.data(), d_words.p, (size_t)U.nnz, hipMemcpyDeviceToHost, s));
        VRX_HIP(hipStreamSynchronize(s));
    }
    lap("download rows");
    greedy_tiles(L, RW, pieces, U, h_idx.data(), h_words.data(), posmap, perm);
    lap("greedy (host threads)");
    return VRX_OK;
}

// VIREO_BALANCE_CHECK=1: the device greedy's result against the specification, bit for bit
static int check_greedy(const DevBuf<int32_t>& d_posmap, const DevBuf<int32_t>& d_perm, const std::vector<int32_t>& posmap,
                        const std::vector<int32_t>& perm, int64_t n_contract, int mode, bool timing, hipStream_t s) {
    std::vector<int32_t> dp(posmap.size()), dq(perm.size());
    VRX_HIP(hipMemcpyAsync(dp.data(), d_posmap.p, dp.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    VRX_HIP(hipMemcpyAsync(dq.data(), d_perm.p, dq.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    VRX_HIP(hipStreamSynchronize(s));
    for (size_t i = 0; i < dp.size(); ++i)
        if (dp[i] != posmap[i]) {
            vrx_set_error("balanced slabs: the device greedy differs from the host's at tile %lld, contracted "
                          "row %lld (%d against %d)", (long long)(i / n_contract), (long long)(i % n_contract),
                          dp[i], posmap[i]);
            return VRX_ERR_UNSUPPORTED;
        }
    if (dq != perm) {
        vrx_set_error("balanced slabs: the device greedy's slab lists differ from the host's");
        return VRX_ERR_UNSUPPORTED;
    }
    if (timing)
        fprintf(stderr, "[vrx build] balanced slabs (mode %d): device greedy == host greedy (%lld columns)\n", mode,
                (long long)dp.size());
    return VRX_OK;
}

// Stage (b)'s result: the relabelled rows the device builder walks instead of the orientation's own, and the
// per-tile permutation that becomes TiledStream::perm
struct BalancedRows {
    DevBuf<int64_t> ptr;    // (rows cut into pieces: the pieces' row pointer ...
    DevBuf<int32_t> iota;   //  ... and the identity as vptr / vrow_row: one piece per row)
    DevBuf<int32_t> idx;
    DevBuf<int2> val;
    DevBuf<int32_t> perm;
};

// Stage (b), balanced slabs: per-tile permutation of the contracted rows, entries relabelled + re-sorted.
// d_vptr: the layout's vptr on the device.
static int balance_slabs(const TileRows& R, const TileShape& S, const TileLayout& L, const int32_t* d_vptr,
                         hipStream_t s, BalancedRows& B, double* seconds) {
    LapTimer lap{s, "balanced slabs (mode " + std::to_string(S.mode) + "):", 28};
    const int64_t nnz = R.nnz, n_contract = R.n_contract;
    const int64_t tile_pos = (int64_t)VRX_LDS_WAVES * S.RW, slots = (int64_t)L.n_slab * L.slab_rows;
    const bool pieces = L.split;
    BalanceUnits U{R.ptr, R.dev, pieces ? L.n_vrows : R.n_rows, nnz, n_contract, {}, {}};
    std::vector<int64_t> pptr;
    DevBuf<int32_t> d_pidx;
    DevBuf<int2> d_pval;
    if (pieces) {
        pptr.assign((size_t)L.n_vrows + 1, 0);
        for (int64_t r = 0; r < R.n_rows; ++r) {
            const int64_t len = R.ptr[r + 1] - R.ptr[r];
            const int32_t v0 = L.vptr[(size_t)r], P = L.vptr[(size_t)r + 1] - v0;
            for (int32_t q = 0; q < P; ++q) pptr[(size_t)(v0 + q) + 1] = (len - q + P - 1) / P;
        }
        for (int64_t v = 0; v < L.n_vrows; ++v) pptr[(size_t)v + 1] += pptr[(size_t)v];
        VRX_HIP(B.ptr.upload(pptr.data(), pptr.size(), s));
        VRX_HIP(d_pidx.alloc((size_t)nnz));
        VRX_HIP(d_pval.alloc((size_t)nnz));
        vrx_build_pieces<<<(unsigned)((nnz + VRX_BLOCK - 1) / VRX_BLOCK), VRX_BLOCK, 0, s>>>(
            nnz, R.n_rows, R.dev.ptr, d_vptr, B.ptr.p, R.dev.idx, R.dev.val, d_pidx.p, d_pval.p);
        VRX_HIP(hipGetLastError());
        U.ptr = pptr.data();
        U.dev = DevRows{B.ptr.p, d_pidx.p, d_pval.p};
    }
    // the tile position of every unit (what both routes of the greedy start from)
    U.tile.assign((size_t)U.n, -1);
    U.tpos.assign((size_t)U.n, -1);
    for (int64_t pos = 0; pos < (int64_t)L.n_tile * tile_pos; ++pos)
        if (L.rowmap[(size_t)pos] >= 0) {
            const int32_t u = pieces ? L.rowmap[(size_t)pos] : L.vrow_row[(size_t)L.rowmap[(size_t)pos]];
            U.tile[(size_t)u] = (int32_t)(pos / tile_pos);
            U.tpos[(size_t)u] = (int32_t)pos;
        }
    DevBuf<int32_t> d_tile_of_row, d_posmap;
    VRX_HIP(d_tile_of_row.upload(U.tile.data(), U.tile.size(), s));
    const VrxBalBlocks blocks = vrx_bal_blocks(L.n_slab, env_int("VIREO_BALANCE_BLOCK", 64));
    const bool check = env_int("VIREO_BALANCE_CHECK", 0) != 0;
    const char* gm = getenv("VIREO_BALANCE_GREEDY");
    const int64_t n_cols_all = (int64_t)L.n_tile * n_contract, n_groups = (int64_t)L.n_tile * blocks.nb;
    bool dev_greedy = !(gm && !strcmp(gm, "host")) && blocks.bs <= 64 &&
                      (tile_pos + 1) * 64 + 2 * VRX_BAL_BATCH * 4 <= 160 * 1024 && tile_pos <= 4095 &&
                      n_cols_all < (int64_t)INT32_MAX && n_groups < ((int64_t)1 << 20) &&
                      (int64_t)L.n_tile * tile_pos < (int64_t)INT32_MAX;
    // (the sort buffers of the greedy's preparation serve the relabel below as well: multi-GB
    //  allocations and releases are what a large build spends its time on)
    DevBuf<uint64_t> k_in, k_out;
    DevBuf<uint32_t> v_in, v_out;
    VRX_HIP(k_in.alloc((size_t)nnz));
    VRX_HIP(k_out.alloc((size_t)nnz));
    VRX_HIP(v_in.alloc((size_t)nnz));
    VRX_HIP(v_out.alloc((size_t)nnz));
    int rc;
    if (dev_greedy) {
        bool declined = false;
        if ((rc = greedy_device(U, L, S.RW, blocks, k_in, k_out, v_in, v_out, d_posmap, B.perm, s, lap, &declined)))
            return rc;
        dev_greedy = !declined;
    }
    if (!dev_greedy || check) {
        std::vector<int32_t> posmap, perm;
        if ((rc = greedy_host(U, L, S.RW, pieces, s, lap, posmap, perm))) return rc;
        if (dev_greedy) {
            if ((rc = check_greedy(d_posmap, B.perm, posmap, perm, n_contract, S.mode, lap.on, s))) return rc;
        } else {
            VRX_HIP(d_posmap.upload(posmap.data(), posmap.size(), s));
            VRX_HIP(B.perm.upload(perm.data(), perm.size(), s));
            VRX_HIP(hipStreamSynchronize(s));  // (the host vectors die here)
        }
    }
    // ---- relabel: key = unit << pbits | position -- as few radix passes as the sizes need
    const unsigned nbe = (unsigned)((nnz + VRX_BLOCK - 1) / VRX_BLOCK);
    const int rbits = bits_for(U.n), pbits = bits_for(std::max<int64_t>(slots, n_contract));
    vrx_build_relabel<<<nbe, VRX_BLOCK, 0, s>>>(nnz, U.n, n_contract, U.dev.ptr, U.dev.idx, d_tile_of_row.p,
                                                d_posmap.p, pbits, k_in.p, v_in.p);
    VRX_HIP(hipGetLastError());
    size_t tmp_bytes = 0;
    VRX_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, k_in.p, k_out.p, v_in.p, v_out.p,
                                               (size_t)nnz, 0, pbits + rbits, s));
    DevBuf<char> tmp;
    VRX_HIP(tmp.alloc(tmp_bytes));
    VRX_HIP(hipcub::DeviceRadixSort::SortPairs(tmp.p, tmp_bytes, k_in.p, k_out.p, v_in.p, v_out.p,
                                               (size_t)nnz, 0, pbits + rbits, s));
    VRX_HIP(B.idx.alloc((size_t)nnz));
    VRX_HIP(B.val.alloc((size_t)nnz));
    vrx_build_relabel_gather<<<nbe, VRX_BLOCK, 0, s>>>(nnz, k_out.p, v_out.p, U.dev.val, pbits, B.idx.p, B.val.p);
    VRX_HIP(hipGetLastError());
    if (pieces) {  // the stream's rows are the pieces now: one piece per "row", nothing left to cut
        std::vector<int32_t> iota((size_t)L.n_vrows + 1);
        for (int64_t v = 0; v <= L.n_vrows; ++v) iota[(size_t)v] = (int32_t)v;
        VRX_HIP(B.iota.upload(iota.data(), iota.size(), s));
    }
    VRX_HIP(hipStreamSynchronize(s));
    lap("upload + relabel + sort");
    *seconds = LapTimer::now() - lap.begin;
    return VRX_OK;
}

// FORM 1 value field: the top 14 bits of the IEEE double (sign, exponent, 2 mantissa bits) of every chunk of
// the count (vrx_form1_chunk: 9 = 8 + 1, ...)
static void push_value(std::vector<uint32_t>& out, int64_t v, uint32_t off) {
    while (v != 0) {
        const int64_t c = vrx_form1_chunk(v);
        const double d = (double)c;
        uint64_t bits;
        std::memcpy(&bits, &d, 8);
        out.push_back((uint32_t)(bits >> 50) << 18 | off);
        v -= c;
    }
}

// Stage (c), the host walk: one wave's stream walks its RW pieces slab by slab, records the (slab, round)
// offsets in bw and appends the words to `dst`; returns its length, or -1 past 2^31 words.  Waves are independent.
static int64_t walk_wave(const TileRows& R, const TileLayout& L, const VrxTileArgs& A, int64_t w, int32_t* bw,
                         std::vector<uint32_t>& dst) {
    constexpr int G = 64 / VRX_LDS_LPE;
    const int RW = A.RW, NR = A.NR, U = A.U, form = A.form, bit_shift = A.bit_shift;
    const int64_t* ptr = R.ptr;
    const int32_t* idx = R.idx;
    const int2* val = R.val;
    dst.reserve((size_t)((double)R.nnz / (double)A.n_wave * 2.3) + 1024);
    const int32_t* rm = L.rowmap.data() + w * RW;
    std::vector<int64_t> cursor((size_t)RW);
    std::vector<uint32_t> segw[G];
    for (int c = 0; c < RW; ++c) cursor[(size_t)c] = rm[c] >= 0 ? ptr[L.vrow_row[(size_t)rm[c]]] : 0;
    int64_t rel = 0;
    for (int sl = 0; sl < A.n_slab; ++sl) {
        const int64_t lim = (int64_t)(sl + 1) * A.slab_rows, base = (int64_t)sl * A.slab_rows;
        for (int r = 0; r < NR; ++r) {
            if (rel >= INT32_MAX - 4096) return -1;
            // the groups' segments of this slab
            int64_t s_lo[G], s_hi[G], s_step[G];
            for (int g = 0; g < G; ++g) {
                const int32_t v = rm[r * G + g];
                s_lo[g] = s_hi[g] = 0;
                s_step[g] = 1;
                if (v >= 0) {
                    const int32_t row = L.vrow_row[(size_t)v];
                    int64_t hi = cursor[(size_t)(r * G + g)];
                    const int64_t seg = hi, stop = ptr[row + 1];
                    while (hi < stop && idx[hi] < lim) ++hi;
                    cursor[(size_t)(r * G + g)] = hi;
                    // this piece's share of the row's slab segment [seg, hi)
                    s_step[g] = L.vptr[(size_t)row + 1] - L.vptr[(size_t)row];
                    s_lo[g] = seg + ((int64_t)(v - L.vptr[(size_t)row]) + sl) % s_step[g];
                    s_hi[g] = hi;
                }
            }
            int64_t longest = 0;
            for (int g = 0; g < G; ++g) {
                std::vector<uint32_t>& sw = segw[g];
                sw.clear();
                for (int64_t e = s_lo[g]; e < s_hi[g]; e += s_step[g]) {
                    if (form == 0) {
                        sw.push_back(((uint32_t)(idx[e] - base) << 22) |
                                     ((uint32_t)val[e].x << 11) | (uint32_t)val[e].y);
                    } else {
                        const uint32_t at = A.f1_base + (uint32_t)(idx[e] - base) * 256u;
                        push_value(sw, val[e].x, at);
                        push_value(sw, (int64_t)val[e].y - val[e].x, at + 128u);
                    }
                }
                longest = std::max<int64_t>(longest, (int64_t)sw.size());
            }
            // Bank conflicts.  The dense rows are 128 B (ID_prob rows; the AD / BD half
            // rows), so the LDS bank of a slice depends on one address bit of the entry
            // (index parity / half).  ds_read_b128 serves lane groups {0,3,5,6}, {1,2,4,7}
            // (+8) together, and the two groups with the same slice rotation (g & 1) collide
            // whenever that bit agrees.  The order of a segment's entries is free, and the
            // zero words that pad a segment to the round's length can point at either
            // parity: group P walks its bit-0 entries (then bit-0 padding) up to a split
            // position z and its bit-1 entries after it, its partner Q the other way round.
            // z exists whenever the pair's bit-0 entries and its bit-1 entries each fit
            // into the round, i.e. almost always.
            if (bit_shift >= 0) {
                for (int g = 0; g < G; ++g) {
                    // the group that shares g's rotation inside g's service group holds
                    // lanes ^ 24 (ds_read_b128: {0-3,12-15,20-27}, {4-11,16-19,28-31}, +32)
                    const int q = g ^ A.xor_partner;
                    if (q < g) continue;
                    std::vector<uint32_t> part[2][2];  // [P / Q][bit]
                    for (int m = 0; m < 2; ++m)
                        for (uint32_t wd : segw[m ? q : g]) part[m][(wd >> bit_shift) & 1u].push_back(wd);
                    const int64_t p0 = (int64_t)part[0][0].size(), p1 = (int64_t)part[0][1].size();
                    const int64_t q0 = (int64_t)part[1][0].size(), q1 = (int64_t)part[1][1].size();
                    const int64_t zlo = std::max(p0, q1), zhi = std::min(longest - p1, longest - q0);
                    if (zlo > zhi) {  // does not fit: opposite orders, as far as that goes
                        segw[g] = part[0][0];
                        segw[g].insert(segw[g].end(), part[0][1].begin(), part[0][1].end());
                        segw[q] = part[1][1];
                        segw[q].insert(segw[q].end(), part[1][0].begin(), part[1][0].end());
                        continue;
                    }
                    const int64_t z = (zlo + zhi) / 2;
                    const uint32_t pad0 = A.pad_word, pad1 = pad0 | 1u << bit_shift;
                    auto lay = [&](std::vector<uint32_t>& out, const std::vector<uint32_t>& first,
                                   uint32_t pad_first, const std::vector<uint32_t>& rest,
                                   uint32_t pad_rest) {
                        out = first;
                        out.resize((size_t)z, pad_first);
                        out.insert(out.end(), rest.begin(), rest.end());
                        out.resize((size_t)longest, pad_rest);
                    };
                    lay(segw[g], part[0][0], pad0, part[0][1], pad1);
                    lay(segw[q], part[1][1], pad1, part[1][0], pad0);
                }
            }
            // offset | entries in the last trip (0 = full): the kernel skips the padding
            bw[(int64_t)sl * NR + r] = (int32_t)(rel | (longest % U));
            longest = (longest + U - 1) / U * U;
            dst.resize((size_t)(rel + longest * G));
            for (int64_t j = 0; j < longest; ++j)
                for (int g = 0; g < G; ++g)  // padding: value 0 (form 1: at the slab's first row)
                    dst[(size_t)(rel + vrx_trip_slot(j, g, G, U, form))] =
                        j < (int64_t)segw[g].size() ? segw[g][(size_t)j] : A.pad_word;
            rel += longest * G;  // (a multiple of 64 words: streams stay 16-B aligned)
        }
    }
    bw[(int64_t)A.n_slab * NR] = (int32_t)rel;
    return rel;
}

// Stage (e), what both builders end with: the waves' offsets, the padding guard, the words (`emit(total,
// wave_start)` fills t.ent), the boundaries (bnd: on the host, or already in t.bnd), the row tables and the
// work list.  A stream the guard rejects stays not ready.
template <class Emit>
static int finish_stream(TiledStream& t, const TileShape& S, const TileLayout& L, const VrxTileArgs& A,
                         const std::vector<int64_t>& wave_len, std::vector<int32_t>& bnd, bool bnd_on_device,
                         int n_cu, int64_t nnz, hipStream_t s, Emit&& emit) {
    const int64_t n_wave = A.n_wave;
    std::vector<int64_t> wave_start((size_t)n_wave);
    int64_t total = 0, longest_wave = 0;
    for (int64_t w = 0; w < n_wave; ++w) {
        wave_start[(size_t)w] = total;
        total += wave_len[(size_t)w];
        longest_wave = std::max(longest_wave, wave_len[(size_t)w]);
    }
    // Guard: past VIREO_LDS_MAX_PAD stream words per entry (default 3; padding x imbalance of
    // the slowest wave) the global-gather pass is the faster one, so no stream is kept.
    t.pad_ratio = nnz > 0 ? (double)total / (double)nnz : 0.0;
    t.imbalance = total > 0 ? (double)longest_wave * (double)n_wave / (double)total : 1.0;
    if (S.guard && t.pad_ratio * std::max(1.0, t.imbalance / 1.5) > (double)env_int("VIREO_LDS_MAX_PAD", 3))
        return VRX_OK;
    // the waves' streams back to back (+ slack for the last dwordx4 refill)
    VRX_HIP(t.ent.alloc((size_t)total + 8));
    VRX_HIP(hipMemsetAsync(t.ent.p + total, 0, 8 * sizeof(uint32_t), s));
    VRX_HIP(t.wave_start.upload(wave_start.data(), wave_start.size(), s));
    int rc = emit(total, wave_start);
    if (rc) return rc;
    if (bnd_on_device)
        VRX_HIP(hipMemcpyAsync(bnd.data(), t.bnd.p, bnd.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    else
        VRX_HIP(t.bnd.upload(bnd.data(), bnd.size(), s));
    VRX_HIP(t.rowmap.upload(L.rowmap.data(), L.rowmap.size(), s));
    if (t.split) {
        VRX_HIP(t.vptr.upload(L.vptr.data(), L.vptr.size(), s));
        VRX_HIP(t.split_rows.upload(L.split_rows.data(), L.split_rows.size(), s));
    }
    VRX_HIP(hipStreamSynchronize(s));
    rc = plan_items(t, bnd.data(), n_cu, L.rowmap.data(), s);
    if (rc) return rc;
    t.ready = true;
    return VRX_OK;
}

static int stream_on_host(TiledStream& t, const TileRows& R, const TileShape& S, const TileLayout& L,
                          const VrxTileArgs& A, int n_cu, hipStream_t s) {
    const int64_t n_wave = A.n_wave, per_wave = (int64_t)A.n_slab * A.NR + 1;
    std::vector<int64_t> wave_len((size_t)n_wave, 0);
    std::vector<int32_t> bnd((size_t)(n_wave * per_wave));
    std::vector<std::vector<uint32_t>> wave_words((size_t)n_wave);
    std::atomic<bool> too_long{false};
    parallel_chunks(n_wave, host_threads(), [&](int64_t b0, int64_t e0, int) {
        for (int64_t w = b0; w < e0 && !too_long; ++w) {
            wave_len[(size_t)w] = walk_wave(R, L, A, w, bnd.data() + w * per_wave, wave_words[(size_t)w]);
            if (wave_len[(size_t)w] < 0) too_long = true;
        }
    });
    if (too_long) {
        vrx_set_error("tiled stream: wave stream >= 2^31 words");
        return VRX_ERR_UNSUPPORTED;
    }
    return finish_stream(t, S, L, A, wave_len, bnd, false, n_cu, R.nnz, s,
                         [&](int64_t total, const std::vector<int64_t>& wave_start) {
        std::unique_ptr<uint32_t[]> all(new uint32_t[(size_t)total + 1]);
        parallel_chunks(n_wave, host_threads(), [&](int64_t b0, int64_t e0, int) {
            for (int64_t w = b0; w < e0; ++w) {
                std::vector<uint32_t>& src = wave_words[(size_t)w];
                if (!src.empty())
                    std::memcpy(all.get() + wave_start[(size_t)w], src.data(), src.size() * sizeof(uint32_t));
                std::vector<uint32_t>().swap(src);
            }
        });
        VRX_HIP(hipMemcpyAsync(t.ent.p, all.get(), (size_t)total * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        VRX_HIP(hipStreamSynchronize(s));
        return VRX_OK;
    });
}

// Stage (d), the device builder's walk (vrx_build.h): every segment's bounds and round length
// (vrx_build_count), the waves' (slab, round) offsets into t.bnd and their lengths (vrx_build_offsets);
// the words follow in stage (e) (vrx_build_fill).
static int stream_on_device(TiledStream& t, const TileRows& R, const TileShape& S, const TileLayout& L,
                            VrxTileArgs A, int n_cu, hipStream_t s, double* balance_seconds) {
    VRX_REQUIRE(R.nnz < (int64_t)UINT32_MAX, "tiled stream: more than 2^32 - 1 entries");
    DevBuf<int32_t> d_rowmap, d_vptr, d_vrow, rlen, d_too;
    DevBuf<uint32_t> seg_lo, seg_hi;  // entry offsets (< 2^32: device_build's limit)
    DevBuf<int64_t> d_wlen;
    VRX_HIP(d_rowmap.upload(L.rowmap.data(), L.rowmap.size(), s));
    VRX_HIP(d_vptr.upload(L.vptr.data(), L.vptr.size(), s));
    VRX_HIP(d_vrow.upload(L.vrow_row.data(), L.vrow_row.size(), s));
    A.rowmap = d_rowmap.p;
    A.vptr = d_vptr.p;
    A.vrow_row = d_vrow.p;
    BalancedRows B;
    if (balance_applies(R, S, L)) {
        const int rc = balance_slabs(R, S, L, d_vptr.p, s, B, balance_seconds);
        if (rc) return rc;
        A.idx = B.idx.p;
        A.val = B.val.p;
        if (L.split) {
            A.ptr = B.ptr.p;
            A.vptr = A.vrow_row = B.iota.p;
        }
        t.perm = std::move(B.perm);
    }
    const int64_t n_wave = A.n_wave, nsr = (int64_t)A.n_slab * A.NR, per_wave = nsr + 1;
    const int64_t n_pos = n_wave * A.n_slab * A.RW;
    VRX_REQUIRE(n_pos < INT32_MAX * (int64_t)VRX_BLOCK, "tiled stream: too many segments");
    VRX_HIP(seg_lo.alloc((size_t)n_pos));
    VRX_HIP(seg_hi.alloc((size_t)n_pos));
    VRX_HIP(rlen.alloc((size_t)(n_wave * nsr)));
    VRX_HIP(d_too.alloc(1));
    VRX_HIP(hipMemsetAsync(d_too.p, 0, sizeof(int32_t), s));
    VRX_HIP(t.bnd.alloc((size_t)(n_wave * per_wave)));
    VRX_HIP(d_wlen.alloc((size_t)n_wave));
    vrx_build_count<<<(unsigned)((n_pos + VRX_BLOCK - 1) / VRX_BLOCK), VRX_BLOCK, 0, s>>>(A, seg_lo.p, seg_hi.p, rlen.p);
    VRX_HIP(hipGetLastError());
    vrx_build_offsets<<<(unsigned)((n_wave + VRX_BLOCK - 1) / VRX_BLOCK), VRX_BLOCK, 0, s>>>(A, rlen.p, t.bnd.p,
                                                                                            d_wlen.p, d_too.p);
    VRX_HIP(hipGetLastError());
    std::vector<int64_t> wave_len((size_t)n_wave);
    int32_t h_too = 0;
    VRX_HIP(hipMemcpyAsync(wave_len.data(), d_wlen.p, (size_t)n_wave * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    VRX_HIP(hipMemcpyAsync(&h_too, d_too.p, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    VRX_HIP(hipStreamSynchronize(s));
    if (h_too) {
        vrx_set_error("tiled stream: wave stream >= 2^31 words");
        return VRX_ERR_UNSUPPORTED;
    }
    std::vector<int32_t> bnd((size_t)(n_wave * per_wave));
    return finish_stream(t, S, L, A, wave_len, bnd, true, n_cu, R.nnz, s,
                         [&](int64_t, const std::vector<int64_t>&) {
        const int64_t n_fill = n_wave * nsr * (A.G / 2);
        VRX_REQUIRE(n_fill < INT32_MAX * (int64_t)VRX_BLOCK, "tiled stream: too many rounds");
        vrx_build_fill<<<(unsigned)((n_fill + VRX_BLOCK - 1) / VRX_BLOCK), VRX_BLOCK, 0, s>>>(
            A, seg_lo.p, seg_hi.p, rlen.p, t.bnd.p, t.wave_start.p, t.ent.p);
        VRX_HIP(hipGetLastError());
        return VRX_OK;
    });
}

// One orientation's tiled stream: (a) the layout, then on the host (c) the walk, or on the device (b) balanced
// slabs where they apply and (d) the count, and (e) the shared finish.  All or nothing: o.tiled becomes the
// new stream only when it is ready; a stream the guard rejects, or a failed build, leaves a default (not
// ready, unbalanced) TiledStream.  *balance_seconds: what stage (b) took (untouched without it).
static int build_tiled(Orient& o, const TileRows& R, const TileShape& S, int n_cu, hipStream_t s,
                       double* balance_seconds = nullptr) {
    o.tiled = TiledStream();
    TileLayout L;
    int rc = tile_layout(L, R, S, n_cu);
    if (rc) return rc;
    TiledStream t;
    t.virt = R.virt;
    t.n_contract = R.n_contract;
    t.form = S.form;
    t.rw = S.RW;
    t.slab_rows = L.slab_rows;
    t.n_slab = L.n_slab;
    t.n_tile = L.n_tile;
    t.n_vrows = L.n_vrows;
    t.split = L.split;
    t.n_split = (int64_t)L.split_rows.size();
    const VrxTileArgs A = tile_args(R, S, L);
    double sec = 0.0;
    rc = R.dev.ptr ? stream_on_device(t, R, S, L, A, n_cu, s, &sec) : stream_on_host(t, R, S, L, A, n_cu, s);
    if (balance_seconds) *balance_seconds = sec;
    if (rc == VRX_OK && t.ready) o.tiled = std::move(t);
    return rc;
}

// Rows per wave of the cell pass.  The (tile, slab) visits of a pass are dealt to one workgroup
// per CU (plan_items); a visit is not divisible, so with one or two slabs (few variants: clone
// mode) the busiest CU gets ceil(visits / CUs) of them, and the shorter tile wins when that
// rounds up less (200 k cells, one slab: 261 tiles of 768 rows = 2 visits on the busiest CU,
// 391 tiles of 512 rows = 2 shorter ones).  (build_tiled then spreads the rows over whole
// rounds of CUs, VIREO_LDS_FILL_CUS.)
static int pick_rw_cell(int64_t n_var, int64_t n_cell, int n_cu, int cell_form) {
    const int tall = cell_form == 1 ? VRX_LDS_RW_CELL : VRX_LDS_RW_CELL_PAIR;
    const int slab = VRX_LDS_SLAB_BYTES / 256;
    const int n_slab_c = (int)((n_var + slab - 1) / slab);
    auto cost = [&](int rw) {  // visits of the busiest CU x rows per wave
        const int64_t tiles = (n_cell + VRX_LDS_WAVES * (int64_t)rw - 1) / (VRX_LDS_WAVES * (int64_t)rw);
        const int64_t cus = std::max(1, n_cu);
        return (double)((tiles * n_slab_c + cus - 1) / cus) * rw;
    };
    return n_slab_c <= 2 && cost(VRX_LDS_RW_CELL_SHORT) < cost(tall) ? VRX_LDS_RW_CELL_SHORT : tall;
}

// Which stream words the LDS-resident passes use.  Single-valued AD / BD words (cell form 1,
// variant form 3) cost ~1.56x less per word than (ad, dp) pair words (c3: 0.39 vs 0.51 ms at
// 1.2 words per entry) and hold any count, but a count with more than three significant bits
// takes several words (45 = 40 + 5): deep data -- clone mode, DP ~ Poisson(50), 2.65 words per
// entry -- is better served by one pair word per entry as long as the counts fit its 11 bits.
// The words per entry are estimated from every 61st entry.  VIREO_CELL_FORM / VIREO_VAR_FORM
// force a form.
struct StreamForms {
    int cell, var;   // cell pass: 1 AD/BD, 0 pairs; variant pass: 3 AD/BD virtual rows, 0 pairs
    bool auto_pair;  // pairs chosen by the estimate: fall back to AD/BD when a count is >= 2048
};
static int pick_forms(int64_t nnz, const int32_t* ad, const int32_t* dp, StreamForms* out) {
    int64_t words = 0, seen = 0;
    for (int64_t e = 0; e < nnz; e += 61) {
        const int64_t a = ad[e], d = dp[e];
        if (a < 0 || d < a) continue;  // (rejected by the validation that follows)
        words += vrx_form1_words(a) + vrx_form1_words(d - a);
        ++seen;
    }
    const double wpe = seen ? (double)words / (double)seen : 1.0;
    const bool pairs = wpe > (double)env_int("VIREO_PAIR_WORDS_X100", 156) / 100.0;
    StreamForms f;
    f.cell = env_int("VIREO_CELL_FORM", pairs ? 0 : 1);
    f.var = env_int("VIREO_VAR_FORM", pairs ? 0 : 3);
    f.auto_pair = pairs && !getenv("VIREO_CELL_FORM") && !getenv("VIREO_VAR_FORM");
    if (f.cell != 0 && f.cell != 1) {
        vrx_set_error("vrx_problem_create: VIREO_CELL_FORM=%d (0: pair words, 1: AD / BD words)", f.cell);
        return VRX_ERR_ARG;
    }
    if (f.var != 0 && f.var != 3) {
        vrx_set_error("vrx_problem_create: VIREO_VAR_FORM=%d (0: pair words, 3: AD / BD virtual rows)", f.var);
        return VRX_ERR_ARG;
    }
    *out = f;
    return VRX_OK;
}

// once the largest count is known: the estimate chose pair words but a count does not fit their 11 bits --
// AD/BD words after all
static StreamForms settle_forms(StreamForms f, int32_t max_count) {
    return max_count >= 2048 && f.auto_pair ? StreamForms{1, 3, false} : f;
}

// narrowest entry format that holds the counts and the contracted index (VIREO_ENTRY_FMT may only widen it)
static int pick_fmt(int32_t max_count, int64_t n_contract) {
    int f = VRX_FMT_WIDE;
    if (max_count < (1 << 16)) f = VRX_FMT_P64;
    if (max_count < 64 && n_contract <= (1 << 20)) f = VRX_FMT_P32;
    const int forced = env_int("VIREO_ENTRY_FMT", -1);
    return forced >= f && forced <= VRX_FMT_WIDE ? forced : f;
}

// what both builders' validations report: kind 1 = colptr, 3 = a negative count, else the row indices
static int input_error(int kind, int64_t col) {
    if (kind == 1)
        vrx_set_error("vrx_problem_create: colptr not monotone at column %lld", (long long)col);
    else if (kind == 3)
        vrx_set_error("vrx_problem_create: negative count in column %lld", (long long)col);
    else
        vrx_set_error("vrx_problem_create: row indices of column %lld not strictly increasing / out of range",
                      (long long)col);
    return VRX_ERR_ARG;
}

// What problem_create2 settles for both builders: the stream forms the counts suggest, VIREO_LDS (0 / 1: the
// LDS-resident passes off / on, 1 without the padding guard), the sizes from which they pay off, slab heights
struct BuildPlan {
    StreamForms forms;
    int lds;
    int64_t min_nnz_cell, min_nnz_var;
    int slab_cell;
};

// The device builder's copy of the input: the merged CSC arrays, validated, and the variant-major rows
// transposed from them (+ the row pointer on the host)
struct DeviceInput {
    DevBuf<int64_t> colptr, rptr;
    DevBuf<int32_t> row, ad, dp, ecol, ridx;
    DevBuf<int2> cval, rval;
    std::vector<int64_t> h_rptr;
};

// upload + validation (vrx_build_validate): p->n_vars and the largest count
static int upload_validate(vrx_problem* p, const int64_t* colptr, const int32_t* rowidx, const int32_t* ad,
                           const int32_t* dp, DeviceInput& D, int32_t* max_count) {
    const int64_t nnz = p->nnz, n_var = p->n_var, n_cell = p->n_cell;
    hipStream_t s = p->stream;
    for (int64_t c = 0; c < n_cell; ++c)
        if (colptr[c + 1] < colptr[c]) return input_error(1, c);
    DevBuf<int32_t> d_nvars, d_status;
    VRX_HIP(D.colptr.upload(colptr, (size_t)n_cell + 1, s));
    VRX_HIP(D.row.upload(rowidx, (size_t)nnz, s));
    VRX_HIP(D.ad.upload(ad, (size_t)nnz, s));
    VRX_HIP(D.dp.upload(dp, (size_t)nnz, s));
    VRX_HIP(D.ecol.alloc((size_t)nnz));
    VRX_HIP(d_nvars.alloc((size_t)n_cell));
    VRX_HIP(hipMemsetAsync(d_nvars.p, 0, (size_t)n_cell * sizeof(int32_t), s));
    const int32_t st0[3] = {INT32_MAX, 0, 0};
    VRX_HIP(d_status.upload(st0, 3, s));
    vrx_build_validate<<<(unsigned)((nnz + VRX_BLOCK - 1) / VRX_BLOCK), VRX_BLOCK, 0, s>>>(
        nnz, n_var, n_cell, D.colptr.p, D.row.p, D.ad.p, D.dp.p, D.ecol.p, d_nvars.p, d_status.p);
    VRX_HIP(hipGetLastError());
    int32_t st[3];
    p->n_vars.assign((size_t)n_cell, 0);
    VRX_HIP(hipMemcpyAsync(st, d_status.p, sizeof st, hipMemcpyDeviceToHost, s));
    VRX_HIP(hipMemcpyAsync(p->n_vars.data(), d_nvars.p, (size_t)n_cell * sizeof(int32_t),
                           hipMemcpyDeviceToHost, s));
    VRX_HIP(hipStreamSynchronize(s));
    if (st[0] != INT32_MAX) return input_error(st[1], st[0]);
    *max_count = st[2];
    return VRX_OK;
}

// transposition (stable radix sort of (variant, entry)) and the packed entry arrays of both orientations (no
// segment tables: the LDS-resident passes serve every K)
static int transpose_pack(vrx_problem* p, DeviceInput& D, int32_t max_count) {
    const int64_t nnz = p->nnz, n_var = p->n_var, n_cell = p->n_cell;
    hipStream_t s = p->stream;
    const unsigned nb = (unsigned)((nnz + VRX_BLOCK - 1) / VRX_BLOCK);
    DevBuf<uint32_t> keys_in, keys_out, vals_in, vals_out;
    VRX_HIP(keys_in.alloc((size_t)nnz));
    VRX_HIP(keys_out.alloc((size_t)nnz));
    VRX_HIP(vals_in.alloc((size_t)nnz));
    VRX_HIP(vals_out.alloc((size_t)nnz));
    vrx_build_iota_keys<<<nb, VRX_BLOCK, 0, s>>>(nnz, D.row.p, keys_in.p, vals_in.p);
    VRX_HIP(hipGetLastError());
    {
        const int bits = bits_for(n_var);
        size_t tmp_bytes = 0;
        VRX_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, keys_in.p, keys_out.p, vals_in.p,
                                                   vals_out.p, (size_t)nnz, 0, bits, s));
        DevBuf<char> tmp;
        VRX_HIP(tmp.alloc(tmp_bytes));
        VRX_HIP(hipcub::DeviceRadixSort::SortPairs(tmp.p, tmp_bytes, keys_in.p, keys_out.p, vals_in.p,
                                                   vals_out.p, (size_t)nnz, 0, bits, s));
        VRX_HIP(hipStreamSynchronize(s));
    }
    keys_in.release();
    vals_in.release();
    VRX_HIP(D.rptr.alloc((size_t)n_var + 1));
    vrx_build_rptr<<<(unsigned)((n_var + 1 + VRX_BLOCK - 1) / VRX_BLOCK), VRX_BLOCK, 0, s>>>(
        n_var, nnz, keys_out.p, D.rptr.p);
    VRX_HIP(hipGetLastError());
    VRX_HIP(D.ridx.alloc((size_t)nnz));
    VRX_HIP(D.rval.alloc((size_t)nnz));
    VRX_HIP(D.cval.alloc((size_t)nnz));
    vrx_build_gather<<<nb, VRX_BLOCK, 0, s>>>(nnz, vals_out.p, D.ecol.p, D.ad.p, D.dp.p, D.ridx.p,
                                              D.rval.p, D.cval.p);
    VRX_HIP(hipGetLastError());
    D.h_rptr.resize((size_t)n_var + 1);
    VRX_HIP(hipMemcpyAsync(D.h_rptr.data(), D.rptr.p, D.h_rptr.size() * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    VRX_HIP(hipStreamSynchronize(s));
    keys_out.release();
    vals_out.release();
    D.ecol.release();
    D.ad.release();
    D.dp.release();
    auto pack = [&](Orient& o, int64_t n_rows, int64_t n_contract, const int32_t* d_idx, const int2* d_val) {
        o.n_rows = n_rows;
        o.n_contract = n_contract;
        o.nnz = nnz;
        o.fmt = pick_fmt(max_count, n_contract);
        o.n_tiles = 1;
        o.n_seg = 0;
        o.n_multi = o.n_slots = 0;
        VRX_HIP(o.ent.alloc((size_t)nnz * (o.fmt + 1)));
        vrx_build_pack<<<nb, VRX_BLOCK, 0, s>>>(nnz, o.fmt, d_idx, d_val, o.ent.p);
        VRX_HIP(hipGetLastError());
        return VRX_OK;
    };
    int rc;
    if ((rc = pack(p->by_cell, n_cell, n_var, D.row.p, D.cval.p))) return rc;
    return pack(p->by_var, n_var, n_cell, D.ridx.p, D.rval.p);
}

// The variant pass on virtual rows (vrx_build.h, vrx_virt_count / vrx_virt_fill): their row pointer on both
// sides, their entries on the device
struct VirtualRows {
    DevBuf<int64_t> ptr;
    DevBuf<int32_t> idx;
    DevBuf<int2> val;
    std::vector<int64_t> h_ptr;
    int64_t nnz = 0;
};

static int virtual_rows(const vrx_problem* p, const DeviceInput& D, VirtualRows& V) {
    const int64_t n_var = p->n_var;
    hipStream_t s = p->stream;
    DevBuf<int64_t> d_cnt;
    VRX_HIP(d_cnt.alloc((size_t)(2 * n_var)));
    const unsigned nbv = (unsigned)((n_var + VRX_BLOCK - 1) / VRX_BLOCK);
    vrx_virt_count<<<nbv, VRX_BLOCK, 0, s>>>(n_var, D.rptr.p, D.ridx.p, D.rval.p, d_cnt.p);
    VRX_HIP(hipGetLastError());
    V.h_ptr.assign((size_t)(2 * n_var + 1), 0);
    VRX_HIP(hipMemcpyAsync(V.h_ptr.data() + 1, d_cnt.p, (size_t)(2 * n_var) * sizeof(int64_t),
                           hipMemcpyDeviceToHost, s));
    VRX_HIP(hipStreamSynchronize(s));
    for (int64_t r = 0; r < 2 * n_var; ++r) V.h_ptr[(size_t)r + 1] += V.h_ptr[(size_t)r];
    V.nnz = V.h_ptr[(size_t)(2 * n_var)];
    VRX_HIP(V.ptr.upload(V.h_ptr.data(), V.h_ptr.size(), s));
    VRX_HIP(V.idx.alloc((size_t)std::max<int64_t>(V.nnz, 1)));
    VRX_HIP(V.val.alloc((size_t)std::max<int64_t>(V.nnz, 1)));
    vrx_virt_fill<<<nbv, VRX_BLOCK, 0, s>>>(n_var, D.rptr.p, D.ridx.p, D.rval.p, V.ptr.p, V.idx.p, V.val.p);
    VRX_HIP(hipGetLastError());
    return VRX_OK;
}

// The two orientations' streams are independent: the variant orientation is built by a second host thread on
// a stream of its own while this one builds the cell orientation (their host halves -- layout, work list --
// and their device halves -- the greedy of balanced slabs is a latency-bound kernel on half the CUs --
// overlap).  Not for problems whose two sets of transient buffers would not fit together.
static int build_both_streams(vrx_problem* p, const TileRows& cell_rows, const TileShape& cell_shape,
                              const TileRows& var_rows, const TileShape& var_shape, LapTimer& lap,
                              double* balance_seconds) {
    hipStream_t s = p->stream;
    double sec_cell = 0.0, sec_var = 0.0;
    auto build_var = [&](hipStream_t sv) -> int {
        const int rcv = build_tiled(p->by_var, var_rows, var_shape, p->n_cu, sv, &sec_var);
        if (rcv) return rcv;
        return hipStreamSynchronize(sv) == hipSuccess ? VRX_OK : VRX_ERR_HIP;
    };
    VRX_HIP(hipStreamSynchronize(s));  // (the rows both builds read are complete)
    const bool concurrent = env_int("VIREO_BUILD_CONCURRENT", 1) != 0 &&
                            p->nnz < (int64_t)env_int("VIREO_BUILD_CONCURRENT_MAX_MNNZ", 1000) * 1000000;
    std::thread var_thread;
    int rc_var = VRX_OK;
    std::string err_var;
    hipStream_t s2 = nullptr;
    struct StreamGuard {  // (destroyed after the thread that uses it has been joined: declared before its guard)
        hipStream_t& st;
        ~StreamGuard() {
            if (st) (void)hipStreamDestroy(st);
        }
    } s2_guard{s2};
    if (concurrent) {
        VRX_HIP(hipStreamCreateWithFlags(&s2, hipStreamNonBlocking));
        const int dev_id = p->device;
        var_thread = std::thread([&, dev_id] {
            if (hipSetDevice(dev_id) != hipSuccess) {
                rc_var = VRX_ERR_HIP;
                err_var = "hipSetDevice failed on the variant orientation's build thread";
                return;
            }
            try {
                rc_var = build_var(s2);
                if (rc_var) err_var = vrx_last_error();
            } catch (const std::exception& e) {  // (a throw must not leave a thread)
                rc_var = VRX_ERR_NOMEM;
                err_var = std::string("variant orientation's build: ") + e.what();
            }
        });
    }
    struct JoinGuard {  // (an early return must not leave the thread running on dying buffers)
        std::thread& t;
        ~JoinGuard() {
            if (t.joinable()) t.join();
        }
    } var_guard{var_thread};
    const int rc = build_tiled(p->by_cell, cell_rows, cell_shape, p->n_cu, s, &sec_cell);
    lap("cell stream");
    if (concurrent) {
        var_thread.join();
        lap("wait for the variant stream (built beside it)");
    }
    if (rc) return rc;
    if (!concurrent) {
        rc_var = build_var(s);
        lap("variant stream");
    } else if (rc_var) {
        vrx_set_error("%s", err_var.c_str());
    }
    if (rc_var) return rc_var;
    VRX_HIP(hipStreamSynchronize(s));
    *balance_seconds = sec_cell + sec_var;
    return VRX_OK;
}

// Large problems: everything from the merged CSC arrays onwards happens on the device
// (vrx_build.h).  *built = false means "not applicable here" (small problem, counts the pair
// words cannot hold, a stream the padding guard rejects): the caller then runs the host builder
// on a problem with both orientations as new.
static int device_build(vrx_problem* p, const int64_t* colptr, const int32_t* rowidx, const int32_t* ad,
                        const int32_t* dp, const BuildPlan& plan, bool* built) {
    *built = false;
    const int64_t nnz = p->nnz, n_var = p->n_var, n_cell = p->n_cell;
    // Entry ids travel through the transposition as 32-bit sort values and the tiled builder keeps
    // segment bounds as 32-bit entry offsets: up to 2^32 - 1 entries (r6: was 2^31 - 1, and the slow
    // host builder took over without a word; 2.2e9 entries are built here in seconds,
    // profiles/r06_big_probe_*.txt).  Beyond that the host builder below is the path.
    if (nnz <= 0 || nnz >= (int64_t)UINT32_MAX - 4096) return VRX_OK;
    LapTimer lap{p->stream, "device_build:", 36};
    DeviceInput D;
    int32_t max_count = 0;
    int rc = upload_validate(p, colptr, rowidx, ad, dp, D, &max_count);
    if (rc) return rc;
    const StreamForms forms = settle_forms(plan.forms, max_count);
    const int var_form = forms.var, cell_form = forms.cell;
    const bool guard = plan.lds != 1;
    // (pair words hold 11-bit counts; a forced pair form leaves such data to the host builder)
    if ((var_form == 0 || cell_form == 0) && max_count >= 2048) return VRX_OK;
    lap("upload + validate");
    if ((rc = transpose_pack(p, D, max_count))) return rc;
    lap("transposition");
    VirtualRows V;
    if (var_form == 3 && (rc = virtual_rows(p, D, V))) return rc;
    lap("virtual rows");
    const TileRows cell_rows{colptr, nullptr, nullptr, {D.colptr.p, D.row.p, D.cval.p}, n_cell, n_var, nnz, false};
    const TileShape cell_shape{pick_rw_cell(n_var, n_cell, p->n_cu, cell_form), plan.slab_cell, cell_form, 1, guard,
                               p->want_balance};
    const TileRows var_rows = var_form == 3
        ? TileRows{V.h_ptr.data(), nullptr, nullptr, {V.ptr.p, V.idx.p, V.val.p}, 2 * n_var, (n_cell + 1) / 2, V.nnz, true}
        : TileRows{D.h_rptr.data(), nullptr, nullptr, {D.rptr.p, D.ridx.p, D.rval.p}, n_var, n_cell, nnz, false};
    const TileShape var_shape = var_form == 3
        ? TileShape{VRX_LDS_RW_CELL, VRX_LDS_SLAB_BYTES / 256, 1, 0, guard, p->want_balance}
        : TileShape{VRX_LDS_RW_VARIANT, VRX_LDS_SLAB_BYTES / 128, 0, 0, guard, p->want_balance};
    double balance_seconds = 0.0;
    if ((rc = build_both_streams(p, cell_rows, cell_shape, var_rows, var_shape, lap, &balance_seconds))) return rc;
    if (!p->by_cell.tiled.ready || !p->by_var.tiled.ready) {  // rejected by the padding guard
        p->by_cell = Orient();
        p->by_var = Orient();
        return VRX_OK;
    }
    p->device_built = true;
    p->balance_seconds = balance_seconds;
    *built = true;
    return VRX_OK;
}

extern "C" int vrx_problem_create(int device, int64_t n_var, int64_t n_cell, int64_t nnz,
                                  const int64_t* colptr, const int32_t* rowidx, const int32_t* ad,
                                  const int32_t* dp, vrx_problem** out) {
    // (VIREO_BALANCE=1 in the environment: balanced slabs for every problem built through this entry)
    return vrx_problem_create2(device, n_var, n_cell, nnz, colptr, rowidx, ad, dp,
                               env_int("VIREO_BALANCE", 0) != 0 ? VRX_PROBLEM_BALANCED : 0, out);
}

static int problem_create2(int device, int64_t n_var, int64_t n_cell, int64_t nnz, const int64_t* colptr,
                           const int32_t* rowidx, const int32_t* ad, const int32_t* dp, int32_t flags,
                           vrx_problem** out);

extern "C" int vrx_problem_create2(int device, int64_t n_var, int64_t n_cell, int64_t nnz,
                                   const int64_t* colptr, const int32_t* rowidx, const int32_t* ad,
                                   const int32_t* dp, int32_t flags, vrx_problem** out) {
    try {  // (the build allocates host arrays of the problem's size: out of memory is a status, not a throw
           //  across the C boundary)
        return problem_create2(device, n_var, n_cell, nnz, colptr, rowidx, ad, dp, flags, out);
    } catch (const std::bad_alloc&) {
        vrx_set_error("vrx_problem_create: out of host memory");
        return VRX_ERR_NOMEM;
    } catch (const std::exception& e) {
        vrx_set_error("vrx_problem_create: %s", e.what());
        return VRX_ERR_UNSUPPORTED;
    }
}

static int host_build(vrx_problem* p, const int64_t* colptr, const int32_t* rowidx, const int32_t* ad,
                      const int32_t* dp, const BuildPlan& plan);

static int problem_create2(int device, int64_t n_var, int64_t n_cell, int64_t nnz, const int64_t* colptr,
                           const int32_t* rowidx, const int32_t* ad, const int32_t* dp, int32_t flags,
                           vrx_problem** out) {
    VRX_REQUIRE(out, "vrx_problem_create: null output");
    *out = nullptr;
    VRX_REQUIRE(n_var > 0 && n_cell > 0 && nnz >= 0, "vrx_problem_create: bad shape");
    VRX_REQUIRE(n_var < INT32_MAX && n_cell < INT32_MAX, "vrx_problem_create: dimension >= 2^31");
    VRX_REQUIRE(colptr && (nnz == 0 || (rowidx && ad && dp)), "vrx_problem_create: null input");
    VRX_REQUIRE(colptr[0] == 0 && colptr[n_cell] == nnz, "vrx_problem_create: colptr/nnz mismatch");
    BuildPlan plan;
    int rc = pick_forms(nnz, ad, dp, &plan.forms);
    if (rc) return rc;
    if (int e = vrx_use_device("vrx_problem_create", device)) return e;
    std::unique_ptr<vrx_problem> p(new vrx_problem());
    p->device = device;
    p->n_var = n_var;
    p->n_cell = n_cell;
    p->nnz = nnz;
    p->want_balance = (flags & VRX_PROBLEM_BALANCED) != 0;
    hipDeviceProp_t prop;
    VRX_HIP(hipGetDeviceProperties(&prop, device));
    p->n_cu = prop.multiProcessorCount;
    VRX_HIP(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking));

    // Problems that will run on the LDS-resident passes anyway (both thresholds met) are built
    // on the device; VIREO_BUILD=host keeps the host builder (the specification the device
    // build is tested against), VIREO_BUILD=device takes the device path whenever VIREO_LDS
    // allows the streams.
    plan.lds = env_int("VIREO_LDS", -1);
    plan.min_nnz_cell = env_int("VIREO_LDS_MIN_NNZ", 4000000);
    plan.min_nnz_var = env_int("VIREO_LDS_MIN_NNZ_VAR", 32000000);
    plan.slab_cell = std::min(VRX_LDS_SLAB_BYTES / 256, std::max(16, env_int("VIREO_LDS_SLAB_CELL", VRX_LDS_SLAB_BYTES / 256)));
    const char* bm = getenv("VIREO_BUILD");
    const bool force_dev = bm && !strcmp(bm, "device"), force_host = bm && !strcmp(bm, "host");
    const bool big = nnz >= plan.min_nnz_cell && nnz >= plan.min_nnz_var;
    bool built = false;
    if (!force_host && plan.lds != 0 && (force_dev || big)) {
        if ((rc = device_build(p.get(), colptr, rowidx, ad, dp, plan, &built))) return rc;
    }
    if (!built && (rc = host_build(p.get(), colptr, rowidx, ad, dp, plan))) return rc;
    VRX_HIP(p->cell_ptr.upload(colptr, (size_t)n_cell + 1, p->stream));
    VRX_HIP(hipStreamSynchronize(p->stream));  // (the caller's colptr may go at return)
    *out = p.release();
    return VRX_OK;
}

// The host builder (the specification the device builder is tested against): validation, transposition and
// packing on host threads, gather tables of both orientations, and the tiled streams where VIREO_LDS and the
// problem's size ask for them.
static int host_build(vrx_problem* p, const int64_t* colptr, const int32_t* rowidx, const int32_t* ad,
                      const int32_t* dp, const BuildPlan& plan) {
    const int64_t nnz = p->nnz, n_var = p->n_var, n_cell = p->n_cell;
    // validate + interleave (ad, dp); count per-cell and per-variant entries.  Cells are cut
    // into one contiguous chunk per host thread; every thread keeps its own per-variant
    // histogram, which also gives it private write cursors for the transposition below
    // (a parallel counting sort: cells stay increasing inside each variant row).
    RawArray<int2> cval((size_t)nnz);
    std::vector<int64_t> rptr((size_t)n_var + 1, 0);
    p->n_vars.assign((size_t)n_cell, 0);
    const int nt = (int)std::max<int64_t>(1, std::min<int64_t>(host_threads(), n_cell));
    std::vector<std::vector<int64_t>> hist((size_t)nt, std::vector<int64_t>((size_t)n_var, 0));
    std::vector<int32_t> tmax((size_t)nt, 0);
    std::vector<int64_t> bad_col((size_t)nt, -1), bad_kind((size_t)nt, 0);
    parallel_chunks(n_cell, nt, [&](int64_t c0, int64_t c1, int tid) {
        auto& h = hist[(size_t)tid];
        int32_t mx = 0;
        for (int64_t c = c0; c < c1; ++c) {
            if (colptr[c + 1] < colptr[c]) {
                bad_col[(size_t)tid] = c, bad_kind[(size_t)tid] = 1;
                return;
            }
            int32_t prev = -1, nv = 0;
            for (int64_t e = colptr[c]; e < colptr[c + 1]; ++e) {
                const int32_t r = rowidx[e];
                if (r <= prev || r >= n_var) {
                    bad_col[(size_t)tid] = c, bad_kind[(size_t)tid] = 2;
                    return;
                }
                if (ad[e] < 0 || dp[e] < 0) {
                    bad_col[(size_t)tid] = c, bad_kind[(size_t)tid] = 3;
                    return;
                }
                prev = r;
                cval[(size_t)e] = make_int2(ad[e], dp[e]);
                mx = std::max(mx, std::max(ad[e], dp[e]));
                ++h[(size_t)r];
                nv += dp[e] > 0;
            }
            p->n_vars[(size_t)c] = nv;
        }
        tmax[(size_t)tid] = mx;
    });
    int32_t max_count = 0;
    for (int t = 0; t < nt; ++t) {
        max_count = std::max(max_count, tmax[(size_t)t]);
        if (bad_kind[(size_t)t]) return input_error((int)bad_kind[(size_t)t], bad_col[(size_t)t]);
    }
    // rptr = exclusive scan of the per-variant totals; hist[t][r] becomes thread t's first
    // write position inside variant row r
    for (int64_t r = 0; r < n_var; ++r) {
        int64_t at = rptr[(size_t)r];
        for (int t = 0; t < nt; ++t) {
            const int64_t n = hist[(size_t)t][(size_t)r];
            hist[(size_t)t][(size_t)r] = at;
            at += n;
        }
        rptr[(size_t)r + 1] = at;
    }
    RawArray<int32_t> ridx((size_t)nnz);
    RawArray<int2> rval((size_t)nnz);
    VRX_REQUIRE(cval.p && ridx.p && rval.p, "out of host memory");
    parallel_chunks(n_cell, nt, [&](int64_t c0, int64_t c1, int tid) {
        auto& cur = hist[(size_t)tid];
        for (int64_t c = c0; c < c1; ++c)
            for (int64_t e = colptr[c]; e < colptr[c + 1]; ++e) {
                const int64_t q = cur[(size_t)rowidx[e]]++;
                ridx[(size_t)q] = (int32_t)c;
                rval[(size_t)q] = cval[(size_t)e];
            }
    });
    const int tiles_c = pick_tiles(n_var, 256.0, "VIREO_TILES_CELL");   // W rows: 16 x 16 B
    const int tiles_v = pick_tiles(n_cell, 128.0, "VIREO_TILES_VAR");   // ID rows: 16 x 8 B
    int rc = build_orient(p->by_cell, n_cell, n_var, colptr, rowidx, cval.data(), rptr.data(),
                          tiles_c, pick_fmt(max_count, n_var), p->stream);
    if (rc) return rc;
    rc = build_orient(p->by_var, n_var, n_cell, rptr.data(), ridx.data(), rval.data(), colptr,
                      tiles_v, pick_fmt(max_count, n_cell), p->stream);
    if (rc) return rc;
    // LDS-resident passes (vrx_spmm_lds) pay off on large problems (two-dimensional tiling,
    // one 160 KiB workgroup per CU); VIREO_LDS=0/1 forces them off/on.  Measured crossovers
    // against the gather kernels (K = 8 and 16): the cell pass wins from ~4 M non-zeros; the
    // variant pass (whose per-range partials also cost the theta kernel a wider read) only
    // ties at 8-16 M and wins clearly at 100 M.
    const int lds = plan.lds;
    const StreamForms f = settle_forms(plan.forms, max_count);
    const int cell_form = f.cell, var_form = f.var;  // cell 1: AD/BD stream; variant 3: AD/BD virtual rows;
    const bool pairs_fit = max_count < 2048;         // else pairs (11-bit counts)
    if ((pairs_fit || cell_form == 1) && lds != 0) {
        // cell pass: slabs of 512 W rows (128 KiB at K = 16); variant pass: 1024 ID rows
        if (lds == 1 || nnz >= plan.min_nnz_cell) {
            const TileRows rows{colptr, rowidx, cval.data(), {}, n_cell, n_var, nnz, false};
            const TileShape shape{pick_rw_cell(n_var, n_cell, p->n_cu, cell_form), plan.slab_cell, cell_form, 1,
                                  lds != 1, false};
            if ((rc = build_tiled(p->by_cell, rows, shape, p->n_cu, p->stream))) return rc;
        }
        if (var_form == 3 && (lds == 1 || nnz >= plan.min_nnz_var)) {
            std::vector<int64_t> vptr2;
            std::vector<int32_t> vidx;
            std::vector<int2> vval;
            derive_virtual_rows(n_var, rptr.data(), ridx.data(), rval.data(), vptr2, vidx, vval);
            const TileRows rows{vptr2.data(), vidx.data(), vval.data(), {}, 2 * n_var, (n_cell + 1) / 2,
                                (int64_t)vidx.size(), true};
            const TileShape shape{VRX_LDS_RW_CELL, VRX_LDS_SLAB_BYTES / 256, 1, 0, lds != 1, false};
            if ((rc = build_tiled(p->by_var, rows, shape, p->n_cu, p->stream))) return rc;
        } else if (pairs_fit && (lds == 1 || nnz >= plan.min_nnz_var)) {
            const TileRows rows{rptr.data(), ridx.data(), rval.data(), {}, n_var, n_cell, nnz, false};
            const TileShape shape{VRX_LDS_RW_VARIANT, VRX_LDS_SLAB_BYTES / 128, 0, 0, lds != 1, false};
            if ((rc = build_tiled(p->by_var, rows, shape, p->n_cu, p->stream))) return rc;
        }
    }
    return VRX_OK;
}

extern "C" void vrx_problem_destroy(vrx_problem* p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    if (p->stream) (void)hipStreamDestroy(p->stream);
    delete p;
}

// The float32 terms are formed on the device in the reference's indexing order (row-major:
// the variant-major orientation's storage order), brought to the host and added there in
// NumPy's float32 pairwise order, so the constant equals the reference's bit for bit (up to a
// term whose float64 value sits within 1e-16 of a float32 rounding boundary: lgamma here,
// log(binom()) there).  Once per problem.
extern "C" int vrx_problem_binom_const(vrx_problem* p, double* sum_out) {
    VRX_REQUIRE(p && sum_out, "vrx_problem_binom_const: null argument");
    if (!p->binom_done) {
        VRX_HIP(hipSetDevice(p->device));
        const Orient& o = p->by_var;
        const int64_t n = o.nnz;
        float total = 0.f;
        if (n > 0) {
            DevBuf<float> terms, sums;
            DevBuf<int32_t> flag;
            VRX_HIP(terms.alloc((size_t)n));
            const unsigned nb = (unsigned)((n + VRX_BLOCK - 1) / VRX_BLOCK);
            if (o.fmt == VRX_FMT_P32)
                vrx_binom_terms<VRX_FMT_P32><<<nb, VRX_BLOCK, 0, p->stream>>>(n, o.ent.p, terms.p);
            else if (o.fmt == VRX_FMT_P64)
                vrx_binom_terms<VRX_FMT_P64><<<nb, VRX_BLOCK, 0, p->stream>>>(n, o.ent.p, terms.p);
            else
                vrx_binom_terms<VRX_FMT_WIDE><<<nb, VRX_BLOCK, 0, p->stream>>>(n, o.ent.p, terms.p);
            VRX_HIP(hipGetLastError());
            // NumPy sums 8192 elements at a time: the full buffers are summed on the device in
            // its order, their sums and the last partial buffer are added on the host.  A NaN
            // mark (an entry with dp == 0, which the reference's DP > 0 mask skips) shifts the
            // buffer boundaries: then all terms come back and are compacted first.
            const int64_t n_chunk = n / 8192, tail = n - n_chunk * 8192;
            std::vector<float> hs((size_t)n_chunk), ht((size_t)tail);
            int32_t has_nan = 0;
            VRX_HIP(flag.alloc(1));
            VRX_HIP(hipMemsetAsync(flag.p, 0, sizeof(int32_t), p->stream));
            if (n_chunk > 0) {
                VRX_HIP(sums.alloc((size_t)n_chunk));
                vrx_np_chunk_sums_f32<<<(unsigned)n_chunk, 64, 0, p->stream>>>(n_chunk, terms.p, sums.p, flag.p);
                VRX_HIP(hipGetLastError());
                VRX_HIP(hipMemcpyAsync(hs.data(), sums.p, (size_t)n_chunk * sizeof(float),
                                       hipMemcpyDeviceToHost, p->stream));
            }
            if (tail > 0)
                VRX_HIP(hipMemcpyAsync(ht.data(), terms.p + n_chunk * 8192, (size_t)tail * sizeof(float),
                                       hipMemcpyDeviceToHost, p->stream));
            VRX_HIP(hipMemcpyAsync(&has_nan, flag.p, sizeof(int32_t), hipMemcpyDeviceToHost, p->stream));
            VRX_HIP(hipStreamSynchronize(p->stream));
            for (float v : ht) has_nan |= v != v;
            if (!has_nan) {
                for (float v : hs) total += v;
                float t = 0.f;
                if (vrx_np_sum_f32(ht.data(), tail, &t)) return VRX_ERR_ARG;
                if (tail > 0) total += t;
            } else {
                std::vector<float> h((size_t)n);
                VRX_HIP(hipMemcpyAsync(h.data(), terms.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost,
                                       p->stream));
                VRX_HIP(hipStreamSynchronize(p->stream));
                int64_t m = 0;
                for (int64_t i = 0; i < n; ++i)
                    if (h[(size_t)i] == h[(size_t)i]) h[(size_t)m++] = h[(size_t)i];  // drop the marks
                if (vrx_np_sum_f32(h.data(), m, &total)) return VRX_ERR_ARG;
            }
        }
        p->binom_sum = (double)total;
        p->binom_done = true;
    }
    *sum_out = p->binom_sum;
    return VRX_OK;
}

// 64-bit FNV-1a of device arrays (downloaded), folded into *x: tests compare the streams of the host and the
// device builder with it
static constexpr uint64_t kFnvBasis = 1469598103934665603ull;
template <class T>
static int fnv_fold(const DevBuf<T>& b, hipStream_t s, uint64_t* x) {
    std::vector<unsigned char> h(b.n * sizeof(T));
    if (!h.empty()) {
        VRX_HIP(hipMemcpyAsync(h.data(), b.p, h.size(), hipMemcpyDeviceToHost, s));
        VRX_HIP(hipStreamSynchronize(s));
    }
    for (unsigned char c : h) *x = (*x ^ c) * 1099511628211ull;
    return VRX_OK;
}

extern "C" int vrx_problem_digest(vrx_problem* p, uint64_t* out12) {
    VRX_REQUIRE(p && out12, "vrx_problem_digest: null argument");
    VRX_HIP(hipSetDevice(p->device));
    int rc;
    for (int i = 0; i < 12; ++i) out12[i] = kFnvBasis;
    uint64_t* x = out12;
    for (Orient* o : {&p->by_var, &p->by_cell}) {
        if ((rc = fnv_fold(o->ent, p->stream, x++))) return rc;
        if ((rc = fnv_fold(o->tiled.ent, p->stream, x++))) return rc;
        if ((rc = fnv_fold(o->tiled.bnd, p->stream, x++))) return rc;
        if ((rc = fnv_fold(o->tiled.wave_start, p->stream, x++))) return rc;
        if ((rc = fnv_fold(o->tiled.rowmap, p->stream, x))) return rc;  // (+ the balanced slabs' permutation)
        if ((rc = fnv_fold(o->tiled.perm, p->stream, x++))) return rc;
        *x++ = (uint64_t)o->n_seg;
    }
    return VRX_OK;
}

extern "C" int vrx_problem_build_info(vrx_problem* p, double* info4) {
    VRX_REQUIRE(p && info4, "vrx_problem_build_info: null argument");
    info4[0] = p->by_var.tiled.balanced() ? 1.0 : 0.0;
    info4[1] = p->by_cell.tiled.balanced() ? 1.0 : 0.0;
    info4[2] = p->balance_seconds;
    info4[3] = p->device_built ? 1.0 : 0.0;
    return VRX_OK;
}

extern "C" int vrx_problem_entry_format(vrx_problem* p, int32_t* fmt2) {
    VRX_REQUIRE(p && fmt2, "vrx_problem_entry_format: null argument");
    fmt2[0] = p->by_var.fmt;
    fmt2[1] = p->by_cell.fmt;
    return VRX_OK;
}

extern "C" int vrx_problem_n_vars(vrx_problem* p, int32_t* out) {
    VRX_REQUIRE(p && out, "vrx_problem_n_vars: null argument");
    std::memcpy(out, p->n_vars.data(), p->n_vars.size() * sizeof(int32_t));
    return VRX_OK;
}

// ------------------------------------------------------------------------------------
// model
// ------------------------------------------------------------------------------------
static constexpr int kTraceInit = 1 << 12;  // ELBO slots per restart a model starts with (ensure_trace grows them)
static constexpr int kEventPairs = 1 << 13;

// One of the four state arrays (ID, GT, beta_mu, beta_sum), each holding R restarts: restart r's
// block is rows x cols at row stride R * cols and column offset r * cols -- ID (M, K), GT (N, K*T),
// beta (1, th_rows * th_cols).
struct StatePart {
    DevBuf<double>* buf = nullptr;  // (null: the model kind has no such array -- GT of BMM)
    int64_t rows = 0, cols = 0;
    int norm = 0;  // a raw draw is normalised over groups of `norm` columns; 0: beta, never
    size_t size(int R) const { return (size_t)(rows * R * cols); }
    size_t block() const { return (size_t)(rows * cols); }
};

// One column-block launch of an LDS-resident pass: the template arguments of the instance that ran
// (MODE: the kernel's, 1 for the variant pass over virtual rows), the block's columns and the operand's
// row stride, whether the balanced gather list was passed, and the slab geometry of the stream
struct LdsLaunch {
    int32_t mode, rw, padk, split, form, kb, ld, perm, slab_rows, n_slab;
};

struct vrx_model {
    vrx_problem* p = nullptr;
    vrx_model_cfg cfg{};
    int K = 0, T = 0, KP = 0;
    int R = 1, Kt = 0;  // restarts in the batch; R * K columns of the dense operands
    int64_t N = 0, M = 0, NK = 0, NKt = 0;
    VrxBatch batch() const { return VrxBatch{R, K, Kt}; }
    int64_t th_rows = 1, th_cols = 0;  // shape of beta_mu / beta_sum
    // variational state
    DevBuf<double> ID, GT, mu, sm;
    StatePart part[4];  // their layout: every state entry point walks this table
    // derived tables
    DevBuf<double> psi;  // [3][th_rows][T]   (Vireo)
    DevBuf<double> S;    // [N][K] double2  (sum ad*ID, sum dp*ID)
    DevBuf<double> W;    // [N][K] double2  (W1, W2)
    DevBuf<double> LID;  // [M][K]          logLik_ID
    DevBuf<double> PV, PC;  // split-row partial slots
    DevBuf<double> RV, RC;  // per-range partials of the LDS-resident passes
    // priors
    DevBuf<double> logq_id, logq_gt, prior1, prior2, tmp, tmp2;
    int id_mode = 0, gt_mode = 0;
    int64_t prior_rows = 1;
    // reductions
    int nb_theta = 0, nb_nk = 0, nb_cell = 0, nb_throws = 0, n_th_part = 1;
    int nb_gt = 0;               // blocks (= KL_GT partials) of the grid-stride vrx_gt_update
    int n_cell_part = 0;         // cell partials of the kernel that ran last (softmax or fused cell pass)
    bool theta_pending = false;  // stage-1 partials wait for the finalisation inside vrx_gt_update
    DevBuf<double> part_theta, part_gt, part_cell, part_th;
    // clone mode: vrx_bmm_theta WRITES the KL_theta partials, so the ELBO block that rides in it
    // (VrxElboRide) must read the previous iteration's from another buffer: two halves of part_th,
    // th_cur = the half written last (Vireo: always 0)
    size_t th_cap = 0;
    int th_cur = 0;
    DevBuf<double> d_elbo, d_parts;
    int64_t trace_cap = 0;  // ELBO slots per restart in d_elbo
    DevBuf<int32_t> ctl;  // device-side loop control (VRX_CTL_*)
    DevBuf<double> snap[3];  // vrx_model_snapshot: ID, GT, beta_mu | beta_sum
    bool snap_valid = false;
    // vrx_model_stage_raw: the NEXT restart's raw draws (ID, GT), uploaded on a copy stream while
    // this one fits (two buffers; staged[b] / consumed[b] order the copy against its consumer)
    DevBuf<double> stage[2][2];
    hipStream_t copy_stream = nullptr;
    hipEvent_t staged[2] = {nullptr, nullptr}, consumed[2] = {nullptr, nullptr};
    hipEvent_t polled[2] = {nullptr, nullptr};  // vrx_model_fit's pipelined polls
    double* h_pin = nullptr;  // pinned staging for scalar read-backs
    int wform = 0;            // layout of W: 0 (W1, W2) pairs, 1 planar (Wa | Wb) rows (FORM 1)
    bool w_valid = false;     // W matches (GT, psi) on the device
    bool s_pending = false;   // S still sits in RV as per-range partials (take_S)
    bool l_pending = false;   // logLik_ID still sits in RC as per-range partials (take_LID)
    // launch-bound problems: the ELBO of the iteration enqueued last has not been finalised yet --
    // it rides as an extra block in the next iteration's vrx_theta_partial (VrxElboRide)
    bool elbo_deferred = false;
    VrxStopRule elbo_rule{};
    // profiling
    bool prof = false;
    std::vector<hipEvent_t> ev;
    std::vector<int> ev_kind;
    int ev_used = 0;
    double prof_ms[VRX_KERN_COUNT] = {0, 0, 0};
    int64_t prof_n[VRX_KERN_COUNT] = {0, 0, 0};
    hipEvent_t t0 = nullptr, t1 = nullptr;
    // the launches of the last LDS-resident pass of each orientation (0 variant, 1 cell): vrx_model_lds_launches
    std::vector<LdsLaunch> lds_log[2];
    // what the dense kernels' last launches of each kind did: vrx_model_dense_launches
    int32_t dense_log[VRX_DENSE_FIELDS] = {0, 0, VRX_DENSE_THETA_NONE, 0, 0, 0, 0, -1, 0, 0, 0, 0, 0, 0, VRX_DENSE_ELBO_NONE};

    ~vrx_model() {
        if (h_pin) (void)hipHostFree(h_pin);
        for (auto e : ev) (void)hipEventDestroy(e);
        if (t0) (void)hipEventDestroy(t0);
        if (t1) (void)hipEventDestroy(t1);
        for (int b = 0; b < 2; ++b) {
            if (staged[b]) (void)hipEventDestroy(staged[b]);
            if (consumed[b]) (void)hipEventDestroy(consumed[b]);
            if (polled[b]) (void)hipEventDestroy(polled[b]);
        }
        if (copy_stream) (void)hipStreamDestroy(copy_stream);
    }
};

// the device-side ELBO trace holds n entries per restart (grown between fits: its content is
// read back before a fit returns and never carried over)
static int ensure_trace(vrx_model* m, int64_t n) {
    if (n <= m->trace_cap) return VRX_OK;
    VRX_REQUIRE(n < ((int64_t)1 << 31), "max_iter too large");
    VRX_HIP(hipStreamSynchronize(m->p->stream));
    int64_t cap = std::max<int64_t>(m->trace_cap, 1);
    while (cap < n) cap *= 2;
    // into a temporary: a failed allocation (huge max_iter) must leave the old trace and its
    // capacity in place -- the model stays usable and the call returns an error code
    DevBuf<double> grown;
    const hipError_t e = grown.alloc((size_t)m->R * (size_t)cap);
    if (e != hipSuccess) {
        (void)hipGetLastError();  // (the runtime keeps a failed call's code for the next hipGetLastError: clear it)
        vrx_set_error("ELBO trace of %lld iterations x %d restarts: %s", (long long)cap, m->R, hipGetErrorString(e));
        return VRX_ERR_HIP;
    }
    m->d_elbo.swap(grown);
    m->trace_cap = cap;
    return VRX_OK;
}

static int pick_kp(int K, int cap = 64) {
    int kp = 1;
    while (kp < K && kp < cap) kp <<= 1;
    return kp;
}

struct ProfScope {  // brackets launches of one kernel class with events when profiling
    vrx_model* m;
    int slot = -1;
    ProfScope(vrx_model* m_, int kind) : m(m_) {
        if (m->prof && m->ev_used + 2 <= (int)m->ev.size()) {
            slot = m->ev_used;
            m->ev_used += 2;
            m->ev_kind[slot / 2] = kind;
            (void)hipEventRecord(m->ev[slot], m->p->stream);
        }
    }
    ~ProfScope() {
        if (slot >= 0) (void)hipEventRecord(m->ev[slot + 1], m->p->stream);
    }
};

static int prof_drain(vrx_model* m) {
    if (m->ev_used == 0) return VRX_OK;
    VRX_HIP(hipStreamSynchronize(m->p->stream));
    for (int s = 0; s < m->ev_used; s += 2) {
        float ms = 0.f;
        VRX_HIP(hipEventElapsedTime(&ms, m->ev[s], m->ev[s + 1]));
        m->prof_ms[m->ev_kind[s / 2]] += ms;
        m->prof_n[m->ev_kind[s / 2]] += 1;
    }
    m->ev_used = 0;
    return VRX_OK;
}

template <int MODE>
static bool lds_eligible(const vrx_problem& p, int K);

extern "C" int vrx_model_create(vrx_problem* p, const vrx_model_cfg* cfg, vrx_model** out) {
    VRX_REQUIRE(p && cfg && out, "vrx_model_create: null argument");
    *out = nullptr;
    VRX_REQUIRE(cfg->kind == VRX_KIND_VIREO || cfg->kind == VRX_KIND_BMM,
                "vrx_model_create: unknown model kind %d", cfg->kind);
    VRX_REQUIRE(cfg->n_donor >= 1, "vrx_model_create: n_donor must be >= 1");
    if (cfg->kind == VRX_KIND_VIREO && (cfg->n_gt < 1 || cfg->n_gt > VRX_MAXT)) {
        vrx_set_error("vrx_model_create: n_GT=%d unsupported (1..%d)", cfg->n_gt, VRX_MAXT);
        return VRX_ERR_UNSUPPORTED;
    }
    VRX_HIP(hipSetDevice(p->device));
    std::unique_ptr<vrx_model> m(new vrx_model());
    m->p = p;
    m->cfg = *cfg;
    m->K = cfg->n_donor;
    m->T = cfg->kind == VRX_KIND_VIREO ? cfg->n_gt : 1;
    m->KP = pick_kp(m->K);
    m->N = p->n_var;
    m->M = p->n_cell;
    m->NK = m->N * m->K;
    m->R = std::max(1, (int)cfg->n_batch);
    VRX_REQUIRE(m->R <= 16, "vrx_model_create: at most 16 restarts per batch");
    m->Kt = m->R * m->K;
    m->NKt = m->NK * m->R;
    VRX_REQUIRE(m->NK < INT32_MAX * (int64_t)VRX_BLOCK, "vrx_model_create: n_var*n_donor too large");
    if (cfg->kind == VRX_KIND_VIREO) {
        m->th_rows = cfg->ase_mode ? m->N : 1;
        m->th_cols = m->T;
    } else {
        m->th_rows = m->N;
        m->th_cols = m->K;
    }
    m->part[0] = {&m->ID, m->M, m->K, m->K};
    if (cfg->kind == VRX_KIND_VIREO) m->part[1] = {&m->GT, m->N, (int64_t)m->K * m->T, m->T};
    m->part[2] = {&m->mu, 1, m->th_rows * m->th_cols, 0};
    m->part[3] = {&m->sm, 1, m->th_rows * m->th_cols, 0};
    hipStream_t s = p->stream;
    const size_t th = (size_t)(m->R * m->th_rows * m->th_cols);
    VRX_HIP(m->ID.alloc((size_t)((m->M + 1) * m->Kt)));  // (+ a row: an odd M's last DOUBLE row, TiledStream::virt)
    VRX_HIP(hipMemsetAsync(m->ID.p + (size_t)(m->M * m->Kt), 0, (size_t)m->Kt * sizeof(double), s));
    VRX_HIP(m->LID.alloc((size_t)(m->M * m->Kt)));
    VRX_HIP(m->mu.alloc(th));  // (th already counts the R restarts)
    VRX_HIP(m->sm.alloc(th));
    VRX_HIP(m->prior1.alloc(th));
    VRX_HIP(m->prior2.alloc(th));
    VRX_HIP(m->S.alloc((size_t)m->NKt * 2));
    VRX_HIP(m->W.alloc((size_t)m->NKt * 2));
    VRX_HIP(m->PV.alloc((size_t)(p->by_var.n_slots * m->Kt * 2)));
    VRX_HIP(m->PC.alloc((size_t)(p->by_cell.n_slots * m->Kt)));
    {
        const TiledStream &tv = p->by_var.tiled, &tc = p->by_cell.tiled;
        if (lds_eligible<0>(*p, m->Kt) && tv.virt)  // planar sums of the virtual rows
            VRX_HIP(m->RV.alloc((size_t)(tv.n_range * tv.n_vrows * m->Kt)));
        else if (lds_eligible<0>(*p, m->Kt) && (tv.n_range > 1 || tv.split))
            VRX_HIP(m->RV.alloc((size_t)(tv.n_range * tv.n_vrows * m->Kt * 2)));
        if (lds_eligible<1>(*p, m->Kt) && (tc.n_range > 1 || tc.split))
            VRX_HIP(m->RC.alloc((size_t)(tc.n_range * tc.n_vrows * m->Kt)));
    }
    m->wform = lds_eligible<1>(*p, m->Kt) && p->by_cell.tiled.form == 1 ? 1 : 0;
    // rows without entries are never written by the passes: zero once
    VRX_HIP(hipMemsetAsync(m->S.p, 0, (size_t)m->NKt * 2 * sizeof(double), s));
    VRX_HIP(hipMemsetAsync(m->LID.p, 0, (size_t)(m->M * m->Kt) * sizeof(double), s));
    VRX_HIP(hipMemsetAsync(m->ID.p, 0, (size_t)(m->M * m->Kt) * sizeof(double), s));
    m->nb_nk = (int)((m->NK + VRX_BLOCK - 1) / VRX_BLOCK);
    m->nb_cell = (int)((m->M * m->KP + VRX_BLOCK - 1) / VRX_BLOCK);
    {   // vrx_cell_softmax strides over the cells: at most VIREO_SOFTMAX_BLOCKS_PER_CU blocks per CU
        // (0 = one block per 256 lanes, as before; c5: dense kernels 40.9 -> 38.0 us at 4, 39.0 at 8,
        //  39.2 at 16; c3: 0.108 -> 0.1055 ms; profiles/r05_ab_softmax_grid.txt)
        const int cap = env_int("VIREO_SOFTMAX_BLOCKS_PER_CU", 4);
        if (cap > 0) m->nb_cell = std::min(m->nb_cell, p->n_cu * cap);
    }
    m->nb_throws = (int)((m->N + VRX_BLOCK - 1) / VRX_BLOCK);
    m->nb_theta = std::min(m->nb_nk, p->n_cu * 4);
    m->nb_gt = std::min(m->nb_nk, p->n_cu * 8);
    m->n_cell_part = m->nb_cell;
    VRX_HIP(m->part_cell.alloc((size_t)m->R * std::max<int64_t>(m->nb_cell, p->by_cell.n_seg / VRX_WAVES + 1) * 2));
    VRX_HIP(m->part_gt.alloc((size_t)m->R * m->nb_nk));
    VRX_HIP(hipMemsetAsync(m->part_gt.p, 0, (size_t)m->R * m->nb_nk * sizeof(double), s));
    if (cfg->kind == VRX_KIND_VIREO) {
        VRX_HIP(m->GT.alloc((size_t)m->NKt * m->T));
        VRX_HIP(m->psi.alloc(3 * th));  // [R][3][rows][T]; th counts the R restarts
        VRX_HIP(m->part_theta.alloc((size_t)m->R * m->nb_theta * 2 * VRX_MAXT));
        m->n_th_part = cfg->ase_mode ? m->nb_throws : 1;
    } else {
        m->n_th_part = m->nb_nk;
    }
    // (clone mode with the range sum fused into vrx_bmm_theta runs 16 lanes per element: 16x the blocks)
    const size_t th_cap = (size_t)m->R * (cfg->kind == VRX_KIND_VIREO ? m->n_th_part : (m->NK * 16 + VRX_BLOCK - 1) / VRX_BLOCK + 1);
    m->th_cap = th_cap;
    VRX_HIP(m->part_th.alloc(th_cap * (cfg->kind == VRX_KIND_BMM ? 2 : 1)));
    VRX_HIP(hipMemsetAsync(m->part_th.p, 0, th_cap * (cfg->kind == VRX_KIND_BMM ? 2 : 1) * sizeof(double), s));
    m->trace_cap = kTraceInit;
    VRX_HIP(m->d_elbo.alloc((size_t)m->R * m->trace_cap));
    VRX_HIP(m->ctl.alloc((size_t)m->R * VRX_CTL_WORDS));
    VRX_HIP(hipMemsetAsync(m->ctl.p, 0, (size_t)m->R * VRX_CTL_WORDS * sizeof(int32_t), s));
    VRX_HIP(m->d_parts.alloc((size_t)m->R * 4));
    VRX_HIP(hipHostMalloc(reinterpret_cast<void**>(&m->h_pin), 64 * sizeof(double), hipHostMallocDefault));
    VRX_HIP(hipEventCreate(&m->t0));
    VRX_HIP(hipEventCreate(&m->t1));
    VRX_HIP(hipStreamSynchronize(s));
    *out = m.release();
    return VRX_OK;
}

extern "C" void vrx_model_destroy(vrx_model* m) {
    if (!m) return;
    (void)hipSetDevice(m->p->device);
    (void)hipStreamSynchronize(m->p->stream);
    delete m;
}

static int h2d(vrx_model* m, DevBuf<double>& dst, const double* src, size_t n) {
    if (!src) return VRX_OK;
    VRX_REQUIRE(dst.n >= n, "internal: upload larger than buffer");
    VRX_HIP(hipMemcpyAsync(dst.p, src, n * sizeof(double), hipMemcpyHostToDevice, m->p->stream));
    return VRX_OK;
}

static int d2h(vrx_model* m, double* dst, const DevBuf<double>& src, size_t n) {
    if (!dst) return VRX_OK;
    VRX_HIP(hipMemcpyAsync(dst, src.p, n * sizeof(double), hipMemcpyDeviceToHost, m->p->stream));
    return VRX_OK;
}

// raw draws -> rows that sum to one, in place: n values in rows of `cols`
static int normalize_raw(hipStream_t s, double* x, size_t n, int cols) {
    const int64_t rows = (int64_t)(n / (size_t)cols);
    vrx_normalize_rows<<<(unsigned)((rows + VRX_BLOCK - 1) / VRX_BLOCK), VRX_BLOCK, 0, s>>>(rows, cols, x);
    VRX_HIP(hipGetLastError());
    return VRX_OK;
}

// (vrx_normalize_rows holds its row in registers)
static int raw_supported(const vrx_model* m, const char* who) {
    if (m->K <= 128 && m->T <= 128) return VRX_OK;
    vrx_set_error("%s: more than 128 columns (normalise on the host)", who);
    return VRX_ERR_UNSUPPORTED;
}

// whole state arrays (all R restarts) from the host; null sources are left as they are
static int upload_state(vrx_model* m, const double* const src[4], bool raw) {
    hipStream_t s = m->p->stream;
    int rc;
    for (int i = 0; i < 4; ++i) {
        const StatePart& P = m->part[i];
        if (!P.buf || !src[i]) continue;
        if ((rc = h2d(m, *P.buf, src[i], P.size(m->R)))) return rc;
        if (raw && P.norm)
            if ((rc = normalize_raw(s, P.buf->p, P.size(m->R), P.norm))) return rc;
    }
    VRX_HIP(hipStreamSynchronize(s));
    m->w_valid = false;
    return VRX_OK;
}

extern "C" int vrx_model_set_state(vrx_model* m, const double* ID_prob, const double* GT_prob,
                                   const double* beta_mu, const double* beta_sum) {
    VRX_REQUIRE(m, "vrx_model_set_state: null model");
    VRX_HIP(hipSetDevice(m->p->device));
    const double* src[4] = {ID_prob, GT_prob, beta_mu, beta_sum};
    return upload_state(m, src, false);
}

extern "C" int vrx_model_set_state_raw(vrx_model* m, const double* ID_raw, const double* GT_raw,
                                       const double* beta_mu, const double* beta_sum) {
    VRX_REQUIRE(m, "vrx_model_set_state_raw: null model");
    int rc = raw_supported(m, "vrx_model_set_state_raw");
    if (rc) return rc;
    VRX_HIP(hipSetDevice(m->p->device));
    const double* src[4] = {ID_raw, GT_raw, beta_mu, beta_sum};
    return upload_state(m, src, true);  // ([M][R][K] and [N][R][K][T]: one row per restart)
}

// ---- staged uploads (vireo_wrap.py:64-87: the restarts run one after the other) -------------
// The raw constructor draws of restart i + 1 (45 MB at c3) travel to the device WHILE restart i
// fits: vrx_model_stage_reserve (once, from the thread that owns the model) makes two staging
// buffers, a copy stream and the events; vrx_model_stage_raw may then be called from a SECOND host
// thread concurrently with vrx_model_fit on the same model -- it touches nothing but its staging
// buffer and the copy stream; vrx_model_set_state_staged (owner thread) normalises the buffer into
// the model's state on the compute stream.  Results are those of vrx_model_set_state_raw, bitwise.
extern "C" int vrx_model_stage_reserve(vrx_model* m) {
    VRX_REQUIRE(m, "vrx_model_stage_reserve: null model");
    VRX_REQUIRE(m->R == 1 && m->cfg.kind == VRX_KIND_VIREO, "vrx_model_stage_reserve: single Vireo models only");
    if (m->copy_stream) return VRX_OK;
    VRX_HIP(hipSetDevice(m->p->device));
    for (int b = 0; b < 2; ++b) {
        for (int i = 0; i < 2; ++i) VRX_HIP(m->stage[b][i].alloc(m->part[i].block()));
        VRX_HIP(hipEventCreateWithFlags(&m->staged[b], hipEventDisableTiming));
        VRX_HIP(hipEventCreateWithFlags(&m->consumed[b], hipEventDisableTiming));
    }
    VRX_HIP(hipStreamCreateWithFlags(&m->copy_stream, hipStreamNonBlocking));
    return VRX_OK;
}

extern "C" int vrx_model_stage_raw(vrx_model* m, int32_t buf, const double* ID_raw, const double* GT_raw) {
    VRX_REQUIRE(m && ID_raw && GT_raw, "vrx_model_stage_raw: null argument");
    VRX_REQUIRE(buf == 0 || buf == 1, "vrx_model_stage_raw: buffer %d", buf);
    VRX_REQUIRE(m->copy_stream, "vrx_model_stage_raw: call vrx_model_stage_reserve first");
    VRX_HIP(hipSetDevice(m->p->device));
    hipStream_t c = m->copy_stream;
    // (the buffer's previous content has been normalised into the state: consumed[buf] was
    //  recorded behind that; an event never recorded counts as complete)
    VRX_HIP(hipStreamWaitEvent(c, m->consumed[buf], 0));
    const double* src[2] = {ID_raw, GT_raw};
    for (int i = 0; i < 2; ++i)
        VRX_HIP(hipMemcpyAsync(m->stage[buf][i].p, src[i], m->stage[buf][i].n * sizeof(double),
                               hipMemcpyHostToDevice, c));
    VRX_HIP(hipEventRecord(m->staged[buf], c));
    VRX_HIP(hipStreamSynchronize(c));  // (the host arrays may be reused by the caller)
    return VRX_OK;
}

extern "C" int vrx_model_set_state_staged(vrx_model* m, int32_t buf, const double* beta_mu,
                                          const double* beta_sum) {
    VRX_REQUIRE(m, "vrx_model_set_state_staged: null model");
    VRX_REQUIRE(buf == 0 || buf == 1, "vrx_model_set_state_staged: buffer %d", buf);
    VRX_REQUIRE(m->copy_stream, "vrx_model_set_state_staged: nothing was staged");
    int rc = raw_supported(m, "vrx_model_set_state_staged");
    if (rc) return rc;
    VRX_HIP(hipSetDevice(m->p->device));
    hipStream_t s = m->p->stream;
    VRX_HIP(hipStreamWaitEvent(s, m->staged[buf], 0));
    for (int i = 0; i < 2; ++i)
        VRX_HIP(hipMemcpyAsync(m->part[i].buf->p, m->stage[buf][i].p, m->stage[buf][i].n * sizeof(double),
                               hipMemcpyDeviceToDevice, s));
    VRX_HIP(hipEventRecord(m->consumed[buf], s));
    for (int i = 0; i < 2; ++i)
        if ((rc = normalize_raw(s, m->part[i].buf->p, m->stage[buf][i].n, m->part[i].norm))) return rc;
    const double* beta[4] = {nullptr, nullptr, beta_mu, beta_sum};
    return upload_state(m, beta, false);
}

// device-side copy of the variational state: the best restart so far is kept in HBM, no
// round trip through the host (vireo_wrap keeps `model_all[argmax]`, vireo_wrap.py:90-91)
extern "C" int vrx_model_snapshot(vrx_model* m, int32_t restore) {
    VRX_REQUIRE(m, "vrx_model_snapshot: null model");
    VRX_HIP(hipSetDevice(m->p->device));
    hipStream_t s = m->p->stream;
    if (restore) {
        VRX_REQUIRE(m->snap_valid, "vrx_model_snapshot: nothing saved");
    } else if (!m->snap[0].p) {
        for (int i = 0; i < 3; ++i)
            if (m->part[i].buf) VRX_HIP(m->snap[i].alloc(m->part[i].size(m->R) * (i == 2 ? 2 : 1)));
    }
    for (int i = 0; i < 4; ++i) {
        const StatePart& P = m->part[i];
        if (!P.buf) continue;
        // (the two beta halves share a buffer: the runtime's copy kernels depend on the alignment)
        double *live = P.buf->p, *saved = i < 3 ? m->snap[i].p : m->snap[2].p + P.size(m->R);
        VRX_HIP(hipMemcpyAsync(restore ? live : saved, restore ? saved : live, P.size(m->R) * sizeof(double),
                               hipMemcpyDeviceToDevice, s));
    }
    VRX_HIP(hipStreamSynchronize(s));
    if (restore)
        m->w_valid = false;
    else
        m->snap_valid = true;
    return VRX_OK;
}

// ---- restart batches -------------------------------------------------------------------
// rows x cols block between two row-major arrays with their own row strides and column offsets
__global__ __launch_bounds__(VRX_BLOCK) void vrx_copy_block(int64_t rows, int cols,
                                                            const double* __restrict__ src,
                                                            int64_t src_ld, int64_t src_off,
                                                            double* __restrict__ dst, int64_t dst_ld,
                                                            int64_t dst_off) {
    const int64_t i = (int64_t)blockIdx.x * VRX_BLOCK + threadIdx.x;
    if (i >= rows * cols) return;
    const int64_t r = i / cols, c = i - r * cols;
    dst[r * dst_ld + dst_off + c] = src[r * src_ld + src_off + c];
}

static int copy_block(hipStream_t s, int64_t rows, int64_t cols, const double* src, int64_t src_ld,
                      int64_t src_off, double* dst, int64_t dst_ld, int64_t dst_off) {
    const int64_t n = rows * cols;
    if (n == 0) return VRX_OK;
    vrx_copy_block<<<(unsigned)((n + VRX_BLOCK - 1) / VRX_BLOCK), VRX_BLOCK, 0, s>>>(
        rows, (int)cols, src, src_ld, src_off, dst, dst_ld, dst_off);
    VRX_HIP(hipGetLastError());
    return VRX_OK;
}

// Slot r of a batch model <- one restart's state, given exactly as vrx_model_set_state[_raw]
// takes it for a single model (ID [M][K], GT [N][K][T], beta [rows][cols]).  raw: the draws are
// row-normalised on the device first, in NumPy's order (vireo_model.py:99,104).
extern "C" int vrx_model_set_restart(vrx_model* m, int32_t r, const double* ID, const double* GT,
                                     const double* beta_mu, const double* beta_sum, int32_t raw) {
    VRX_REQUIRE(m, "vrx_model_set_restart: null model");
    VRX_REQUIRE(r >= 0 && r < m->R, "vrx_model_set_restart: slot %d outside the batch of %d", r, m->R);
    int rc;
    if (raw && (rc = raw_supported(m, "vrx_model_set_restart"))) return rc;
    VRX_HIP(hipSetDevice(m->p->device));
    hipStream_t s = m->p->stream;
    const double* src[4] = {ID, GT, beta_mu, beta_sum};
    DevBuf<double>* tmp[2] = {&m->tmp, &m->tmp2};  // (ID, GT: through the device, into the strided slot)
    for (int i = 0; i < 4; ++i) {
        const StatePart& P = m->part[i];
        if (!P.buf || !src[i]) continue;
        const size_t n = P.block();
        if (!P.norm) {  // beta: one row per restart, the slot is contiguous
            VRX_HIP(hipMemcpyAsync(P.buf->p + r * P.cols, src[i], n * sizeof(double), hipMemcpyHostToDevice, s));
            continue;
        }
        DevBuf<double>& t = *tmp[i];
        if (t.n != n) VRX_HIP(t.alloc(n));
        VRX_HIP(hipMemcpyAsync(t.p, src[i], n * sizeof(double), hipMemcpyHostToDevice, s));
        if (raw && (rc = normalize_raw(s, t.p, n, P.norm))) return rc;
        if ((rc = copy_block(s, P.rows, P.cols, t.p, P.cols, 0, P.buf->p, m->R * P.cols, r * P.cols))) return rc;
    }
    VRX_HIP(hipStreamSynchronize(s));  // (the host arrays may be reused by the caller)
    m->w_valid = false;
    return VRX_OK;
}

// dst (a single model of the same problem and shape) <- the state of slot r of `src`, on the
// device: the winner of a batch moves on without a host round trip (vireo_wrap.py:90-91)
extern "C" int vrx_model_copy_restart(vrx_model* dst, vrx_model* src, int32_t r) {
    VRX_REQUIRE(dst && src, "vrx_model_copy_restart: null model");
    VRX_REQUIRE(r >= 0 && r < src->R, "vrx_model_copy_restart: slot %d outside the batch of %d", r, src->R);
    VRX_REQUIRE(dst->R == 1 && dst->p == src->p && dst->K == src->K && dst->T == src->T &&
                    dst->cfg.kind == src->cfg.kind && dst->th_rows == src->th_rows,
                "vrx_model_copy_restart: models differ in problem or shape");
    VRX_HIP(hipSetDevice(src->p->device));
    hipStream_t s = src->p->stream;
    int rc;
    for (int i = 0; i < 4; ++i) {
        const StatePart& P = src->part[i];
        if (!P.buf) continue;
        double* to = dst->part[i].buf->p;
        if (!P.norm)  // beta: one row per restart, the slot is contiguous
            VRX_HIP(hipMemcpyAsync(to, P.buf->p + r * P.cols, P.block() * sizeof(double), hipMemcpyDeviceToDevice, s));
        else if ((rc = copy_block(s, P.rows, P.cols, P.buf->p, src->R * P.cols, r * P.cols, to, P.cols, 0)))
            return rc;
    }
    VRX_HIP(hipStreamSynchronize(s));
    dst->w_valid = false;
    return VRX_OK;
}

extern "C" int vrx_model_get_state(vrx_model* m, double* ID_prob, double* GT_prob, double* beta_mu,
                                   double* beta_sum) {
    VRX_REQUIRE(m, "vrx_model_get_state: null model");
    VRX_HIP(hipSetDevice(m->p->device));
    double* dst[4] = {ID_prob, GT_prob, beta_mu, beta_sum};
    int rc;
    for (int i = 0; i < 4; ++i)
        if (m->part[i].buf && (rc = d2h(m, dst[i], *m->part[i].buf, m->part[i].size(m->R)))) return rc;
    VRX_HIP(hipStreamSynchronize(m->p->stream));
    return VRX_OK;
}

// (internal: vrx_common.h) the state arrays vrx_comm_bcast_model sends / receives in place
int vrx_model_state_buffers(vrx_model* m, bool will_write, VrxModelBuffers* out) {
    VRX_REQUIRE(m && out, "vrx_model_state_buffers: null argument");
    VRX_HIP(hipSetDevice(m->p->device));
    VRX_HIP(hipStreamSynchronize(m->p->stream));
    for (int i = 0; i < 4; ++i) {
        const StatePart& P = m->part[i];
        out->p[i] = P.buf ? P.buf->p : nullptr;
        out->n[i] = P.buf ? P.size(m->R) : 0;
    }
    out->device = m->p->device;
    if (will_write) m->w_valid = false;
    return VRX_OK;
}

// logLik_ID as the call that defined it last left it: VRX_STEP_ID / VRX_STEP_LOGLIK, vrx_model_set_loglik,
// or the last iteration of a fit / vrx_model_run_iters.  On tiled cell streams with several ranges or split
// rows a fit's cell passes leave logLik_ID as partials in RC (take_LID); vrx_cell_softmax sums them and
// STORES the summed row into LID, so LID is final behind every iteration on every path
// (tests/test_gpu_model_sequences.py holds it against the oracle and against set_loglik, bit for bit).
extern "C" int vrx_model_get_loglik(vrx_model* m, double* out) {
    VRX_REQUIRE(m && out, "vrx_model_get_loglik: null argument");
    VRX_HIP(hipSetDevice(m->p->device));
    int rc = d2h(m, out, m->LID, (size_t)(m->M * m->Kt));
    if (rc) return rc;
    VRX_HIP(hipStreamSynchronize(m->p->stream));
    return VRX_OK;
}

extern "C" int vrx_model_set_loglik(vrx_model* m, const double* in) {
    VRX_REQUIRE(m && in, "vrx_model_set_loglik: null argument");
    VRX_HIP(hipSetDevice(m->p->device));
    int rc = h2d(m, m->LID, in, (size_t)(m->M * m->Kt));
    if (rc) return rc;
    VRX_HIP(hipStreamSynchronize(m->p->stream));
    return VRX_OK;
}

extern "C" int vrx_model_get_elbo_parts(vrx_model* m, double* parts4) {
    VRX_REQUIRE(m && parts4, "vrx_model_get_elbo_parts: null argument");
    VRX_HIP(hipSetDevice(m->p->device));
    VRX_HIP(hipMemcpyAsync(parts4, m->d_parts.p, (size_t)m->R * 4 * sizeof(double), hipMemcpyDeviceToHost,
                           m->p->stream));
    VRX_HIP(hipStreamSynchronize(m->p->stream));
    return VRX_OK;
}

// upload a probability table and turn it into row-normalised logs on the device
static int upload_log_rows(vrx_model* m, DevBuf<double>& dst, const double* src, int64_t rows,
                           int cols) {
    const size_t n = (size_t)(rows * cols);
    VRX_HIP(dst.alloc(n));
    VRX_HIP(m->tmp.alloc(n));
    VRX_HIP(hipMemcpyAsync(m->tmp.p, src, n * sizeof(double), hipMemcpyHostToDevice, m->p->stream));
    const int nb = (int)((rows + VRX_BLOCK - 1) / VRX_BLOCK);
    vrx_log_rows<<<nb, VRX_BLOCK, 0, m->p->stream>>>(rows, cols, m->tmp.p, dst.p);
    VRX_HIP(hipGetLastError());
    VRX_HIP(hipStreamSynchronize(m->p->stream));
    m->tmp.release();
    return VRX_OK;
}

// a prior of 0, 1 or one row per cell / variant: mode 0 (none), 1 (one row for all) or 2 (per row);
// each row holds `tables` probability tables of `cols`, kept as row-normalised logs
static int set_log_prior(vrx_model* m, DevBuf<double>& logq, int& mode, const double* src, int64_t rows,
                         int64_t tables, int cols) {
    if (rows == 0) {
        mode = 0;
        logq.release();
        return VRX_OK;
    }
    int rc = upload_log_rows(m, logq, src, rows * tables, cols);
    if (rc) return rc;
    mode = rows == 1 ? 1 : 2;
    return VRX_OK;
}

extern "C" int vrx_model_set_prior(vrx_model* m, const double* ID_prior, int64_t id_rows,
                                   const double* GT_prior, int64_t gt_rows, const double* s1_prior,
                                   const double* s2_prior, int64_t theta_prior_rows) {
    VRX_REQUIRE(m, "vrx_model_set_prior: null model");
    VRX_HIP(hipSetDevice(m->p->device));
    VRX_REQUIRE(id_rows == 0 || id_rows == 1 || id_rows == m->M,
                "vrx_model_set_prior: ID_prior must have 0, 1 or n_cell rows (got %lld)",
                (long long)id_rows);
    VRX_REQUIRE(id_rows == 0 || ID_prior, "vrx_model_set_prior: null ID_prior");
    int rc;
    if ((rc = set_log_prior(m, m->logq_id, m->id_mode, ID_prior, id_rows, 1, m->K))) return rc;
    if (m->cfg.kind == VRX_KIND_VIREO) {
        VRX_REQUIRE(gt_rows == 0 || gt_rows == 1 || gt_rows == m->N,
                    "vrx_model_set_prior: GT_prior must have 0, 1 or n_var rows (got %lld)",
                    (long long)gt_rows);
        VRX_REQUIRE(gt_rows == 0 || GT_prior, "vrx_model_set_prior: null GT_prior");
        if ((rc = set_log_prior(m, m->logq_gt, m->gt_mode, GT_prior, gt_rows, m->K, m->T))) return rc;
    }
    VRX_REQUIRE(s1_prior && s2_prior, "vrx_model_set_prior: null theta prior");
    VRX_REQUIRE(theta_prior_rows == 1 || theta_prior_rows == m->th_rows,
                "vrx_model_set_prior: theta prior rows must be 1 or %lld", (long long)m->th_rows);
    m->prior_rows = theta_prior_rows;
    const size_t n = (size_t)(theta_prior_rows * m->th_cols);
    if ((rc = h2d(m, m->prior1, s1_prior, n))) return rc;
    if ((rc = h2d(m, m->prior2, s2_prior, n))) return rc;
    VRX_HIP(hipStreamSynchronize(m->p->stream));
    return VRX_OK;
}

// ------------------------------------------------------------------------------------
// launches
// ------------------------------------------------------------------------------------
template <int LPE, int CPL, int MODE>
static void launch_spmm_fmt(const Orient& o, dim3 grid, hipStream_t s, const double* X, int K,
                            double* out, double* partial, const int32_t* ctl, int R,
                            const VrxCellFuse* fuse = nullptr) {
#define VRX_GO(F, FU)                                                                           \
    vrx_spmm<LPE, CPL, MODE, F, FU><<<grid, VRX_BLOCK, 0, s>>>(                                 \
        o.n_seg, o.seg_begin.p, o.seg_len.p, o.seg_dst.p, o.ent.p, X, K, out, partial, ctl, R,  \
        fuse ? *fuse : VrxCellFuse{})
    if constexpr (MODE == 1 && CPL == 1) {
        if (fuse) {  // cell pass + softmax + ELBO partials in one launch (vrx_kernels.h: FUSE = 1)
            if (o.fmt == VRX_FMT_P32)
                VRX_GO(VRX_FMT_P32, 1);
            else if (o.fmt == VRX_FMT_P64)
                VRX_GO(VRX_FMT_P64, 1);
            else
                VRX_GO(VRX_FMT_WIDE, 1);
            return;
        }
    }
    if (o.fmt == VRX_FMT_P32)
        VRX_GO(VRX_FMT_P32, 0);
    else if (o.fmt == VRX_FMT_P64)
        VRX_GO(VRX_FMT_P64, 0);
    else
        VRX_GO(VRX_FMT_WIDE, 0);
#undef VRX_GO
}

// LDS-resident pass: K <= 16 (4 columns per lane, the dense rows zero-padded to a multiple of
// 4 columns in LDS), counts < 2048 (checked when the tiled stream is built)
// (K > 16: column blocks of 16)
template <int MODE>
static bool lds_eligible(const vrx_problem& p, int K) {
    const Orient& o = MODE == 0 ? p.by_var : p.by_cell;
    if (p.device_built) return true;  // (no gather tables)
    return o.tiled.ready && K >= 2;
}

// One instance of vrx_spmm_lds: the kernel together with the template arguments it was compiled with.
// The selection below returns both from one place, so what a launch records (LdsLaunch,
// vrx_model_lds_launches) cannot drift from what it ran.
using LdsKernel = void (*)(const uint32_t*, const int64_t*, const int32_t*, const int32_t*, const int32_t*,
                           const int32_t*, int, int, int64_t, int64_t, const double*, int, int, double*,
                           const int32_t*, int, const int32_t*);
struct LdsInstance {
    LdsKernel fn;
    int mode, rw, padk, split, form;
};
template <int LPE, int MODE, int RW, int PADK, int SPLIT, int FORM = 0>
static LdsInstance lds_instance() {
    return LdsInstance{vrx_spmm_lds<LPE, MODE, RW, PADK, SPLIT, FORM>, MODE, RW, PADK, SPLIT, FORM};
}

// kernel instance for K: zero-padded rows when K % 4, 2 / 4 entries at once when K <= 8 / 4
template <int LPE, int MODE, int RW>
static LdsInstance lds_kernel_rw(int K, bool strided) {
    const int split = K <= 4 ? 4 : K <= 8 ? 2 : 1;
    // (the element-wise slab copy handles row strides and rows that do not fill whole lanes)
    const bool pad = K % (16 / LPE) != 0 || strided;
    if (split == 4) return pad ? lds_instance<LPE, MODE, RW, 1, 4>() : lds_instance<LPE, MODE, RW, 0, 4>();
    if (split == 2) return pad ? lds_instance<LPE, MODE, RW, 1, 2>() : lds_instance<LPE, MODE, RW, 0, 2>();
    return pad ? lds_instance<LPE, MODE, RW, 1, 1>() : lds_instance<LPE, MODE, RW, 0, 1>();
}

// the AD/BD form of the cell pass (FORM 1): one instance for K = 16, one that stages
// element-wise and masks its stores for every other K / column block
// (pad: 0 flat rows of 16 columns, 1 element-wise, 2 whole 16-B units -- see the kernel)
template <int RW>
static LdsInstance lds_kernel_form1(int pad) {
    if (pad == 1) return lds_instance<VRX_LDS_LPE, 1, RW, 1, 1, 1>();
    if (pad == 2) return lds_instance<VRX_LDS_LPE, 1, RW, 2, 1, 1>();
    return lds_instance<VRX_LDS_LPE, 1, RW, 0, 1, 1>();
}

// rows per wave: the pass default, or (cell pass) the shorter tile of short_tile_pays()
template <int LPE, int MODE>
static LdsInstance lds_kernel(int K, int ld, bool strided, int rw, int form) {
    // AD/BD forms: flat rows, or whole 16-B units (even K and row stride), or element-wise
    const int pad = K == 16 && !strided ? 0 : ((K | ld) & 1) == 0 ? 2 : 1;
    // (the caller has checked rw against the heights compiled for this mode and form: lds_rw_ok)
    if (MODE == 1 && form == 1) {
        return rw == VRX_LDS_RW_CELL_SHORT ? lds_kernel_form1<VRX_LDS_RW_CELL_SHORT>(pad)
                                           : lds_kernel_form1<VRX_LDS_RW_CELL>(pad);
    }
    if (MODE == 1 && rw == VRX_LDS_RW_CELL_SHORT)
        return lds_kernel_rw<LPE, MODE, MODE == 1 ? VRX_LDS_RW_CELL_SHORT : VRX_LDS_RW_VARIANT>(K, strided);
    return lds_kernel_rw<LPE, MODE, MODE == 1 ? VRX_LDS_RW_CELL_PAIR : VRX_LDS_RW_VARIANT>(K, strided);
}

// the tile heights a kernel instance exists for: a stream built with any other height would be
// walked with the wrong rows-per-wave (bnd / rowmap strides) -- refuse instead of defaulting
template <int MODE>
static bool lds_rw_ok(int rw, int form) {
    if (MODE == 1 && form == 1) return rw == VRX_LDS_RW_CELL || rw == VRX_LDS_RW_CELL_SHORT;
    if (MODE == 0) return rw == VRX_LDS_RW_VARIANT;
    return rw == VRX_LDS_RW_CELL_PAIR || rw == VRX_LDS_RW_CELL_SHORT;
}

template <int LPE, int MODE>
static int launch_lds_one(const Orient& o, hipStream_t s, const double* X, int K, double* dst,
                          const int32_t* ctl, int R, std::vector<LdsLaunch>& log) {
    const TiledStream& t = o.tiled;
    log.clear();  // (the record of this orientation's last pass)
    VRX_REQUIRE(lds_rw_ok<MODE>(t.rw, t.form),
                "LDS pass: no kernel instance for %d rows per wave (mode %d, form %d)", t.rw, MODE, t.form);
    constexpr int XD = MODE == 1 ? 2 : 1, NV = MODE == 0 ? 2 : 1;
    const unsigned grid = (unsigned)t.n_wg;  // persistent: one workgroup per CU walks its items
    // operands wider than 16 columns go through in blocks of 16 (the stream is re-read per
    // block, like the column chunks of the gather kernels)
    for (int c0 = 0; c0 < K; c0 += 16) {
        const int kb = std::min(16, K - c0);
        const bool f1 = MODE == 1 && t.form == 1;  // planar operand, 256-B LDS rows
        constexpr int CPL = 16 / LPE;  // columns per lane: LDS rows hold whole lanes
        const size_t lds = (size_t)t.slab_rows * (f1 ? 256 : (kb + CPL - 1) / CPL * CPL * (MODE == 1 ? 16 : 8)) +
                           VRX_LDS_WAVES * VRX_RING * 4;
        const LdsInstance inst = lds_kernel<LPE, MODE>(kb, K, K > 16, t.rw, t.form);
        const LdsKernel kern = inst.fn;
        VRX_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        log.push_back(LdsLaunch{inst.mode, inst.rw, inst.padk, inst.split, inst.form, kb, K, t.perm.p != nullptr,
                                t.slab_rows, t.n_slab});
        kern<<<grid, VRX_LDS_WAVES * 64, lds, s>>>(t.ent.p, t.wave_start.p, t.bnd.p, t.rowmap.p, t.items.p,
                                     t.wg_first.p, t.n_slab,
                                     t.slab_rows, t.n_contract, t.n_vrows,
                                     X + (size_t)c0 * (f1 ? 1 : XD), kb, K, dst + (size_t)c0 * NV, ctl, R,
                                     t.perm.p);  // (null: not balanced)
        VRX_HIP(hipGetLastError());
    }
    return VRX_OK;
}

template <int MODE>
static int launch_spmm_lds(vrx_model* m, const Orient& o, const double* X, int K, double* out,
                           double* range_partial, bool defer_sum) {
    hipStream_t s = m->p->stream;
    const TiledStream& t = o.tiled;
    constexpr int NV = MODE == 0 ? 2 : 1;
    if (MODE == 0 && t.virt) {
        // virtual rows: the cell pass's kernel over (variant, AD) / (variant, BD) rows and the
        // operand as double rows; planar partial sums [slot][virtual piece][K], turned into
        // S = (S1, S1 + S2) by take_S or by its consumer (vrx_theta_partial)
        return launch_lds_one<VRX_LDS_LPE, 1>(o, s, X, K, range_partial, m->ctl.p, m->R, m->lds_log[MODE]);
    }
    double* dst = t.n_range == 1 && !t.split ? out : range_partial;
    int rc;
    rc = launch_lds_one<VRX_LDS_LPE, MODE>(o, s, X, K, dst, m->ctl.p, m->R, m->lds_log[MODE]);  // K < 16 leaves lanes idle
    if (rc) return rc;
    if (t.split && !(MODE == 1 && defer_sum)) {  // rows cut into pieces: sum pieces and ranges in one fixed order
        // (the cell pass's consumer, vrx_cell_softmax, sums the pieces itself when asked to: defer_sum)
        const int64_t n = o.n_rows * K * NV;
        if ((int64_t)t.n_range * t.n_vrows >= 64 * o.n_rows)  // >= 64 terms per row on average
            vrx_sum_pieces_wave<<<(unsigned)((n * 64 + VRX_BLOCK - 1) / VRX_BLOCK), VRX_BLOCK, 0, s>>>(
                o.n_rows, K * NV, t.n_range, t.n_vrows, t.vptr.p, t.npiece.p, range_partial, out, m->ctl.p, m->R);
        else
            vrx_sum_pieces<<<(unsigned)((n + VRX_BLOCK - 1) / VRX_BLOCK), VRX_BLOCK, 0, s>>>(
                o.n_rows, K * NV, t.n_range, t.n_vrows, t.vptr.p, t.npiece.p, range_partial, out, m->ctl.p, m->R);
        VRX_HIP(hipGetLastError());
    } else if (t.n_range > 1 && !defer_sum) {
        const int64_t n = o.n_rows * K * NV;
        vrx_sum_ranges<<<(unsigned)((n + VRX_BLOCK - 1) / VRX_BLOCK), VRX_BLOCK, 0, s>>>(
            n, K * NV, t.npiece.p, range_partial, out, m->ctl.p, m->R);
        VRX_HIP(hipGetLastError());
    }
    return VRX_OK;
}

template <int MODE>
static int launch_spmm(vrx_model* m, const Orient& o, const double* X, int K, double* out,
                       double* partial, const VrxCellFuse* fuse = nullptr) {
    if (o.n_seg == 0) return VRX_OK;
    hipStream_t s = m->p->stream;
    // lanes per entry x columns per lane: 16 B per lane wherever the layout allows
    const int cpl = (MODE == 0 && K % 2 == 0) ? 2 : 1;
    const int lpe = pick_kp((K + cpl - 1) / cpl, 16 / cpl);
    const int cols = lpe * cpl;
    dim3 grid((unsigned)(o.n_seg / VRX_WAVES), (unsigned)((K + cols - 1) / cols));
    if (cpl == 2) {
        if (MODE == 0) {  // (guard keeps the CPL=2 cell-pass templates from being instantiated)
            switch (lpe) {
                case 1: launch_spmm_fmt<1, 2, 0>(o, grid, s, X, K, out, partial, m->ctl.p, m->R); break;
                case 2: launch_spmm_fmt<2, 2, 0>(o, grid, s, X, K, out, partial, m->ctl.p, m->R); break;
                case 4: launch_spmm_fmt<4, 2, 0>(o, grid, s, X, K, out, partial, m->ctl.p, m->R); break;
                default: launch_spmm_fmt<8, 2, 0>(o, grid, s, X, K, out, partial, m->ctl.p, m->R); break;
            }
        }
    } else {
        switch (lpe) {
            case 1: launch_spmm_fmt<1, 1, MODE>(o, grid, s, X, K, out, partial, m->ctl.p, m->R, fuse); break;
            case 2: launch_spmm_fmt<2, 1, MODE>(o, grid, s, X, K, out, partial, m->ctl.p, m->R, fuse); break;
            case 4: launch_spmm_fmt<4, 1, MODE>(o, grid, s, X, K, out, partial, m->ctl.p, m->R, fuse); break;
            case 8: launch_spmm_fmt<8, 1, MODE>(o, grid, s, X, K, out, partial, m->ctl.p, m->R, fuse); break;
            default: launch_spmm_fmt<16, 1, MODE>(o, grid, s, X, K, out, partial, m->ctl.p, m->R, fuse); break;
        }
    }
    VRX_HIP(hipGetLastError());
    if (o.n_multi > 0) {
        constexpr int VPE = MODE == 0 ? 2 : 1;
        const int64_t tot = o.n_multi * K * VPE;
        vrx_sum_slots<VPE><<<(unsigned)((tot + VRX_BLOCK - 1) / VRX_BLOCK), VRX_BLOCK, 0, s>>>(
            o.n_multi, K, o.multi_row.p, o.multi_ptr.p, partial, out, m->ctl.p, m->R);
        VRX_HIP(hipGetLastError());
    }
    return VRX_OK;
}

// the rows a tiled stream cut into pieces: sum of all their terms -> slot 0 of the first piece
// (vrx_fold_split), for the consumers that sum the partial arrays themselves.  NOT idempotent:
// only take_S / take_LID run it, once per deferred pass.
static int fold_split(vrx_model* m, const TiledStream& t, double* partial) {
    if (t.n_split == 0) return VRX_OK;
    const int64_t lanes = t.n_split * m->Kt * 8;  // eight lanes per (split row, column)
    vrx_fold_split<<<(unsigned)((lanes + VRX_BLOCK - 1) / VRX_BLOCK), VRX_BLOCK, 0, m->p->stream>>>(
        t.n_split, t.split_rows.p, m->Kt, t.n_vrows, t.vptr.p, t.npiece.p, partial, m->ctl.p, m->R);
    VRX_HIP(hipGetLastError());
    return VRX_OK;
}

// How a consumer reads a pass output: npiece null -- the array is final; otherwise the consumer's
// kernel sums the per-range (and per-piece) partials itself with these arguments.
struct PassSum {
    const uint16_t* npiece = nullptr;
    const double* partial = nullptr;  // (RV / RC: passed whether or not they are summed)
    int64_t n_vrows = 0;
    const int32_t* vptr = nullptr;
};

// S for its consumer.  A deferred variant pass (s_pending) leaves S as partials in RV, summed by
// exactly one consumer: f non-null -- the consumer can fuse the sum and *f gets its arguments;
// f null -- S is formed here.  Either way S is final for everything after.
static int take_S(vrx_model* m, PassSum* f) {
    const TiledStream& tv = m->p->by_var.tiled;
    if (f) {
        *f = PassSum{};
        f->partial = m->RV.p;
    }
    if (!m->s_pending) return VRX_OK;
    m->s_pending = false;
    if (f) {
        if (tv.virt && tv.split) {  // rows cut into pieces: their terms first
            int rc = fold_split(m, tv, m->RV.p);
            if (rc) return rc;
        }
        f->npiece = tv.npiece.p;
        f->n_vrows = tv.virt ? tv.n_vrows : 0;
        f->vptr = tv.virt && tv.split ? tv.vptr.p : nullptr;
        return VRX_OK;
    }
    if (tv.virt) {
        const int64_t n = m->NKt;
        vrx_s_from_virtual<<<(unsigned)((n + VRX_BLOCK - 1) / VRX_BLOCK), VRX_BLOCK, 0, m->p->stream>>>(
            m->N, m->Kt, tv.n_vrows, tv.split ? tv.vptr.p : nullptr, tv.npiece.p, m->RV.p,
            reinterpret_cast<double2*>(m->S.p), m->ctl.p, m->R);
    } else {
        const int64_t n = m->NKt * 2;
        vrx_sum_ranges<<<(unsigned)((n + VRX_BLOCK - 1) / VRX_BLOCK), VRX_BLOCK, 0, m->p->stream>>>(
            n, m->Kt * 2, tv.npiece.p, m->RV.p, m->S.p, m->ctl.p, m->R);
    }
    VRX_HIP(hipGetLastError());
    return VRX_OK;
}

// logLik_ID for its one consumer, vrx_cell_softmax, which always fuses the sum of the partials a
// deferred cell pass (l_pending) left in RC.  (n_vrows: rows of the array it reads, M when final)
static int take_LID(vrx_model* m, PassSum* f) {
    const TiledStream& tc = m->p->by_cell.tiled;
    *f = PassSum{};
    f->partial = m->RC.p;
    f->n_vrows = m->M;
    if (!m->l_pending) return VRX_OK;
    m->l_pending = false;
    if (tc.split) {  // rows cut into pieces: their terms first
        int rc = fold_split(m, tc, m->RC.p);
        if (rc) return rc;
    }
    f->npiece = tc.npiece.p;
    f->n_vrows = tc.n_vrows;
    f->vptr = tc.split ? tc.vptr.p : nullptr;
    return VRX_OK;
}

// S <- (AD @ ID_prob, DP @ ID_prob)        vireo_model.py:169-170,207-208; bmm_model.py:137-138
// defer_sum: per-range / virtual-row partials stay in RV for the consumer (take_S)
static int variant_pass(vrx_model* m, bool defer_sum = false) {
    ProfScope ps(m, VRX_KERN_VARIANT_PASS);
    if (lds_eligible<0>(*m->p, m->Kt)) {
        const TiledStream& tv = m->p->by_var.tiled;
        int rc = launch_spmm_lds<0>(m, m->p->by_var, m->ID.p, m->Kt, m->S.p, m->RV.p, true);
        if (rc) return rc;
        m->s_pending = tv.virt || (tv.n_range > 1 && !tv.split);  // (split pieces were summed above)
        return defer_sum ? VRX_OK : take_S(m, nullptr);
    }
    return launch_spmm<0>(m, m->p->by_var, m->ID.p, m->Kt, m->S.p, m->PV.p);
}

// LID <- AD^T W1 + DP^T W2                 vireo_model.py:190-196; bmm_model.py:125-129
static int cell_pass(vrx_model* m, bool defer_sum = false) {
    ProfScope ps(m, VRX_KERN_CELL_PASS);
    if (lds_eligible<1>(*m->p, m->Kt)) {
        m->l_pending = defer_sum && (m->p->by_cell.tiled.n_range > 1 || m->p->by_cell.tiled.split);
        return launch_spmm_lds<1>(m, m->p->by_cell, m->W.p, m->Kt, m->LID.p, m->RC.p, defer_sum);
    }
    return launch_spmm<1>(m, m->p->by_cell, m->W.p, m->Kt, m->LID.p, m->PC.p);
}

// Small problems (gather kernels, one restart, K <= 16, every cell exactly one segment -- none
// split, none without entries):
// the cell pass's waves hold complete logLik_ID rows, so the softmax and the cells' ELBO terms
// ride in its epilogue -- one launch less per iteration (c2: ~4 us of ~37).
static bool cell_softmax_fusable(const vrx_model* m) {
    const int on = env_int("VIREO_FUSE_SOFTMAX", 1);  // (read per call: the tests switch it)
    const Orient& o = m->p->by_cell;
    return on && m->R == 1 && m->Kt <= 16 && o.n_seg > 0 && o.n_multi == 0 && o.n_empty == 0 &&
           !lds_eligible<1>(*m->p, m->Kt);
}

static int cell_pass_softmax(vrx_model* m) {
    ProfScope ps(m, VRX_KERN_CELL_PASS);
    const Orient& o = m->p->by_cell;
    VrxCellFuse F;
    F.logq = m->logq_id.p;
    F.id_mode = m->id_mode;
    F.logq_uni = -std::log((double)m->K);
    F.ID = m->ID.p;
    F.part = m->part_cell.p;
    m->n_cell_part = (int)(o.n_seg / VRX_WAVES);
    m->dense_log[VRX_DENSE_CELL_SOURCE] = VRX_DENSE_CELL_FUSED;
    m->l_pending = false;
    return launch_spmm<1>(m, o, m->W.p, m->Kt, m->LID.p, m->PC.p, &F);
}

static VrxElboIn elbo_inputs(vrx_model* m);

static void log_elbo(vrx_model* m, const VrxElboIn& e, int carrier) {
    const int at = carrier == VRX_DENSE_ELBO_RIDE ? VRX_DENSE_RIDE_CELL : VRX_DENSE_ELBO_CELL;
    m->dense_log[at] = e.n_cell_part;
    m->dense_log[at + 1] = e.n_gt_part;
    m->dense_log[at + 2] = e.n_th_part;
    m->dense_log[VRX_DENSE_ELBO_CARRIER] = carrier;
}

// the ELBO a previous iteration left deferred (with its stop rule), as the extra block of the
// theta launch that carries it; off when none waits
static VrxElboRide take_ride(vrx_model* m) {
    VrxElboRide E{};
    if (!m->elbo_deferred) return E;
    E.on = 1;
    E.in = elbo_inputs(m);
    E.rule = m->elbo_rule;
    m->elbo_deferred = false;
    log_elbo(m, E.in, VRX_DENSE_ELBO_RIDE);
    return E;
}

// theta update (update=1) or just psi/KL from the current beta (update=0).  defer_final: the
// caller runs gt_step next, whose kernel finalises the shared theta itself (VrxThetaFuse).
static int theta_step(vrx_model* m, int update, bool defer_final = false) {
    ProfScope ps(m, VRX_KERN_DENSE);
    hipStream_t s = m->p->stream;
    const auto& c = m->cfg;
    int rc;
    if (c.kind == VRX_KIND_BMM) {
        // the range sum fuses into an update on a stream that is neither virtual nor split
        const TiledStream& tv = m->p->by_var.tiled;
        PassSum f;
        if ((rc = take_S(m, update && !tv.virt && !tv.split ? &f : nullptr))) return rc;
        // (fused range sum: 16 lanes per element; the KL partials are zero-filled past nb_nk blocks' worth)
        const unsigned nb = f.npiece ? (unsigned)((m->NK * 16 + VRX_BLOCK - 1) / VRX_BLOCK) : (unsigned)m->nb_nk;
        // the previous iteration's ELBO + stop rule reads the KL_theta partials of the half this
        // launch does not write
        const VrxElboRide E = take_ride(m);
        m->th_cur ^= 1;
        m->n_th_part = (int)nb;
        m->dense_log[VRX_DENSE_NB_THETA] = (int32_t)nb;
        vrx_bmm_theta<<<dim3(nb + E.on, m->R), VRX_BLOCK, 0, s>>>(
            m->NK, update, c.fix_beta_sum, reinterpret_cast<double2*>(m->S.p), f.npiece,
            reinterpret_cast<const double2*>(m->RV.p), m->prior1.p,
            m->prior2.p, m->prior_rows == 1 ? 0 : 1, m->mu.p, m->sm.p, m->W.p, m->K, m->wform,
            m->part_th.p + (size_t)m->th_cur * m->th_cap, m->batch(), m->ctl.p, E);
        m->w_valid = true;
    } else if (c.ase_mode) {
        if ((rc = take_S(m, nullptr))) return rc;  // (the ASE kernel does not fuse the range sum)
        m->dense_log[VRX_DENSE_NB_THETA] = m->nb_throws;
        vrx_theta_ase<<<dim3(m->nb_throws, m->R), VRX_BLOCK, 0, s>>>(
            m->N, m->K, m->T, update, c.fix_beta_sum, reinterpret_cast<const double2*>(m->S.p),
            m->GT.p, m->prior1.p, m->prior2.p, (int)m->prior_rows, m->mu.p, m->sm.p, m->psi.p,
            m->part_th.p, m->batch(), m->ctl.p);
        m->w_valid = false;
    } else {
        if (update) {
            PassSum f;
            if ((rc = take_S(m, &f))) return rc;  // every layout fuses here
            auto* kern = m->T == 3 ? vrx_theta_partial<3> : vrx_theta_partial<VRX_MAXT>;
            const VrxElboRide E = take_ride(m);  // the previous iteration's ELBO + stop rule: one extra block
            m->dense_log[VRX_DENSE_NB_THETA] = m->nb_theta;
            kern<<<dim3(m->nb_theta + E.on, m->R), VRX_BLOCK, 0, s>>>(
                m->NK, m->T, reinterpret_cast<double2*>(m->S.p), f.npiece,
                reinterpret_cast<const double2*>(f.partial), f.n_vrows, f.vptr,
                m->GT.p, m->part_theta.p, m->batch(), m->ctl.p, E);
            VRX_HIP(hipGetLastError());
        }
        // Worth it only while the partials are few: every block of vrx_gt_update re-reads them
        // (c2, 157 partials: 43.4 -> 41.9 us per iteration; c3, 1024 partials = 128 KB per
        // block: 0.994 -> 1.012 ms, so large problems keep the separate one-block kernel).
        static const int fuse_max = env_int("VIREO_FUSE_THETA_MAX_PARTS", 256);
        if (update && defer_final && m->nb_theta <= fuse_max) {
            m->theta_pending = true;
        } else {
            if (update) {
                m->dense_log[VRX_DENSE_THETA_FINAL] = VRX_DENSE_THETA_KERNEL;
                m->dense_log[VRX_DENSE_THETA_PARTS] = m->nb_theta;
            }
            vrx_theta_final<<<m->R, VRX_BLOCK, 0, s>>>(m->nb_theta, m->T, update, c.fix_beta_sum,
                                                     m->part_theta.p, m->prior1.p, m->prior2.p,
                                                     m->mu.p, m->sm.p, m->psi.p, m->part_th.p, m->ctl.p);
        }
        m->w_valid = false;
    }
    VRX_HIP(hipGetLastError());
    return VRX_OK;
}

// GT softmax (learn=1) or W/KL from the fixed GT (learn=0); always refreshes W
static int gt_step(vrx_model* m, int learn) {
    ProfScope ps(m, VRX_KERN_DENSE);
    if (learn) {
        int rc = take_S(m, nullptr);
        if (rc) return rc;
    }
    VrxThetaFuse F{};
    if (m->theta_pending) {
        F.on = 1;
        F.n_part = m->nb_theta;
        F.fix_sum = m->cfg.fix_beta_sum;
        F.part = m->part_theta.p;
        F.prior1 = m->prior1.p;
        F.prior2 = m->prior2.p;
        F.mu = m->mu.p;
        F.sm = m->sm.p;
        F.psi = m->psi.p;
        F.kl_out = m->part_th.p;
        m->theta_pending = false;
        m->dense_log[VRX_DENSE_THETA_FINAL] = VRX_DENSE_THETA_FUSED;
        m->dense_log[VRX_DENSE_THETA_PARTS] = F.n_part;
    }
    m->dense_log[VRX_DENSE_NB_GT] = m->nb_gt;
    auto* kern = m->T == 3 ? vrx_gt_update<3> : vrx_gt_update<VRX_MAXT>;
    kern<<<dim3(m->nb_gt, m->R), VRX_BLOCK, 0, m->p->stream>>>(
        m->NK, m->K, m->T, learn, m->cfg.ase_mode, m->N, reinterpret_cast<const double2*>(m->S.p),
        m->psi.p, m->logq_gt.p, m->gt_mode, -std::log((double)m->T), m->GT.p, m->W.p, m->wform,
        m->part_gt.p, F, m->batch(), m->ctl.p);
    VRX_HIP(hipGetLastError());
    m->w_valid = true;
    return VRX_OK;
}

static VrxElboIn elbo_inputs(vrx_model* m) {
    VrxElboIn e;
    e.cell_part = m->part_cell.p;
    e.gt_part = m->part_gt.p;
    e.th_part = m->part_th.p + (size_t)m->th_cur * m->th_cap;
    e.n_cell_part = m->n_cell_part;  // (of the kernel that formed them last)
    e.n_gt_part = m->cfg.kind == VRX_KIND_VIREO ? m->nb_gt : 0;
    e.n_th_part = m->n_th_part;
    e.elbo = m->d_elbo.p;
    e.parts = m->d_parts.p;
    e.trace_stride = m->trace_cap;
    return e;
}

static VrxStopRule no_rule(int slot) {
    VrxStopRule r;
    r.it = slot;
    r.min_iter = r.max_iter = r.active = 0;
    r.eps = 0.0;
    r.form = VRX_STOP_VIREO;  // (never judged)
    return r;
}

static int softmax_step(vrx_model* m, int update) {
    ProfScope ps(m, VRX_KERN_DENSE);
    hipStream_t s = m->p->stream;
    const double lu = -std::log((double)m->K);
    PassSum f;  // (fused sum of the partials, of the pieces of long rows too)
    int rc = take_LID(m, &f);
    if (rc) return rc;
    m->n_cell_part = m->nb_cell;
    m->dense_log[VRX_DENSE_NB_CELL] = m->nb_cell;
    m->dense_log[VRX_DENSE_KP] = m->KP;
    m->dense_log[VRX_DENSE_CELL_SOURCE] = VRX_DENSE_CELL_SOFTMAX;
#define VRX_SM_CASE(KPV)                                                                        \
    case KPV:                                                                                   \
        vrx_cell_softmax<KPV><<<dim3(m->nb_cell, m->R), VRX_BLOCK, 0, s>>>(                     \
            m->M, m->K, update, m->LID.p, f.npiece, f.partial, f.vptr, f.n_vrows, m->logq_id.p, m->id_mode, lu, \
            m->ID.p, m->part_cell.p, m->batch(), m->ctl.p);                                     \
        break;
    switch (m->KP) {
        VRX_SM_CASE(1)
        VRX_SM_CASE(2)
        VRX_SM_CASE(4)
        VRX_SM_CASE(8)
        VRX_SM_CASE(16)
        VRX_SM_CASE(32)
        VRX_SM_CASE(64)
    }
#undef VRX_SM_CASE
    VRX_HIP(hipGetLastError());
    return VRX_OK;
}

// ELBO of iteration rule.it into the trace; evaluates the stop rule when it is active
static int elbo_step(vrx_model* m, const VrxStopRule& rule) {
    ProfScope ps(m, VRX_KERN_DENSE);
    const VrxElboIn in = elbo_inputs(m);
    log_elbo(m, in, VRX_DENSE_ELBO_KERNEL);
    vrx_elbo_final<<<m->R, VRX_BLOCK, 0, m->p->stream>>>(in, rule, m->ctl.p);
    VRX_HIP(hipGetLastError());
    return VRX_OK;
}

// One iteration of _fit_VB (vireo_model.py:257-264) / _fit_BV (bmm_model.py:183-188).
// Enqueue only; no host synchronisation.
// an ELBO that still waits for a ride is finalised by the kernel of its own after all
static int flush_elbo(vrx_model* m) {
    if (!m->elbo_deferred) return VRX_OK;
    m->elbo_deferred = false;
    return elbo_step(m, m->elbo_rule);
}

// shared-theta Vireo updates run vrx_theta_partial, which can carry the previous iteration's ELBO
// (rule: the stop rule of the fit, inactive for vrx_model_run_iters)
static bool elbo_can_ride(const vrx_model* m, const VrxStopRule& rule) {
    // Only where an iteration is short against a launch: when the rule fires, the next iteration's
    // variant pass has already run for nothing -- 8 us at c2 (a 29-us iteration minus 3 us, every
    // iteration), 0.3 ms at c3 (where one ELBO kernel per iteration is 1 % of it and a fit would
    // need > 30 iterations to win the wasted pass back).  Measured gain at nnz x columns = 2 / 8 /
    // 16 / 32 M: 10.5 / 6 / 4 / 2.8 % per iteration (profiles/r05_ab_elbo_ride_small_problems.txt);
    // the default stops at 2^25.  VIREO_ELBO_RIDE=0 / 1 forces it off / on (read per call).
    // Clone mode rides in vrx_bmm_theta, for the iterations whose stop rule cannot fire (it <=
    // min_iter, see enqueue_iterations): its fits run min_iter >= 20 iterations by default
    // (bmm_model.py:178), so there the rule is min_iter, not size -- nothing is ever wasted;
    // without a stop rule nothing is wasted either.
    const auto& c = m->cfg;
    if (c.kind == VRX_KIND_VIREO && (c.ase_mode || !c.learn_theta)) return false;
    const bool small = m->p->nnz * (int64_t)m->Kt < ((int64_t)1 << 25);
    const bool dflt = small || (c.kind == VRX_KIND_BMM && (!rule.active || rule.min_iter >= 12));
    return env_int("VIREO_ELBO_RIDE", dflt ? 1 : 0) != 0;
}

// defer_elbo: the caller enqueues an iteration WITH the theta update right behind this one
static int enqueue_iteration(vrx_model* m, bool do_theta, const VrxStopRule& rule, bool defer_elbo = false) {
    int rc;
    const auto& c = m->cfg;
    if (m->elbo_deferred && !(c.kind == VRX_KIND_BMM || (do_theta && !c.ase_mode)))
        if ((rc = flush_elbo(m))) return rc;  // (not reached by the callers below: they defer only in front of a ride)
    if (c.kind == VRX_KIND_BMM) {
        if ((rc = variant_pass(m, true))) return rc;
        if ((rc = theta_step(m, 1))) return rc;  // also refreshes W (digamma tables)
    } else {
        bool have_s = false;
        if (do_theta) {
            if ((rc = variant_pass(m, true))) return rc;  // range sum fused into the theta kernel
            have_s = true;
            if ((rc = theta_step(m, 1, true))) return rc;  // (a gt_step always follows)
        }
        if (c.learn_gt) {
            // the reference recomputes AD@ID_prob, DP@ID_prob here (vireo_model.py:207-208);
            // ID_prob has not changed since update_theta_size, so S is reused.
            if (!have_s)
                if ((rc = variant_pass(m, true))) return rc;
            if ((rc = gt_step(m, 1))) return rc;
        } else if (!m->w_valid) {
            if ((rc = gt_step(m, 0))) return rc;
        }
    }
    if (cell_softmax_fusable(m)) {
        if ((rc = cell_pass_softmax(m))) return rc;
    } else {
        if ((rc = cell_pass(m, true))) return rc;  // range sum fused into the softmax kernel
        if ((rc = softmax_step(m, 1))) return rc;
    }
    if (defer_elbo) {  // finalised by the next iteration's vrx_theta_partial (theta_step)
        m->elbo_deferred = true;
        m->elbo_rule = rule;
        return VRX_OK;
    }
    return elbo_step(m, rule);                 // ELBO + the stop rule, on the device
}

// The iterations of a fit or of a timed run: which update theta, and which leave their ELBO to
// ride in the next iteration's theta launch
struct Schedule {
    VrxStopRule rule;  // (rule.it is set per iteration; active = 0: no stop rule)
    int theta_from;    // the first iteration that updates theta (delay_fit_theta)
    bool ride;         // elbo_can_ride, read once per call
};

static bool updates_theta(const vrx_model* m, const Schedule& sc, int it) {
    return m->cfg.kind == VRX_KIND_VIREO && m->cfg.learn_theta && it >= sc.theta_from;
}

// Iterations [from, to).  The last one finalises its own ELBO (a fit's poll reads its stop word).
static int enqueue_iterations(vrx_model* m, const Schedule& sc, int from, int to) {
    for (int it = from; it < to; ++it) {
        VrxStopRule rule = sc.rule;
        rule.it = it;
        // Vireo: an ELBO rides when the next iteration updates theta -- vrx_theta_partial writes
        // S and partial sums only; the kernels that write state run behind the rider.
        // Clone mode: vrx_bmm_theta WRITES model state (beta_mu, beta_sum, W), and its ordinary
        // blocks read the stop word before the rider in the same launch has judged the previous
        // iteration -- a stop found there would leave theta one update ahead of what
        // bmm_model.py:190-199 breaks out with.  So an ELBO rides only while its rule cannot
        // fire (it <= min_iter: `judge` of vrx_elbo_final_block is false); from min_iter + 1 on
        // every iteration finalises its own.
        const bool next_carries = m->cfg.kind == VRX_KIND_BMM ? !(rule.active && it > rule.min_iter)
                                                               : updates_theta(m, sc, it + 1);
        const bool defer = sc.ride && it + 1 < to && next_carries;
        int rc = enqueue_iteration(m, updates_theta(m, sc, it), rule, defer);
        if (rc) return rc;
    }
    return VRX_OK;
}

static int reset_ctl(vrx_model* m) {  // stop flag, stop iteration, warn flags (tickets stay 0)
    m->elbo_deferred = false;  // (a call that failed half-way may have left one waiting: dropped)
    VRX_HIP(hipMemsetAsync(m->ctl.p, 0, (size_t)m->R * VRX_CTL_WORDS * sizeof(int32_t), m->p->stream));
    return VRX_OK;
}

// the start of a fit / run of n iterations: an ELBO trace that holds them, clean control words,
// psi / KL_theta (and, for fixed GT or BMM, W) consistent with the state just uploaded
static int prepare(vrx_model* m, int64_t n) {
    int rc;
    if ((rc = ensure_trace(m, n))) return rc;
    if ((rc = reset_ctl(m))) return rc;
    if ((rc = theta_step(m, 0))) return rc;
    if (m->cfg.kind == VRX_KIND_VIREO && !m->cfg.learn_gt)
        if ((rc = gt_step(m, 0))) return rc;
    return VRX_OK;
}

extern "C" int vrx_model_fit(vrx_model* m, int32_t max_iter, int32_t min_iter, double eps,
                             int32_t delay_fit_theta, double* elbo_trace, int32_t* it_out,
                             int32_t* warn_flags) {
    VRX_REQUIRE(m && elbo_trace && it_out, "vrx_model_fit: null argument");
    VRX_REQUIRE(max_iter >= 1, "vrx_model_fit: max_iter must be >= 1");
    VRX_HIP(hipSetDevice(m->p->device));
    hipStream_t s = m->p->stream;
    int rc;
    // (the reference takes any max_iter, vireo_model.py:251: its trace is np.zeros(max_iter))
    if ((rc = prepare(m, max_iter))) return rc;
    // The stop rule runs on the device (vrx_elbo_final_block); the host enqueues a batch of
    // iterations, then reads three control words.  The first batch reaches the first iteration
    // the rule can fire at (min_iter + 1); a kernel launched after the stop returns at once, so
    // an overshoot costs launches, not work.
    static const int batch = std::max(1, env_int("VIREO_FIT_BATCH", 4));
    // Polls are PIPELINED: batch b + 1 is enqueued before the host waits for the control words
    // batch b left, so the device never idles between batches (a 20-iteration restart used to
    // pay five drained queues).  VIREO_FIT_PIPELINE=0: wait before enqueuing, as before.
    // A batch enqueued behind the one that stopped costs its launches (batch x ~5-10 no-op kernels,
    // drained by the final synchronisation): on launch-bound problems that is more than the drained
    // queues it saves (c2, 32 one-restart fits: 24.8 ms pipelined against 23.1 ms,
    // profiles/r05_ab_pipeline_small_problems.txt), so the default pipelines only where an
    // iteration is long against a launch -- the criterion restarts.restart_batch uses.
    // VIREO_FIT_PIPELINE=1 / 0 forces it on / off (read per call: the tests switch it).
    const int pipeline = env_int("VIREO_FIT_PIPELINE", m->p->nnz * (int64_t)m->Kt >= ((int64_t)1 << 24) ? 1 : 0);
    VrxStopRule rule;
    rule.it = 0;
    rule.min_iter = min_iter;
    rule.max_iter = max_iter;
    rule.active = 1;
    rule.eps = eps;
    rule.form = vrx_stop_form_of_kind(m->cfg.kind);
    const Schedule sc{rule, delay_fit_theta, elbo_can_ride(m, rule)};
    const int R = m->R;  // elbo_trace [R][max_iter], it_out [R], warn_flags [R]
    // two pinned read-back buffers of R * VRX_CTL_WORDS <= 64 words inside h_pin (64 doubles)
    int32_t* hbuf[2] = {reinterpret_cast<int32_t*>(m->h_pin), reinterpret_cast<int32_t*>(m->h_pin) + 64};
    for (int b = 0; b < 2; ++b)
        if (!m->polled[b]) VRX_HIP(hipEventCreateWithFlags(&m->polled[b], hipEventDisableTiming));
    int next = 0, nb = 0;
    auto enqueue_batch = [&]() -> int {  // iterations [next, upto) + the read-back of their control words
        const int upto = std::min(max_iter, next == 0 ? std::max(min_iter + 2, batch) : next + batch);
        int rc2 = enqueue_iterations(m, sc, next, upto);
        if (rc2) return rc2;
        next = upto;
        VRX_HIP(hipMemcpyAsync(hbuf[nb & 1], m->ctl.p, (size_t)R * VRX_CTL_WORDS * sizeof(int32_t),
                               hipMemcpyDeviceToHost, s));
        VRX_HIP(hipEventRecord(m->polled[nb & 1], s));
        ++nb;
        return VRX_OK;
    };
    if ((rc = enqueue_batch())) return rc;
    int32_t* hctl = hbuf[0];
    for (int b = 0;; ++b) {  // b: the batch whose control words are read next
        if (pipeline && next < max_iter)
            if ((rc = enqueue_batch())) return rc;  // (no-ops if batch b turns out to have stopped)
        VRX_HIP(hipEventSynchronize(m->polled[b & 1]));
        hctl = hbuf[b & 1];
        bool stopped = true;  // the batch runs until its last restart has stopped
        for (int r = 0; r < R; ++r) stopped = stopped && hctl[r * VRX_CTL_WORDS + VRX_CTL_STOP] != 0;
        if (stopped) break;
        if (b + 1 == nb) {  // nothing in flight behind batch b
            if (next >= max_iter) break;
            if ((rc = enqueue_batch())) return rc;
        }
    }
    // (a batch enqueued behind the one that stopped changes nothing: its kernels return at once,
    //  the control words are final; the sync below drains it)
    bool any_stop = false;
    for (int r = 0; r < R; ++r) {
        const int32_t* c = hctl + r * VRX_CTL_WORDS;
        any_stop = any_stop || c[VRX_CTL_STOP] != 0;
        // Python leaves `it` at the last executed index
        const int it = c[VRX_CTL_STOP] ? c[VRX_CTL_IT] : max_iter - 1;
        it_out[r] = it;
        if (warn_flags) warn_flags[r] = c[VRX_CTL_WARN];
        VRX_HIP(hipMemcpyAsync(elbo_trace + (size_t)r * max_iter, m->d_elbo.p + (size_t)r * m->trace_cap,
                               (size_t)(it + 1) * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    VRX_HIP(hipStreamSynchronize(s));
    if (any_stop) {  // the launches behind a stop did nothing; the next call starts clean
        if ((rc = reset_ctl(m))) return rc;
    }
    return prof_drain(m);
}

extern "C" int vrx_model_run_iters(vrx_model* m, int32_t n_iter, int32_t theta_from_iter,
                                   double* elbo_trace, double* ms_out) {
    VRX_REQUIRE(m && n_iter >= 1, "vrx_model_run_iters: bad argument");
    VRX_HIP(hipSetDevice(m->p->device));
    hipStream_t s = m->p->stream;
    int rc;
    if ((rc = prepare(m, n_iter))) return rc;
    const Schedule sc{no_rule(0), theta_from_iter, elbo_can_ride(m, no_rule(0))};  // (no stop rule)
    VRX_HIP(hipEventRecord(m->t0, s));
    if ((rc = enqueue_iterations(m, sc, 0, n_iter))) return rc;
    VRX_HIP(hipEventRecord(m->t1, s));
    VRX_HIP(hipStreamSynchronize(s));
    float ms = 0.f;
    VRX_HIP(hipEventElapsedTime(&ms, m->t0, m->t1));
    if (ms_out) *ms_out = ms;
    if (elbo_trace)  // [R][n_iter]
        for (int r = 0; r < m->R; ++r)
            VRX_HIP(hipMemcpy(elbo_trace + (size_t)r * n_iter, m->d_elbo.p + (size_t)r * m->trace_cap,
                              (size_t)n_iter * sizeof(double), hipMemcpyDeviceToHost));
    return prof_drain(m);
}

extern "C" int vrx_model_step(vrx_model* m, int32_t which, double* elbo_out) {
    VRX_REQUIRE(m, "vrx_model_step: null model");
    VRX_HIP(hipSetDevice(m->p->device));
    hipStream_t s = m->p->stream;
    const auto& c = m->cfg;
    int rc;
    if ((rc = reset_ctl(m))) return rc;
    switch (which) {
        case VRX_STEP_THETA:
            if ((rc = variant_pass(m))) return rc;
            if ((rc = theta_step(m, 1))) return rc;
            break;
        case VRX_STEP_GT:
            VRX_REQUIRE(c.kind == VRX_KIND_VIREO, "vrx_model_step: GT step needs a Vireo model");
            if ((rc = theta_step(m, 0))) return rc;
            if ((rc = variant_pass(m))) return rc;
            if ((rc = gt_step(m, 1))) return rc;
            break;
        case VRX_STEP_ID:
        case VRX_STEP_LOGLIK:
            if ((rc = theta_step(m, 0))) return rc;  // BMM: refreshes W as well
            if (c.kind == VRX_KIND_VIREO)
                if ((rc = gt_step(m, 0))) return rc;
            if ((rc = cell_pass(m))) return rc;
            if (which == VRX_STEP_ID)
                if ((rc = softmax_step(m, 1))) return rc;
            break;
        case VRX_STEP_SOFTMAX:
            if ((rc = softmax_step(m, 1))) return rc;
            break;
        case VRX_STEP_ELBO:
            VRX_REQUIRE(elbo_out, "vrx_model_step: null elbo_out");
            if ((rc = theta_step(m, 0))) return rc;
            if (c.kind == VRX_KIND_VIREO)
                if ((rc = gt_step(m, 0))) return rc;
            if ((rc = softmax_step(m, 0))) return rc;
            if ((rc = elbo_step(m, no_rule(0)))) return rc;
            for (int r = 0; r < m->R; ++r)  // elbo_out [R]
                VRX_HIP(hipMemcpyAsync(m->h_pin + r, m->d_elbo.p + (size_t)r * m->trace_cap, sizeof(double),
                                       hipMemcpyDeviceToHost, s));
            VRX_HIP(hipStreamSynchronize(s));
            for (int r = 0; r < m->R; ++r) elbo_out[r] = m->h_pin[r];
            break;
        default:
            vrx_set_error("vrx_model_step: unknown step %d", which);
            return VRX_ERR_ARG;
    }
    VRX_HIP(hipStreamSynchronize(s));
    return prof_drain(m);
}

extern "C" int vrx_model_info(vrx_model* m, int32_t* info) {
    VRX_REQUIRE(m && info, "vrx_model_info: null argument");
    const Orient &v = m->p->by_var, &c = m->p->by_cell;
    info[0] = lds_eligible<0>(*m->p, m->Kt);
    info[1] = lds_eligible<1>(*m->p, m->Kt);
    info[2] = v.fmt;
    info[3] = c.fmt;
    info[4] = v.n_tiles;
    info[5] = c.n_tiles;
    info[6] = v.tiled.ready ? v.tiled.n_range : 0;
    info[7] = c.tiled.ready ? c.tiled.n_range : 0;
    info[8] = v.tiled.ready ? (int32_t)(v.tiled.pad_ratio * 1000.0 + 0.5) : 0;
    info[9] = c.tiled.ready ? (int32_t)(c.tiled.pad_ratio * 1000.0 + 0.5) : 0;
    info[10] = v.tiled.ready ? (int32_t)(v.tiled.n_vrows - (v.tiled.virt ? 2 : 1) * v.n_rows) : 0;
    info[11] = c.tiled.ready ? (int32_t)(c.tiled.n_vrows - c.n_rows) : 0;
    info[12] = c.tiled.ready ? c.tiled.form : 0;
    info[13] = v.tiled.ready ? (v.tiled.virt ? 3 : v.tiled.form) : 0;  // 3: AD/BD virtual rows
    info[14] = m->R;
    // longest wave stream / mean wave stream of each pass, x 1000: variant in the low, cell in the high half
    const int32_t iv = v.tiled.ready ? (int32_t)std::min(65535.0, v.tiled.imbalance * 1000.0 + 0.5) : 0;
    const int32_t ic = c.tiled.ready ? (int32_t)std::min(32767.0, c.tiled.imbalance * 1000.0 + 0.5) : 0;
    info[15] = iv | (ic << 16);
    return VRX_OK;
}

extern "C" int vrx_model_lds_launches(vrx_model* m, int32_t orient, int32_t* out, int32_t cap, int32_t* n_out) {
    VRX_REQUIRE(m && n_out && (out || cap == 0), "vrx_model_lds_launches: null argument");
    VRX_REQUIRE((orient == 0 || orient == 1) && cap >= 0, "vrx_model_lds_launches: orientation %d, room for %d",
                orient, cap);
    const std::vector<LdsLaunch>& log = m->lds_log[orient];
    static_assert(sizeof(LdsLaunch) == VRX_LDS_LAUNCH_FIELDS * sizeof(int32_t), "a record is its fields");
    const size_t n = std::min(log.size(), (size_t)cap);
    if (n) memcpy(out, log.data(), n * sizeof(LdsLaunch));
    *n_out = (int32_t)log.size();
    return VRX_OK;
}

extern "C" int vrx_model_dense_launches(vrx_model* m, int32_t* out) {
    VRX_REQUIRE(m && out, "vrx_model_dense_launches: null argument");
    m->dense_log[VRX_DENSE_N_CU] = m->p->n_cu;
    memcpy(out, m->dense_log, sizeof(m->dense_log));
    return VRX_OK;
}

extern "C" int vrx_model_profile(vrx_model* m, int32_t enable) {
    VRX_REQUIRE(m, "vrx_model_profile: null model");
    VRX_HIP(hipSetDevice(m->p->device));
    if (enable && m->ev.empty()) {
        m->ev.resize(2 * kEventPairs);
        m->ev_kind.resize(kEventPairs);
        for (auto& e : m->ev) VRX_HIP(hipEventCreate(&e));
    }
    m->prof = enable != 0;
    m->ev_used = 0;
    for (int i = 0; i < VRX_KERN_COUNT; ++i) {
        m->prof_ms[i] = 0.0;
        m->prof_n[i] = 0;
    }
    return VRX_OK;
}

extern "C" int vrx_model_profile_read(vrx_model* m, double* ms_total, int64_t* launches) {
    VRX_REQUIRE(m && ms_total && launches, "vrx_model_profile_read: null argument");
    VRX_HIP(hipSetDevice(m->p->device));
    int rc = prof_drain(m);
    if (rc) return rc;
    for (int i = 0; i < VRX_KERN_COUNT; ++i) {
        ms_total[i] = m->prof_ms[i];
        launches[i] = m->prof_n[i];
    }
    return VRX_OK;
}

// ------------------------------------------------------------------------------------
// one-shot cell log-likelihood against caller-supplied tables (doublet step)
// ------------------------------------------------------------------------------------
// psi1 / psi2 / psis, th values each -> the three planes of psi
static int upload_psi(hipStream_t s, double* psi, const double* psi1, const double* psi2,
                      const double* psis, size_t th) {
    const double* src[3] = {psi1, psi2, psis};
    for (int i = 0; i < 3; ++i)
        VRX_HIP(hipMemcpyAsync(psi + i * th, src[i], th * sizeof(double), hipMemcpyHostToDevice, s));
    return VRX_OK;
}

// W is in place: cell pass -> logLik; with prob_out, the ID prior and the softmax -> posterior
static int loglik_and_posterior(vrx_model* m, const double* ID_prior, int64_t id_rows, double* logLik,
                                double* prob_out) {
    int rc;
    if ((rc = cell_pass(m))) return rc;
    if ((rc = d2h(m, logLik, m->LID, (size_t)(m->M * m->K)))) return rc;
    if (prob_out) {
        if ((rc = set_log_prior(m, m->logq_id, m->id_mode, ID_prior, id_rows, 1, m->K))) return rc;
        if ((rc = softmax_step(m, 1))) return rc;
        if ((rc = d2h(m, prob_out, m->ID, (size_t)(m->M * m->K)))) return rc;
    }
    VRX_HIP(hipStreamSynchronize(m->p->stream));
    return VRX_OK;
}

extern "C" int vrx_problem_doublet(vrx_problem* p, int64_t n_donor, int64_t n_gt,
                                   const double* GT_prob, const double* psi1, const double* psi2,
                                   const double* psis, int64_t psi_rows, const double* ID_prior,
                                   int64_t id_rows, double* logLik, double* prob_out) {
    VRX_REQUIRE(p && GT_prob && psi1 && psi2 && psis && logLik, "vrx_problem_doublet: null argument");
    VRX_REQUIRE(n_donor >= 2 && n_gt >= 1 && n_gt <= VRX_MAXT,
                "vrx_problem_doublet: needs n_donor >= 2 and 1 <= n_GT <= %d", VRX_MAXT);
    VRX_REQUIRE(psi_rows == 1 || psi_rows == p->n_var, "vrx_problem_doublet: psi rows must be 1 or n_var");
    const int64_t C = n_donor + n_donor * (n_donor - 1) / 2;
    const int G = (int)(n_gt + n_gt * (n_gt - 1) / 2);
    VRX_REQUIRE(id_rows == 0 || id_rows == 1 || id_rows == p->n_cell,
                "vrx_problem_doublet: ID_prior must have 0, 1 or n_cell rows");
    VRX_REQUIRE(id_rows == 0 || ID_prior, "vrx_problem_doublet: null ID_prior");
    vrx_model_cfg cfg{};
    cfg.kind = VRX_KIND_VIREO;
    cfg.n_donor = (int32_t)C;
    cfg.n_gt = 1;  // the pair classes live in registers; no N x C x G tensor
    vrx_model* m = nullptr;
    int rc = vrx_model_create(p, &cfg, &m);
    if (rc) return rc;
    std::unique_ptr<vrx_model> guard(m);
    hipStream_t s = p->stream;
    DevBuf<double> gt, psi;
    DevBuf<int2> pairs;
    std::vector<int2> hp;
    for (int a = 0; a < n_donor; ++a)
        for (int b = a + 1; b < n_donor; ++b) hp.push_back(make_int2(a, b));  // combinations order
    const size_t n_gt_el = (size_t)(p->n_var * n_donor * n_gt), th = (size_t)(psi_rows * G);
    VRX_HIP(gt.upload(GT_prob, n_gt_el, s));
    VRX_HIP(pairs.upload(hp.data(), hp.size(), s));
    VRX_HIP(psi.alloc(3 * th));
    if ((rc = upload_psi(s, psi.p, psi1, psi2, psis, th))) return rc;
    const int64_t n = p->n_var * C;
    vrx_doublet_w<<<(unsigned)((n + VRX_BLOCK - 1) / VRX_BLOCK), VRX_BLOCK, 0, s>>>(
        p->n_var, (int)n_donor, (int)n_gt, (int)C, psi_rows == 1 ? 0 : 1, gt.p, pairs.p, psi.p,
        psi.p + th, psi.p + 2 * th, m->W.p, m->wform);
    VRX_HIP(hipGetLastError());
    return loglik_and_posterior(m, ID_prior, id_rows, logLik, prob_out);
}

extern "C" int vrx_problem_donor_reads(vrx_problem* p, int64_t n_col, const double* ID_prob,
                                       double* AD_reads, double* DP_reads) {
    VRX_REQUIRE(p && ID_prob && AD_reads && DP_reads, "vrx_problem_donor_reads: null argument");
    VRX_REQUIRE(n_col >= 1, "vrx_problem_donor_reads: bad shape");
    vrx_model_cfg cfg{};
    cfg.kind = VRX_KIND_BMM;  // no genotype layer needed: only ID_prob and S
    cfg.n_donor = (int32_t)n_col;
    vrx_model* m = nullptr;
    int rc = vrx_model_create(p, &cfg, &m);
    if (rc) return rc;
    std::unique_ptr<vrx_model> guard(m);
    if ((rc = h2d(m, m->ID, ID_prob, (size_t)(m->M * m->K)))) return rc;
    if ((rc = variant_pass(m))) return rc;
    std::vector<double> S((size_t)m->NK * 2);
    if ((rc = d2h(m, S.data(), m->S, S.size()))) return rc;
    VRX_HIP(hipStreamSynchronize(p->stream));
    for (int64_t i = 0; i < m->NK; ++i) {
        AD_reads[i] = S[(size_t)i * 2];
        DP_reads[i] = S[(size_t)i * 2 + 1];
    }
    return VRX_OK;
}

extern "C" int vrx_problem_cell_loglik(vrx_problem* p, int64_t n_col, int64_t n_class,
                                       const double* GT, const double* psi1, const double* psi2,
                                       const double* psis, int64_t psi_rows,
                                       const double* ID_prior, int64_t id_rows, double* logLik,
                                       double* prob_out) {
    VRX_REQUIRE(p && GT && psi1 && psi2 && psis && logLik, "vrx_problem_cell_loglik: null argument");
    VRX_REQUIRE(id_rows == 0 || id_rows == 1 || id_rows == p->n_cell,
                "vrx_problem_cell_loglik: ID_prior must have 0, 1 or n_cell rows");
    VRX_REQUIRE(id_rows == 0 || ID_prior, "vrx_problem_cell_loglik: null ID_prior");
    VRX_REQUIRE(n_col >= 1 && n_class >= 1, "vrx_problem_cell_loglik: bad shape");
    if (n_class > VRX_MAXT) {
        vrx_set_error("vrx_problem_cell_loglik: %lld genotype classes unsupported (max %d)",
                      (long long)n_class, VRX_MAXT);
        return VRX_ERR_UNSUPPORTED;
    }
    VRX_REQUIRE(psi_rows == 1 || psi_rows == p->n_var, "vrx_problem_cell_loglik: psi rows must be 1 or n_var");
    vrx_model_cfg cfg{};
    cfg.kind = VRX_KIND_VIREO;
    cfg.n_donor = (int32_t)n_col;
    cfg.n_gt = (int32_t)n_class;
    cfg.learn_gt = 0;
    cfg.learn_theta = 0;
    cfg.ase_mode = psi_rows == 1 ? 0 : 1;
    vrx_model* m = nullptr;
    int rc = vrx_model_create(p, &cfg, &m);
    if (rc) return rc;
    std::unique_ptr<vrx_model> guard(m);
    if ((rc = h2d(m, m->GT, GT, (size_t)m->NK * m->T))) return rc;
    if ((rc = upload_psi(p->stream, m->psi.p, psi1, psi2, psis, (size_t)(psi_rows * n_class)))) return rc;
    if ((rc = gt_step(m, 0))) return rc;
    return loglik_and_posterior(m, ID_prior, id_rows, logLik, prob_out);
}

// ---- ambient RNA (vrx_ambient.h) ------------------------------------------------------------

extern "C" int vrx_problem_elbo_gain(vrx_problem* p, int64_t n_col, const double* ID_prob,
                                     double pseudocount, double* gain) {
    VRX_REQUIRE(p && ID_prob && gain, "vrx_problem_elbo_gain: null argument");
    VRX_REQUIRE(n_col >= 1 && n_col < INT32_MAX - 1, "vrx_problem_elbo_gain: bad shape");
    // one variant pass with ID_prob and a column of ones: AD@ID, DP@ID and the row sums together
    const int64_t K1 = n_col + 1, M = p->n_cell, N = p->n_var;
    std::vector<double> id1((size_t)(M * K1));
    for (int64_t c = 0; c < M; ++c) {
        std::memcpy(&id1[(size_t)(c * K1)], ID_prob + c * n_col, (size_t)n_col * sizeof(double));
        id1[(size_t)(c * K1 + n_col)] = 1.0;
    }
    vrx_model_cfg cfg{};
    cfg.kind = VRX_KIND_BMM;  // no genotype layer needed: only ID_prob and S
    cfg.n_donor = (int32_t)K1;
    vrx_model* m = nullptr;
    int rc = vrx_model_create(p, &cfg, &m);
    if (rc) return rc;
    std::unique_ptr<vrx_model> guard(m);
    if ((rc = h2d(m, m->ID, id1.data(), id1.size()))) return rc;
    if ((rc = variant_pass(m))) return rc;
    DevBuf<double> d_gain;
    VRX_HIP(d_gain.alloc((size_t)N));
    vrx_amb_gain<<<(unsigned)((N + VRX_BLOCK - 1) / VRX_BLOCK), VRX_BLOCK, 0, p->stream>>>(
        N, (int)K1, pseudocount, m->S.p, d_gain.p);
    VRX_HIP(hipGetLastError());
    VRX_HIP(hipMemcpyAsync(gain, d_gain.p, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, p->stream));
    VRX_HIP(hipStreamSynchronize(p->stream));
    return VRX_OK;
}

template <int FMT>
static int amb_compact(vrx_problem* p, const int32_t* d_rank, DevBuf<int64_t>& sptr, DevBuf<int32_t>& ev,
                       DevBuf<int32_t>& ea, DevBuf<int32_t>& eb) {
    const int64_t M = p->n_cell;
    hipStream_t s = p->stream;
    const unsigned nb = (unsigned)((M + VRX_AMB_CELLS - 1) / VRX_AMB_CELLS);
    VRX_HIP(sptr.alloc((size_t)M + 1));
    VRX_HIP(hipMemsetAsync(sptr.p, 0, sizeof(int64_t), s));
    vrx_amb_count<FMT><<<nb, 64 * VRX_AMB_CELLS, 0, s>>>(M, p->cell_ptr.p, p->by_cell.ent.p, d_rank, sptr.p + 1);
    VRX_HIP(hipGetLastError());
    DevBuf<char> tmp;
    VRX_HIP(vrx_cub(tmp, VRX_CUB_CALL(DeviceScan::InclusiveSum, sptr.p + 1, sptr.p + 1, (size_t)M, s)));
    int64_t total = 0;
    VRX_HIP(hipMemcpyAsync(&total, sptr.p + M, sizeof total, hipMemcpyDeviceToHost, s));
    VRX_HIP(hipStreamSynchronize(s));
    VRX_HIP(ev.alloc((size_t)std::max<int64_t>(total, 1)));
    VRX_HIP(ea.alloc((size_t)std::max<int64_t>(total, 1)));
    VRX_HIP(eb.alloc((size_t)std::max<int64_t>(total, 1)));
    vrx_amb_scatter<FMT><<<nb, 64 * VRX_AMB_CELLS, 0, s>>>(M, p->cell_ptr.p, p->by_cell.ent.p, d_rank, sptr.p,
                                                           ev.p, ea.p, eb.p);
    VRX_HIP(hipGetLastError());
    return VRX_OK;
}

// theta rows of a cell's entries stay in LDS up to this budget per wave (VIREO_AMBIENT_LDS bytes):
// the most entries a cell may have to be cached, and the LDS of one wave
static void amb_plan(int K, int& cap, size_t& lds) {
    const size_t budget = (size_t)std::max(env_int("VIREO_AMBIENT_LDS", 16384), 0);
    const size_t fixed = vrx_amb_lds_bytes(K, 0);
    cap = budget > fixed ? (int)std::min<size_t>((budget - fixed) / ((size_t)(K | 1) * sizeof(double)), INT32_MAX)
                         : 0;
    lds = vrx_amb_lds_bytes(K, cap);
}

extern "C" int vrx_ambient_info(int64_t n_donor, int32_t* cap_out, int64_t* lds_bytes_out) {
    VRX_REQUIRE(cap_out && lds_bytes_out, "vrx_ambient_info: null argument");
    VRX_REQUIRE(n_donor >= 1 && n_donor <= 4096, "vrx_ambient_info: n_donor must be 1..4096");
    int cap = 0;
    size_t lds = 0;
    amb_plan((int)n_donor, cap, lds);
    *cap_out = cap;
    *lds_bytes_out = (int64_t)lds;
    return VRX_OK;
}

extern "C" int vrx_problem_ambient(vrx_problem* p, int64_t n_donor, const double* theta,
                                   const uint8_t* selected, const double* psi_init, int32_t min_iter,
                                   int32_t max_iter, double epsilon, double* psi, double* var,
                                   double* llr, int32_t* n_iter, double* ms3) {
    VRX_REQUIRE(p && theta && selected && psi_init && psi && var && llr && n_iter,
                "vrx_problem_ambient: null argument");
    VRX_REQUIRE(n_donor >= 1 && n_donor <= 4096, "vrx_problem_ambient: n_donor must be 1..4096");
    VRX_REQUIRE(max_iter >= 2 && min_iter >= 0, "vrx_problem_ambient: max_iter >= 2, min_iter >= 0");
    VRX_REQUIRE(p->cell_ptr.n == (size_t)p->n_cell + 1 && p->by_cell.ent.p, "vrx_problem_ambient: no cell entries");
    VRX_HIP(hipSetDevice(p->device));
    const int K = (int)n_donor;
    const int64_t N = p->n_var, M = p->n_cell;
    hipStream_t s = p->stream;
    // the selected rows of theta, and every variant's row among them (-1: not selected)
    std::vector<int32_t> rank((size_t)N);
    std::vector<double> th_sel;
    int32_t n_sel = 0;
    for (int64_t v = 0; v < N; ++v) {
        rank[(size_t)v] = selected[v] ? n_sel++ : -1;
        if (selected[v]) th_sel.insert(th_sel.end(), theta + v * K, theta + (v + 1) * K);
    }
    if (th_sel.empty()) th_sel.assign((size_t)K, 0.5);
    VrxQueue timer;  // four events on the problem's stream
    VRX_TRY(timer.events(4));
    DevBuf<int32_t> d_rank, ev, ea, eb;
    DevBuf<double> d_theta, d_psi0, d_psi, d_var, d_llr;
    DevBuf<int32_t> d_it;
    DevBuf<int64_t> sptr;
    VRX_HIP(d_rank.upload(rank.data(), rank.size(), s));
    VRX_HIP(d_theta.upload(th_sel.data(), th_sel.size(), s));
    VRX_HIP(d_psi0.upload(psi_init, (size_t)(M * K), s));
    VRX_HIP(d_psi.alloc((size_t)(M * K)));
    VRX_HIP(d_var.alloc((size_t)(M * K)));
    VRX_HIP(d_llr.alloc((size_t)M));
    VRX_HIP(d_it.alloc((size_t)M));
    VRX_HIP(hipEventRecord(timer.ev[0], s));
    int rc = p->by_cell.fmt == VRX_FMT_P32   ? amb_compact<VRX_FMT_P32>(p, d_rank.p, sptr, ev, ea, eb)
             : p->by_cell.fmt == VRX_FMT_P64 ? amb_compact<VRX_FMT_P64>(p, d_rank.p, sptr, ev, ea, eb)
                                             : amb_compact<VRX_FMT_WIDE>(p, d_rank.p, sptr, ev, ea, eb);
    if (rc) return rc;
    VRX_HIP(hipEventRecord(timer.ev[1], s));
    int cap = 0;
    size_t lds = 0;
    amb_plan(K, cap, lds);
    VRX_REQUIRE(lds <= 64 * 1024, "vrx_problem_ambient: %zu bytes of LDS per cell (n_donor too large)", lds);
    vrx_amb_em<<<(unsigned)M, 64, lds, s>>>(K, sptr.p, ev.p, ea.p, eb.p, d_theta.p, d_psi0.p, min_iter, max_iter,
                                            epsilon, cap, d_psi.p, d_var.p, d_llr.p, d_it.p);
    VRX_HIP(hipGetLastError());
    VRX_HIP(hipEventRecord(timer.ev[2], s));
    VRX_HIP(hipMemcpyAsync(psi, d_psi.p, (size_t)(M * K) * sizeof(double), hipMemcpyDeviceToHost, s));
    VRX_HIP(hipMemcpyAsync(var, d_var.p, (size_t)(M * K) * sizeof(double), hipMemcpyDeviceToHost, s));
    VRX_HIP(hipMemcpyAsync(llr, d_llr.p, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, s));
    VRX_HIP(hipMemcpyAsync(n_iter, d_it.p, (size_t)M * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    VRX_HIP(hipEventRecord(timer.ev[3], s));
    VRX_HIP(hipStreamSynchronize(s));
    if (ms3)
        for (int i = 0; i < 3; ++i) VRX_TRY(timer.ms(i, i + 1, &ms3[i]));
    return VRX_OK;
}

// ------------------------------------------------------------------------------------
// the stop rule (vrx_stop.h) as the device compiles it: one lane per row, for the tests
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void vrx_stop_rows(int64_t n, const int32_t* __restrict__ rows_i,
                                                     const double* __restrict__ rows_d,
                                                     int32_t* __restrict__ verdict, double* __restrict__ prev_out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int form = rows_i[4 * i], it = rows_i[4 * i + 1], min_iter = rows_i[4 * i + 2], max_iter = rows_i[4 * i + 3];
    const double eps = rows_d[3 * i], trace_prev = rows_d[3 * i + 1], cur = rows_d[3 * i + 2];
    const double prev = vrx_stop_prev(it, max_iter, trace_prev, cur);
    prev_out[i] = prev;
    verdict[i] = vrx_stop_judge(form, it, min_iter, max_iter, eps, prev, cur);
}

extern "C" int vrx_stop_verdicts(int device, int64_t n, const int32_t* rows_i, const double* rows_d,
                                 int32_t* verdict, double* prev) {
    VRX_REQUIRE(n >= 1 && n <= ((int64_t)1 << 24) && rows_i && rows_d && verdict && prev,
                "vrx_stop_verdicts: null argument, or n outside 1..2^24");
    if (int e = vrx_use_device("vrx_stop_verdicts", device)) return e;
    DevBuf<int32_t> d_i, d_v;
    DevBuf<double> d_d, d_p;
    VRX_HIP(d_i.upload(rows_i, (size_t)n * 4, 0));
    VRX_HIP(d_d.upload(rows_d, (size_t)n * 3, 0));
    VRX_HIP(d_v.alloc((size_t)n));
    VRX_HIP(d_p.alloc((size_t)n));
    vrx_stop_rows<<<(unsigned)((n + 255) / 256), 256, 0, 0>>>(n, d_i.p, d_d.p, d_v.p, d_p.p);
    VRX_HIP(hipGetLastError());
    VRX_HIP(hipMemcpy(verdict, d_v.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    VRX_HIP(hipMemcpy(prev, d_p.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    return VRX_OK;
}
