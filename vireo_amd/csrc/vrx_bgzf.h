// BGZF members inflated one per wavefront: the decoder behind the vrx_bgzf_* entries of include/vireo_hip.h.
//
// Plain C++ for host and device from one text: the host build (one lane) is what the sanitizer program of
// tests/san/ runs against zlib, the device build is the kernel of vrx_vcf.hip.  This header includes nothing of
// HIP and nothing of the library, so that a stand-alone program can include it alone.
//
// One wavefront decodes one member; a workgroup is that one wavefront (64 threads).  Every lane runs the same
// serial decode on the same values (bit reader, table walks, symbol loop), so the lanes never have to exchange
// state; lane 0 alone writes what the decode produces (code lengths, tables, literals), and the 64 lanes share
// the two jobs that are parallel: the match copy and the CRC.
//
// Where the output lives: in a 64 KiB window in LDS (a BGZF member holds at most 64 KiB of text), flushed to
// global memory once the member has passed its checks.  A match copy therefore reads bytes that other lanes
// stored a moment earlier from LDS, where a workgroup barrier (__syncthreads: s_waitcnt lgkmcnt(0) + s_barrier)
// is the documented ordering; no question of L1 visibility of the wave's own global stores arises.  The price
// is occupancy: VrxBgzfWork is 69 584 bytes (the window, three tables of 640 bytes, 320 code lengths, 1 792
// bytes of CRC tables), so a CU's 160 KiB of LDS hold 2 workgroups = 2 waves per CU, 512 members in flight on
// 256 CUs.
//
// Huffman lookup: the canonical count / first-code walk (count[len] codes of each length, symbols sorted by
// code).  A walk reads the 16 counts and one symbol from LDS; no primary table has to be filled per block.
//
// No input can make a loop here run away: every loop is bounded by a size of the member (payload bytes, ISIZE,
// the 320 code lengths, 15 code bits), and the block and symbol loops also count their iterations against
// payload bits + ISIZE + a constant, since each one consumes a bit or writes a byte.  Anything the decoder
// cannot vouch for is a status bit of the member; nothing traps, aborts or writes outside [0, ISIZE).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define VRX_BGZF_FN __host__ __device__ inline
#else
#define VRX_BGZF_FN inline
#endif

// ---- statuses ------------------------------------------------------------------------------------------------------
// of a member (bits, vrx_bgzf_inflate)
enum {
    VRX_BGZF_ST_EOF = 1,            // the deflate stream reads past the payload
    VRX_BGZF_ST_BTYPE = 2,          // block type 3
    VRX_BGZF_ST_STORED = 4,         // a stored block whose NLEN is not ~LEN
    VRX_BGZF_ST_LENGTHS = 8,        // HLIT > 286, HDIST > 30, a repeat with nothing to repeat or past the last length
    VRX_BGZF_ST_OVERSUBSCRIBED = 16,
    VRX_BGZF_ST_INCOMPLETE = 32,    // but for the distance code zlib accepts: none, or a single code of length 1
    VRX_BGZF_ST_NO_END = 64,        // no code for the end-of-block symbol
    VRX_BGZF_ST_SYMBOL = 128,       // bits that are no code of the table; literal/length 286, 287; distance 30, 31
    VRX_BGZF_ST_DISTANCE = 256,     // a match that starts before the member's first byte
    VRX_BGZF_ST_OVERFLOW = 512,     // a write at or beyond ISIZE
    VRX_BGZF_ST_SHORT = 1024,       // fewer bytes than ISIZE at the final block's end
    VRX_BGZF_ST_TRAILING = 2048,    // whole payload bytes left after the final block
    VRX_BGZF_ST_CRC = 4096,
    VRX_BGZF_ST_SPIN = 8192,        // the iteration cap (never reached by a loop that keeps its promise)
    VRX_BGZF_ST_ISIZE = 16384       // the footer's ISIZE is not the size the caller laid out (or exceeds 64 KiB)
};
// of a file (one value, vrx_bgzf_scan)
enum {
    VRX_BGZF_SCAN_OK = 0,
    VRX_BGZF_SCAN_HEADER = 1,     // a member that does not begin with the 18 bytes bgzip writes
    VRX_BGZF_SCAN_TRUNCATED = 2,  // a member that runs past the end of the file
    VRX_BGZF_SCAN_SIZE = 3        // BSIZE too small for header and footer, or ISIZE above 64 KiB
};

enum {
    VRX_BGZF_LANES = 64,
    VRX_BGZF_TEXT_MAX = 65536,   // bytes of text in one member
    VRX_BGZF_HEADER = 18,
    VRX_BGZF_FOOTER = 8,
    VRX_BGZF_CRC_CHUNK = 1024,   // VRX_BGZF_TEXT_MAX / VRX_BGZF_LANES: a lane's share of the CRC
    VRX_BGZF_CRC_LEVELS = 6      // log2(VRX_BGZF_LANES)
};

// ---- working memory of one member (LDS on the device) ------------------------------------------------------------
struct VrxBgzfTable {
    uint16_t count[16];    // codes of each length
    uint16_t offs[16];     // (table_build's cursor per length)
    uint16_t symbol[288];  // symbols in code order
};

struct VrxBgzfCrc {
    uint32_t table[256];                        // the byte table of the reflected polynomial 0xEDB88320
    uint32_t shift[VRX_BGZF_CRC_LEVELS][32];    // shift[j][b]: register bit b after VRX_BGZF_CRC_CHUNK << j zero bytes
};

struct alignas(16) VrxBgzfWork {
    uint8_t window[VRX_BGZF_TEXT_MAX];
    VrxBgzfTable lit, dist, clen;
    uint8_t lens[320];
    VrxBgzfCrc crc;
    uint32_t word;   // what lane 0 tells the others
    uint32_t pad[3];
};
static_assert(sizeof(VrxBgzfWork) == 69584 && 2 * sizeof(VrxBgzfWork) <= 160 * 1024, "two workgroups per CU");

// ---- lanes: the only device-specific text --------------------------------------------------------------------------
#if defined(__HIP_DEVICE_COMPILE__)
VRX_BGZF_FN uint32_t vrx_bgzf_lane() { return threadIdx.x; }
VRX_BGZF_FN void vrx_bgzf_sync() { __syncthreads(); }
#else
VRX_BGZF_FN uint32_t vrx_bgzf_lane() { return 0; }
VRX_BGZF_FN void vrx_bgzf_sync() {}
#endif

// ---- CRC32 ---------------------------------------------------------------------------------------------------------
// The register after message M from start value I is shift_|M|(I) xor raw(M), raw(M) the register from start 0.
// Lane l takes the chunk of VRX_BGZF_CRC_CHUNK bytes that ends (63 - l) chunks before the END of the text, so the
// lane that holds byte 0 starts from 0xFFFFFFFF, the lanes in front of it hold nothing and carry 0 (shifted or not,
// 0 stays 0), and level j of the tree joins neighbours with the fixed operator of CHUNK << j bytes.
VRX_BGZF_FN void vrx_bgzf_crc_init(VrxBgzfCrc& c) {
    for (uint32_t i = 0; i < 256; ++i) {
        uint32_t r = i;
        for (int k = 0; k < 8; ++k) r = (r >> 1) ^ (0xEDB88320u & (0u - (r & 1u)));
        c.table[i] = r;
    }
    for (uint32_t b = 0; b < 32; ++b) {
        uint32_t r = 1u << b;
        for (uint32_t k = 0; k < VRX_BGZF_CRC_CHUNK; ++k) r = c.table[r & 0xffu] ^ (r >> 8);
        c.shift[0][b] = r;
    }
    for (uint32_t j = 1; j < VRX_BGZF_CRC_LEVELS; ++j)   // twice the length: the operator applied to itself
        for (uint32_t b = 0; b < 32; ++b) {
            uint32_t x = c.shift[j - 1][b], y = 0;
            for (uint32_t k = 0; k < 32; ++k)
                if ((x >> k) & 1u) y ^= c.shift[j - 1][k];
            c.shift[j][b] = y;
        }
}

VRX_BGZF_FN uint32_t vrx_bgzf_crc_shift(const uint32_t* m, uint32_t x) {
    uint32_t y = 0;
    for (uint32_t k = 0; k < 32; ++k)
        if ((x >> k) & 1u) y ^= m[k];
    return y;
}

// the register of lane `lane` over its chunk of text[0, n)
VRX_BGZF_FN uint32_t vrx_bgzf_crc_lane(const VrxBgzfCrc& c, const uint8_t* text, uint32_t n, uint32_t lane) {
    const int32_t end = (int32_t)n - (int32_t)((VRX_BGZF_LANES - 1 - lane) * VRX_BGZF_CRC_CHUNK);
    if (end <= 0) return 0;
    int32_t beg = end - VRX_BGZF_CRC_CHUNK;
    uint32_t r = 0;
    if (beg <= 0) {
        beg = 0;
        r = 0xFFFFFFFFu;
    }
    for (int32_t i = beg; i < end; ++i) r = c.table[(r ^ text[i]) & 0xffu] ^ (r >> 8);
    return r;
}

// CRC32 (zlib's) of text[0, n), n <= VRX_BGZF_TEXT_MAX; every lane returns it
VRX_BGZF_FN uint32_t vrx_bgzf_crc(const VrxBgzfCrc& c, const uint8_t* text, uint32_t n) {
    if (n == 0) return 0;
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t lane = vrx_bgzf_lane();
    uint32_t r = vrx_bgzf_crc_lane(c, text, n, lane);
    for (uint32_t j = 0; j < VRX_BGZF_CRC_LEVELS; ++j) {
        const uint32_t s = 1u << j, mask = 2u * s - 1u;
        const uint32_t left = (uint32_t)__shfl((int)r, (int)((lane - s) & (VRX_BGZF_LANES - 1)), VRX_BGZF_LANES);
        if ((lane & mask) == mask) r = vrx_bgzf_crc_shift(c.shift[j], left) ^ r;
    }
    r = (uint32_t)__shfl((int)r, VRX_BGZF_LANES - 1, VRX_BGZF_LANES);
#else
    uint32_t reg[VRX_BGZF_LANES];
    for (uint32_t l = 0; l < VRX_BGZF_LANES; ++l) reg[l] = vrx_bgzf_crc_lane(c, text, n, l);
    for (uint32_t j = 0; j < VRX_BGZF_CRC_LEVELS; ++j) {
        const uint32_t s = 1u << j;
        for (uint32_t l = 2u * s - 1u; l < VRX_BGZF_LANES; l += 2u * s)
            reg[l] = vrx_bgzf_crc_shift(c.shift[j], reg[l - s]) ^ reg[l];
    }
    const uint32_t r = reg[VRX_BGZF_LANES - 1];
#endif
    return ~r;
}

// ---- bit reader ----------------------------------------------------------------------------------------------------
// Least-significant bit first.  Loads only in[0, n); bits past the payload read as zeros, and consuming one sets
// VRX_BGZF_ST_EOF.
struct VrxBgzfBits {
    const uint8_t* in;
    uint32_t n, pos;  // pos: bytes taken into buf (counts the zero bytes past n as well)
    uint32_t cnt;     // valid bits in buf
    uint64_t buf;
    uint32_t status;
};

VRX_BGZF_FN void vrx_bgzf_bits_open(VrxBgzfBits& b, const uint8_t* in, uint32_t n) {
    b.in = in;
    b.n = n;
    b.pos = 0;
    b.cnt = 0;
    b.buf = 0;
    b.status = 0;
}

// at least 32 valid bits
VRX_BGZF_FN void vrx_bgzf_bits_fill(VrxBgzfBits& b) {
    if (b.cnt > 32) return;
    uint32_t w = 0;
    if (b.pos + 4 <= b.n) {
        const uint8_t* p = b.in + b.pos;
        w = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
    } else {
        for (uint32_t k = 0; k < 4; ++k)
            if (b.pos + k < b.n) w |= (uint32_t)b.in[b.pos + k] << (8 * k);
    }
    b.buf |= (uint64_t)w << b.cnt;
    b.pos += 4;
    b.cnt += 32;
}

VRX_BGZF_FN uint32_t vrx_bgzf_bits_used(const VrxBgzfBits& b) { return b.pos * 8u - b.cnt; }

// the next k <= 16 bits, not consumed
VRX_BGZF_FN uint32_t vrx_bgzf_bits_peek(VrxBgzfBits& b, uint32_t k) {
    vrx_bgzf_bits_fill(b);
    return (uint32_t)b.buf & ((1u << k) - 1u);
}

// consumes k <= 32 bits that a fill has made valid
VRX_BGZF_FN void vrx_bgzf_bits_drop(VrxBgzfBits& b, uint32_t k) {
    b.buf >>= k;
    b.cnt -= k;
    if (vrx_bgzf_bits_used(b) > b.n * 8u) b.status |= VRX_BGZF_ST_EOF;
}

VRX_BGZF_FN uint32_t vrx_bgzf_bits_get(VrxBgzfBits& b, uint32_t k) {
    const uint32_t v = vrx_bgzf_bits_peek(b, k);
    vrx_bgzf_bits_drop(b, k);
    return v;
}

// ---- Huffman tables ------------------------------------------------------------------------------------------------
// One thread builds a table (lane 0 on the device).  lens[s] <= 15 for s < n <= 288.  lone_ok: the table may hold
// no code at all, or one code of length 1 (what zlib accepts of a distance code).
VRX_BGZF_FN uint32_t vrx_bgzf_table_build(VrxBgzfTable& t, const uint8_t* lens, uint32_t n, bool lone_ok) {
    for (uint32_t len = 0; len < 16; ++len) t.count[len] = 0;
    for (uint32_t s = 0; s < n; ++s) t.count[lens[s] & 15u] += 1;
    const uint32_t used = n - t.count[0];
    int32_t left = 1;
    for (uint32_t len = 1; len < 16; ++len) {
        left <<= 1;
        left -= (int32_t)t.count[len];
        if (left < 0) return VRX_BGZF_ST_OVERSUBSCRIBED;
    }
    if (left > 0 && !(lone_ok && (used == 0 || (used == 1 && t.count[1] == 1)))) return VRX_BGZF_ST_INCOMPLETE;
    t.offs[0] = 0;
    t.offs[1] = 0;
    for (uint32_t len = 1; len < 15; ++len) t.offs[len + 1] = (uint16_t)(t.offs[len] + t.count[len]);
    for (uint32_t s = 0; s < n; ++s) {
        const uint32_t len = lens[s] & 15u;
        if (len != 0) {
            t.symbol[t.offs[len]] = (uint16_t)s;   // offs[len] < used <= 288
            t.offs[len] += 1;
        }
    }
    return 0;
}

// the symbol of the next code (consumed), or -1 with nothing consumed if the next 15 bits begin no code
VRX_BGZF_FN int32_t vrx_bgzf_table_decode(VrxBgzfBits& b, const VrxBgzfTable& t) {
    uint32_t bits = vrx_bgzf_bits_peek(b, 15);
    uint32_t code = 0, first = 0, index = 0;
#if defined(__clang__)
#pragma unroll
#endif
    for (uint32_t len = 1; len <= 15; ++len) {
        code |= bits & 1u;
        bits >>= 1;
        const uint32_t c = t.count[len];
        if (code < first + c) {   // first <= code: a smaller code of this length would have ended the walk earlier
            vrx_bgzf_bits_drop(b, len);
            return (int32_t)t.symbol[index + (code - first)];
        }
        index += c;
        first = (first + c) << 1;
        code <<= 1;
    }
    return -1;
}

// lane 0's verdict on a table build, told to every lane (brackets the build with the two barriers it needs)
template <class Build>
VRX_BGZF_FN uint32_t vrx_bgzf_by_lane0(VrxBgzfWork& w, Build build) {
    vrx_bgzf_sync();   // the code lengths lane 0 stored are in place
    if (vrx_bgzf_lane() == 0) w.word = build();
    vrx_bgzf_sync();
    return w.word;
}

// ---- match copy: the one function with two forms -------------------------------------------------------------------
// out[pos, pos + len) from the bytes dist back; 1 <= dist <= pos, pos + len <= VRX_BGZF_TEXT_MAX (the caller checked)
VRX_BGZF_FN void vrx_bgzf_match(uint8_t* out, uint32_t pos, uint32_t len, uint32_t dist) {
#if defined(__HIP_DEVICE_COMPILE__)
    // Every source byte lies in front of pos, so no lane reads what this copy writes; the barrier makes the
    // literals and copies in front of pos, which other lanes stored, visible to this one.
    vrx_bgzf_sync();
    const uint32_t lane = vrx_bgzf_lane();
    for (uint32_t base = 0; base < len; base += VRX_BGZF_LANES) {
        const uint32_t i = base + lane;
        if (i < len) out[pos + i] = out[pos - dist + (dist >= len ? i : i % dist)];
    }
#else
    for (uint32_t i = 0; i < len; ++i) out[pos + i] = out[pos - dist + i];
#endif
}

// ---- one member ----------------------------------------------------------------------------------------------------
struct VrxBgzfRun {
    VrxBgzfBits bits;
    uint8_t* out;
    uint32_t isize, pos;   // pos: bytes written
    uint32_t iters, cap;
};

VRX_BGZF_FN bool vrx_bgzf_tick(VrxBgzfRun& r) {
    if (++r.iters > r.cap) r.bits.status |= VRX_BGZF_ST_SPIN;
    return r.bits.status == 0;
}

VRX_BGZF_FN void vrx_bgzf_stored(VrxBgzfRun& r) {
    VrxBgzfBits& b = r.bits;
    vrx_bgzf_bits_fill(b);
    vrx_bgzf_bits_drop(b, b.cnt & 7u);   // to the byte boundary
    const uint32_t len = vrx_bgzf_bits_get(b, 16), nlen = vrx_bgzf_bits_get(b, 16);
    if (b.status) return;
    if ((len ^ 0xffffu) != nlen) {
        b.status |= VRX_BGZF_ST_STORED;
        return;
    }
    if (len > r.isize - r.pos) {
        b.status |= VRX_BGZF_ST_OVERFLOW;
        return;
    }
    const bool writer = vrx_bgzf_lane() == 0;
    for (uint32_t i = 0; i < len && b.status == 0; ++i) {
        const uint32_t v = vrx_bgzf_bits_get(b, 8);
        if (writer && b.status == 0) r.out[r.pos + i] = (uint8_t)v;
    }
    if (b.status == 0) r.pos += len;
}

// the literal/length and distance tables of a dynamic block into w.lit and w.dist
VRX_BGZF_FN void vrx_bgzf_dynamic(VrxBgzfRun& r, VrxBgzfWork& w) {
    static const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    VrxBgzfBits& b = r.bits;
    const bool writer = vrx_bgzf_lane() == 0;
    const uint32_t nlen = vrx_bgzf_bits_get(b, 5) + 257, ndist = vrx_bgzf_bits_get(b, 5) + 1,
                   ncode = vrx_bgzf_bits_get(b, 4) + 4;
    if (b.status) return;
    if (nlen > 286 || ndist > 30) {
        b.status |= VRX_BGZF_ST_LENGTHS;
        return;
    }
    for (uint32_t i = 0; i < 19; ++i) {
        const uint32_t v = i < ncode ? vrx_bgzf_bits_get(b, 3) : 0;
        if (writer) w.lens[order[i]] = (uint8_t)v;
    }
    if (b.status) return;
    b.status |= vrx_bgzf_by_lane0(w, [&]() { return vrx_bgzf_table_build(w.clen, w.lens, 19, false); });
    const uint32_t total = nlen + ndist;
    uint32_t have = 0, prev = 0;
    while (have < total && vrx_bgzf_tick(r)) {
        const int32_t sym = vrx_bgzf_table_decode(b, w.clen);
        if (sym < 0) {
            b.status |= VRX_BGZF_ST_SYMBOL;
            break;
        }
        uint32_t rep = 1, val = (uint32_t)sym;
        if (sym == 16) {
            if (have == 0) {
                b.status |= VRX_BGZF_ST_LENGTHS;
                break;
            }
            rep = 3 + vrx_bgzf_bits_get(b, 2);
            val = prev;
        } else if (sym == 17) {
            rep = 3 + vrx_bgzf_bits_get(b, 3);
            val = 0;
        } else if (sym == 18) {
            rep = 11 + vrx_bgzf_bits_get(b, 7);
            val = 0;
        }
        if (have + rep > total) {   // (a repeat may run from the literal lengths into the distance lengths)
            b.status |= VRX_BGZF_ST_LENGTHS;
            break;
        }
        if (writer)
            for (uint32_t k = 0; k < rep; ++k) w.lens[have + k] = (uint8_t)val;
        have += rep;
        prev = val;
    }
    if (b.status) return;
    b.status |= vrx_bgzf_by_lane0(w, [&]() -> uint32_t {
        if (w.lens[256] == 0) return VRX_BGZF_ST_NO_END;
        return vrx_bgzf_table_build(w.lit, w.lens, nlen, false) | vrx_bgzf_table_build(w.dist, w.lens + nlen, ndist, true);
    });
}

VRX_BGZF_FN void vrx_bgzf_fixed(VrxBgzfRun& r, VrxBgzfWork& w) {
    r.bits.status |= vrx_bgzf_by_lane0(w, [&]() {
        for (uint32_t s = 0; s < 288; ++s) w.lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
        for (uint32_t s = 0; s < 32; ++s) w.lens[288 + s] = 5;
        return vrx_bgzf_table_build(w.lit, w.lens, 288, false) | vrx_bgzf_table_build(w.dist, w.lens + 288, 32, false);
    });
}

// the symbols of a block with the tables w.lit and w.dist, up to its end-of-block code
VRX_BGZF_FN void vrx_bgzf_symbols(VrxBgzfRun& r, const VrxBgzfWork& w) {
    VrxBgzfBits& b = r.bits;
    const bool writer = vrx_bgzf_lane() == 0;
    while (vrx_bgzf_tick(r)) {
        const int32_t sym = vrx_bgzf_table_decode(b, w.lit);
        if (b.status) return;
        if (sym < 0 || sym > 285) {
            b.status |= VRX_BGZF_ST_SYMBOL;
            return;
        }
        if (sym == 256) return;
        if (sym < 256) {
            if (r.pos >= r.isize) {
                b.status |= VRX_BGZF_ST_OVERFLOW;
                return;
            }
            if (writer) r.out[r.pos] = (uint8_t)sym;
            r.pos += 1;
            continue;
        }
        // lengths 3 ... 258: 257-264 one each, then four codes per extra bit, 285 is 258
        uint32_t len;
        if (sym < 265) {
            len = (uint32_t)sym - 254;
        } else if (sym == 285) {
            len = 258;
        } else {
            const uint32_t k = (uint32_t)sym - 261, e = k >> 2;
            len = ((4 + (k & 3u)) << e) + 3 + vrx_bgzf_bits_get(b, e);
        }
        const int32_t dsym = vrx_bgzf_table_decode(b, w.dist);
        if (b.status) return;
        if (dsym < 0 || dsym > 29) {
            b.status |= VRX_BGZF_ST_SYMBOL;
            return;
        }
        // distances 1 ... 32768: 0-3 one each, then two codes per extra bit
        uint32_t dist;
        if (dsym < 4) {
            dist = (uint32_t)dsym + 1;
        } else {
            const uint32_t e = ((uint32_t)dsym >> 1) - 1;
            dist = ((2 + ((uint32_t)dsym & 1u)) << e) + 1 + vrx_bgzf_bits_get(b, e);
        }
        if (b.status) return;
        if (dist > r.pos) {
            b.status |= VRX_BGZF_ST_DISTANCE;
            return;
        }
        if (len > r.isize - r.pos) {
            b.status |= VRX_BGZF_ST_OVERFLOW;
            return;
        }
        vrx_bgzf_match(r.out, r.pos, len, dist);
        r.pos += len;
    }
}

// Inflates the n payload bytes of one member into out[0, isize), isize <= VRX_BGZF_TEXT_MAX, and holds the result to
// the footer's crc.  Returns the member's status (0: out holds the text); every lane returns the same.  On the device
// out is w.window.
VRX_BGZF_FN uint32_t vrx_bgzf_member(VrxBgzfWork& w, const uint8_t* payload, uint32_t n, uint32_t isize, uint32_t crc,
                                     uint8_t* out) {
    if (isize > VRX_BGZF_TEXT_MAX) return VRX_BGZF_ST_ISIZE;
    VrxBgzfRun r;
    vrx_bgzf_bits_open(r.bits, payload, n);
    r.out = out;
    r.isize = isize;
    r.pos = 0;
    r.iters = 0;
    r.cap = n * 8u + isize + 16u;
    VrxBgzfBits& b = r.bits;
    uint32_t last = 0;
    while (!last && vrx_bgzf_tick(r)) {
        last = vrx_bgzf_bits_get(b, 1);
        const uint32_t type = vrx_bgzf_bits_get(b, 2);
        if (b.status) break;
        if (type == 0) {
            vrx_bgzf_stored(r);
        } else if (type == 3) {
            b.status |= VRX_BGZF_ST_BTYPE;
        } else {
            if (type == 1)
                vrx_bgzf_fixed(r, w);
            else
                vrx_bgzf_dynamic(r, w);
            if (b.status == 0) vrx_bgzf_symbols(r, w);
        }
        if (b.status) break;
    }
    vrx_bgzf_sync();   // every byte of the window is in place, whoever stored it
    if (b.status) return b.status;
    if (r.pos != isize) return VRX_BGZF_ST_SHORT;
    if ((vrx_bgzf_bits_used(b) + 7u) / 8u != n) return VRX_BGZF_ST_TRAILING;
    if (vrx_bgzf_crc(w.crc, out, isize) != crc) return VRX_BGZF_ST_CRC;
    return 0;
}

// ---- the members of a file image (host) ----------------------------------------------------------------------------
VRX_BGZF_FN uint32_t vrx_bgzf_le32(const uint8_t* p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// Walks file[0, n): every member begins with the 18 bytes bgzip / htslib write (1f 8b 08 04, XLEN 6, subfield BC of
// length 2) and the BSIZE chain ends exactly at n.  Members beyond `room` are counted, not stored.  payload_off[i],
// payload_len[i]: the deflate stream of member i; isize[i]: its footer's; out_off[i]: the sum of isize in front
// of it (out_off has room + 1 places: out_off[*n_members] is the total).  Returns VRX_BGZF_SCAN_*; *n_members then counts the whole
// members in front of the fault.  A missing end-of-file member is no fault.
inline int vrx_bgzf_scan_image(const uint8_t* file, int64_t n, int64_t room, int64_t* n_members, int64_t* payload_off,
                               int32_t* payload_len, int32_t* isize, int64_t* out_off) {
    int64_t at = 0, count = 0, text = 0;
    int rc = VRX_BGZF_SCAN_OK;
    while (at < n) {
        if (n - at < VRX_BGZF_HEADER) {
            rc = VRX_BGZF_SCAN_TRUNCATED;
            break;
        }
        const uint8_t* h = file + at;
        if (!(h[0] == 0x1f && h[1] == 0x8b && h[2] == 8 && h[3] == 4 && h[10] == 6 && h[11] == 0 && h[12] == 'B' &&
              h[13] == 'C' && h[14] == 2 && h[15] == 0)) {
            rc = VRX_BGZF_SCAN_HEADER;
            break;
        }
        const int64_t bsize = (int64_t)((uint32_t)h[16] | ((uint32_t)h[17] << 8)) + 1;
        if (bsize < VRX_BGZF_HEADER + VRX_BGZF_FOOTER) {
            rc = VRX_BGZF_SCAN_SIZE;
            break;
        }
        if (bsize > n - at) {
            rc = VRX_BGZF_SCAN_TRUNCATED;
            break;
        }
        const uint32_t size = vrx_bgzf_le32(h + bsize - 4);
        if (size > VRX_BGZF_TEXT_MAX) {
            rc = VRX_BGZF_SCAN_SIZE;
            break;
        }
        if (count < room) {
            payload_off[count] = at + VRX_BGZF_HEADER;
            payload_len[count] = (int32_t)(bsize - VRX_BGZF_HEADER - VRX_BGZF_FOOTER);
            isize[count] = (int32_t)size;
            out_off[count] = text;
        }
        text += size;
        count += 1;
        at += bsize;
    }
    if (out_off && count <= room) out_off[count] = text;
    *n_members = count;
    return rc;
}
