"""What the BGZF tests share: a BGZF writer on zlib, a small deflate bit-writer for the streams zlib does not produce
on demand, the crafted cases (valid and invalid, each invalid one with the status bit it must raise), seeded
mutations, and the CRC scheme of csrc/vrx_bgzf.h restated in NumPy.  zlib is the judge of everything here
(tests/test_bgzf_cpu.py)."""
import gzip
import struct
import zlib

import numpy as np

EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
TEXT_MAX = 65536

# status bits of a member (csrc/vrx_bgzf.h)
ST = dict(EOF=1, BTYPE=2, STORED=4, LENGTHS=8, OVERSUBSCRIBED=16, INCOMPLETE=32, NO_END=64, SYMBOL=128, DISTANCE=256,
          OVERFLOW=512, SHORT=1024, TRAILING=2048, CRC=4096, SPIN=8192, ISIZE=16384)

# writer modes: name -> (level, strategy, full flush in mid-member)
MODES = {
    "stored": (0, zlib.Z_DEFAULT_STRATEGY, False),
    "fixed": (6, zlib.Z_FIXED, False),
    "rle": (6, zlib.Z_RLE, False),
    "huffman_only": (6, zlib.Z_HUFFMAN_ONLY, False),
    "level1": (1, zlib.Z_DEFAULT_STRATEGY, False),
    "level6": (6, zlib.Z_DEFAULT_STRATEGY, False),
    "level9": (9, zlib.Z_DEFAULT_STRATEGY, False),
    "full_flush": (6, zlib.Z_DEFAULT_STRATEGY, True),
}
MEMBER_TEXT_LENGTHS = (0, 1, 63, 64, 65, 65279, 65280)


# ---- the writer ------------------------------------------------------------------------------------------------------
def member(payload, text=None, crc=None, isize=None):
    """one BGZF member around a raw deflate stream; the footer is that of ``text`` unless given"""
    crc = zlib.crc32(text) if crc is None else crc
    isize = len(text) if isize is None else isize
    bsize = 18 + len(payload) + 8 - 1
    assert bsize < 65536, "a member holds at most 64 KiB"
    head = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", bsize)
    return head + payload + struct.pack("<II", crc & 0xffffffff, isize & 0xffffffff)


def deflate(text, mode="level6"):
    level, strategy, flush = MODES[mode]
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    if flush:
        half = len(text) // 2
        return c.compress(text[:half]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(text[half:]) + c.flush()
    return c.compress(text) + c.flush()


def bgzf(texts, mode="level6", eof=True):
    """a BGZF file with one member per text (and the empty end-of-file member)"""
    return b"".join(member(deflate(t, mode), t) for t in texts) + (EOF_MEMBER if eof else b"")


def vcf_like(n, seed):
    """n bytes that look like VCF lines: compressible, with long and short matches"""
    rng = np.random.RandomState(seed)
    out, size = [], 0
    while size < n:
        line = "chr%d\t%d\t.\t%s\t%s\t.\tPASS\tAD=%d;DP=%d;OTH=0\tGT:AD:DP\t%s\n" % (
            rng.randint(1, 23), rng.randint(1, 10 ** 8), "ACGT"[rng.randint(4)], "ACGT"[rng.randint(4)],
            rng.randint(50), rng.randint(100),
            "\t".join(rng.choice(["0/0:0:3", "1/0:1:2", ".:.:.", "1/1:4:4"], size=rng.randint(1, 40))))
        out.append(line.encode())
        size += len(out[-1])
    return b"".join(out)[:n]


def split_members(image):
    """the members of a well-formed BGZF image: (start, payload start, payload end, end) each"""
    at, out = 0, []
    while at < len(image):
        bsize = struct.unpack_from("<H", image, at + 16)[0] + 1
        out.append((at, at + 18, at + bsize - 8, at + bsize))
        at += bsize
    return out


# ---- the bit-writer --------------------------------------------------------------------------------------------------
class Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value, nbits):
        """a number, least-significant bit first"""
        self.acc |= (value & ((1 << nbits) - 1)) << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 0xff)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, nbits):
        """a Huffman code, most-significant bit first"""
        for k in range(nbits - 1, -1, -1):
            self.put((code >> k) & 1, 1)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def bytes(self):
        self.align()
        return bytes(self.out)


def canonical(lengths):
    """symbol -> (code, length) of the canonical code with these lengths (RFC 1951 3.2.2); valid or not"""
    count = [0] * 17
    for n in lengths:
        count[n] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for bits in range(1, 17):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    out = {}
    for sym, n in enumerate(lengths):
        if n:
            out[sym] = (nxt[n], n)
            nxt[n] += 1
    return out


def complete_lengths(symbols, size):
    """lengths of a complete code over ``symbols`` (two or more) in an alphabet of ``size``"""
    k = len(symbols)
    top = max(1, (k - 1).bit_length())
    short = (1 << top) - k
    lens = [0] * size
    for i, s in enumerate(symbols):
        lens[s] = top - 1 if i < short else top
    return lens


_CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
_CL_LENS = [4] * 13 + [5] * 6                     # a complete code over all 19 code-length symbols
_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
             227, 258]
_LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
_DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
              4097, 6145, 8193, 12289, 16385, 24577]
_DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in range(2)]


def length_symbol(n):
    s = max(i for i in range(29) if _LEN_BASE[i] <= n) if n < 258 else 28
    return 257 + s, n - _LEN_BASE[s], _LEN_EXTRA[s]


def dist_symbol(d):
    s = max(i for i in range(30) if _DIST_BASE[i] <= d)
    return s, d - _DIST_BASE[s], _DIST_EXTRA[s]


def _emit(b, ops, lit, dist):
    """ops: ints are literal/length symbols sent as they are (256 ends the block), ('m', length, distance) a match,
    ('d', symbol) a bare distance symbol"""
    for op in ops:
        if isinstance(op, int):
            b.code(*lit[op])
        elif op[0] == 'm':
            s, extra, nbits = length_symbol(op[1])
            b.code(*lit[s])
            b.put(extra, nbits)
            s, extra, nbits = dist_symbol(op[2])
            b.code(*dist[s])
            b.put(extra, nbits)
        else:
            b.code(*dist[op[1]])


def dynamic_block(b, lit_lens, dist_lens, ops, final=True, cl_seq=None, hlit=None):
    """a dynamic block with these code lengths; cl_seq: the code-length symbols as (symbol, extra value) pairs when the
    plain one-symbol-per-length form is not wanted; hlit: the HLIT field when it shall lie"""
    b.put(1 if final else 0, 1)
    b.put(2, 2)
    b.put(len(lit_lens) - 257 if hlit is None else hlit, 5)
    b.put(len(dist_lens) - 1, 5)
    b.put(19 - 4, 4)
    for s in _CL_ORDER:
        b.put(_CL_LENS[s], 3)
    cl = canonical(_CL_LENS)
    if cl_seq is None:
        cl_seq = [(n, 0) for n in list(lit_lens) + list(dist_lens)]
    for s, extra in cl_seq:
        b.code(*cl[s])
        if s >= 16:
            b.put(extra, {16: 2, 17: 3, 18: 7}[s])
    _emit(b, ops, canonical(lit_lens), canonical(dist_lens))


_FIXED_LIT = canonical([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
_FIXED_DIST = canonical([5] * 32)


def fixed_block(b, ops, final=True):
    b.put(1 if final else 0, 1)
    b.put(1, 2)
    _emit(b, ops, _FIXED_LIT, _FIXED_DIST)


def stored_block(b, data, final=True, nlen=None):
    b.put(1 if final else 0, 1)
    b.put(0, 2)
    b.align()
    b.put(len(data), 16)
    b.put(len(data) ^ 0xffff if nlen is None else nlen, 16)
    for x in data:
        b.put(x, 8)


# ---- the crafted cases -----------------------------------------------------------------------------------------------
def _lits(text):
    """the literal symbols of a text"""
    return list(text)


def crafted():
    """-> (valid, invalid): valid name -> (member, text); invalid name -> (member, status bit, deflate-level?)
    deflate-level: zlib.decompress(payload, -15) itself raises; otherwise only the footer or the framing is wrong and
    gzip is the one that raises."""
    valid, invalid = {}, {}

    def ok(name, b, text):
        valid[name] = (member(b.bytes(), text), text)

    def bad(name, b, bit, text=b"", deflate_level=True, **kw):
        invalid[name] = (member(b.bytes(), text, **kw), ST[bit], deflate_level)

    # a 15-bit code: lengths 1, 2, ..., 14, 15, 15 over fifteen letters and the end symbol; no distance code
    letters = b"abcdefghijklmno"
    lens = [0] * 257
    for i, ch in enumerate(letters):
        lens[ch] = i + 1
    lens[256] = 15
    text = letters * 3 + b"onmlk"
    b = Bits()
    dynamic_block(b, lens, [0], _lits(text) + [256])
    ok("code_of_15_bits", b, text)

    # no distance code at all, literals only (over a complete code of 4 symbols)
    text = b"abcabcaabbcc"
    b = Bits()
    dynamic_block(b, complete_lengths([97, 98, 99, 256], 257), [0], _lits(text) + [256])
    ok("no_distance_code", b, text)

    # a lone distance code of length 1
    ops = [97, 98, ('m', 5, 1), 97, 256]
    text = b"ab" + b"b" * 5 + b"a"
    b = Bits()
    dynamic_block(b, complete_lengths([97, 98, 256, length_symbol(5)[0]], 260), [1], ops)
    ok("lone_distance_code", b, text)

    # a repeat that runs from the literal lengths into the distance lengths: ... 2 (symbol 256), then code 16 x 4
    lit_lens = complete_lengths([97, 98, 256, 257], 258)          # four codes of length 2
    dist_lens = [2, 2, 2, 2]
    seq = [(18, 97 - 11), (2, 0), (2, 0), (18, 138 - 11), (18, 256 - 99 - 138 - 11), (2, 0), (2, 0), (16, 4 - 3)]
    assert 97 + 2 + 138 + (256 - 99 - 138) + 2 + 4 == 258 + 4
    ops = [97, 98, 97, ('m', 3, 2), ('m', 3, 4), 256]
    text = b"aba" + b"bab" + b"aba"
    b = Bits()
    dynamic_block(b, lit_lens, dist_lens, ops, cl_seq=seq)
    ok("repeat_across_the_boundary", b, text)

    # length 258 at distance 1
    ops = [120, ('m', 258, 1), 121, 256]
    text = b"x" * 259 + b"y"
    b = Bits()
    dynamic_block(b, complete_lengths([120, 121, 256, 285], 286), [1], ops)
    ok("length_258_distance_1", b, text)

    # distance 32 768: 32 768 literals over four letters, then a match back to the first byte
    rng = np.random.RandomState(5)
    head = bytes(rng.choice(list(b"ACGT"), size=32768).tolist())
    ops = _lits(head) + [('m', 7, 32768), 256]
    text = head + head[:7]
    b = Bits()
    dynamic_block(b, complete_lengths([65, 67, 71, 84, 256, length_symbol(7)[0]], 262),
                  complete_lengths([28, 29], 30), ops)
    ok("distance_32768", b, text)

    # a match that reaches back to the member's first byte, and one that reaches one byte before it
    for name, dist in (("match_to_first_byte", 3), ("match_before_first_byte", 4)):
        ops = [97, 98, 99, ('m', 4, dist), 256]
        b = Bits()
        dynamic_block(b, complete_lengths([97, 98, 99, 256, length_symbol(4)[0]], 259), complete_lengths([2, 3], 4), ops)
        if dist == 3:
            ok(name, b, b"abcabca")
        else:
            bad(name, b, "DISTANCE", text=b"abcabca")

    # several blocks of all three kinds in one member, an empty stored block among them
    b = Bits()
    stored_block(b, b"stored,", final=False)
    fixed_block(b, _lits(b"fixed,") + [('m', 6, 6), 256], final=False)
    stored_block(b, b"", final=False)
    dynamic_block(b, complete_lengths([100, 121, 110, 256], 257), [0], _lits(b"dyn") + [256])
    ok("three_kinds_of_block", b, b"stored,fixed,fixed,dyn")

    # ---- invalid streams
    b = Bits()                                                       # repeat code 16 as the first length
    dynamic_block(b, complete_lengths([97, 256], 257), [0], [97, 256], cl_seq=[(16, 0)] + [(0, 0)] * 257)
    bad("repeat_16_first", b, "LENGTHS")

    b = Bits()                                                       # a repeat past the last length
    dynamic_block(b, complete_lengths([97, 256], 257), [0], [97, 256],
                  cl_seq=[(18, 127)] + [(18, 127 - 19)] + [(18, 127)])
    bad("repeat_past_the_end", b, "LENGTHS")

    b = Bits()                                                       # HLIT says 288 literal/length codes
    dynamic_block(b, complete_lengths([97, 256], 257), [0], [97, 256], hlit=31)
    bad("hlit_288", b, "LENGTHS")

    b = Bits()                                                       # literal/length symbol 286 (fixed code)
    fixed_block(b, [97, 286, 256])
    bad("symbol_286", b, "SYMBOL", text=b"aa")

    b = Bits()                                                       # distance code 30 (fixed code)
    fixed_block(b, [97, 257, ('d', 30), 256])
    bad("distance_code_30", b, "SYMBOL", text=b"aaaa")

    lens = [0] * 257                                                 # over-subscribed: three codes of length 1
    lens[97] = lens[98] = lens[256] = 1
    b = Bits()
    dynamic_block(b, lens, [0], [97, 256])
    bad("oversubscribed", b, "OVERSUBSCRIBED")

    lens = [0] * 257                                                 # incomplete: three codes of length 2
    lens[97] = lens[98] = lens[256] = 2
    b = Bits()
    dynamic_block(b, lens, [0], [97, 256])
    bad("incomplete", b, "INCOMPLETE")

    b = Bits()                                                       # incomplete distance code of length 2
    dynamic_block(b, complete_lengths([97, 256, 257, 258], 259), [2], [97, ('m', 3, 1), 256])
    bad("incomplete_distance", b, "INCOMPLETE")

    lens = complete_lengths([97, 98], 257)                           # no end-of-block code
    b = Bits()
    dynamic_block(b, lens, [0], [97, 98])
    bad("no_end_of_block", b, "NO_END")

    b = Bits()                                                       # NLEN is not ~LEN
    stored_block(b, b"abc", nlen=0x1234)
    bad("nlen_wrong", b, "STORED")

    b = Bits()                                                       # block type 3
    b.put(1, 1)
    b.put(3, 2)
    bad("block_type_3", b, "BTYPE")

    text = vcf_like(3000, 11)
    good = deflate(text)
    invalid["payload_cut"] = (member(good[:-5], text), ST["EOF"], True)
    # the stream is sound, the footer or the framing is not
    invalid["one_byte_more_than_isize"] = (member(good, text[:-1]), ST["OVERFLOW"], False)
    invalid["one_byte_fewer_than_isize"] = (member(good, text + b"\n"), ST["SHORT"], False)
    invalid["wrong_crc"] = (member(good, text, crc=zlib.crc32(text) ^ 0x10), ST["CRC"], False)
    invalid["spare_byte"] = (member(good + b"\x00", text), ST["TRAILING"], False)
    return valid, invalid


# ---- mutations -------------------------------------------------------------------------------------------------------
def mutation_bases():
    """name -> member: small members of several kinds whose payloads are mutated"""
    valid, _ = crafted()
    out = {name: valid[name][0] for name in ("code_of_15_bits", "repeat_across_the_boundary", "lone_distance_code",
                                             "three_kinds_of_block", "length_258_distance_1")}
    for mode in ("fixed", "level6", "level9", "stored", "full_flush", "huffman_only"):
        t = vcf_like(700, 3)
        out["vcf_" + mode] = member(deflate(t, mode), t)
    return out


def mutate(image, offset, mask):
    """the member with one payload byte xor mask (offset counts from the payload's start, modulo its length)"""
    n = len(image) - 26
    out = bytearray(image)
    out[18 + offset % n] ^= mask
    return bytes(out)


def zlib_verdict(image):
    """what zlib makes of the member's payload as a whole raw stream: its text, or None when it raises, ends early,
    leaves bytes over or inflates to more than a member holds"""
    payload = image[18:-8]
    d = zlib.decompressobj(-15)
    try:
        text = d.decompress(payload, TEXT_MAX + 1)
    except zlib.error:
        return None
    if not d.eof or d.unused_data or d.unconsumed_tail or len(text) > TEXT_MAX:
        return None
    return text


def refoot(image, text):
    return image[:-8] + struct.pack("<II", zlib.crc32(text), len(text))


def seeded_mutations(n_per_base, seed=2024):
    """(base name, offset, mask): single bits and whole bytes, seeded"""
    rng = np.random.RandomState(seed)
    out = []
    for name in mutation_bases():
        for k in range(n_per_base):
            off = int(rng.randint(1 << 20))
            mask = 1 << int(rng.randint(8)) if k % 2 == 0 else int(rng.randint(1, 256))
            out.append((name, off, mask))
    return out


# The mutated payloads the device is shown (tests/test_gpu_bgzf.py), as (base, payload offset, xor mask): four per
# base, drawn once (seeded_mutations(4, seed=7)) and written down.  tests/test_bgzf_cpu.py runs exactly these through
# the sanitizer build of the same decoder first; zlib itself rejects 30 of the 44 payloads and accepts 14.
DEVICE_MUTATIONS = (
    ('code_of_15_bits', 585903, 16), ('code_of_15_bits', 573977, 247), ('code_of_15_bits', 759363, 8),
    ('code_of_15_bits', 328599, 104), ('repeat_across_the_boundary', 886108, 2), ('repeat_across_the_boundary', 712078, 24),
    ('repeat_across_the_boundary', 618056, 2), ('repeat_across_the_boundary', 127342, 43), ('lone_distance_code', 551642, 1),
    ('lone_distance_code', 543911, 231), ('lone_distance_code', 132164, 1), ('lone_distance_code', 120703, 136),
    ('three_kinds_of_block', 351148, 1), ('three_kinds_of_block', 78923, 56), ('three_kinds_of_block', 256250, 64),
    ('three_kinds_of_block', 728851, 189), ('length_258_distance_1', 27692, 128), ('length_258_distance_1', 943429, 57),
    ('length_258_distance_1', 230552, 128), ('length_258_distance_1', 1035189, 113), ('vcf_fixed', 889595, 32),
    ('vcf_fixed', 765888, 35), ('vcf_fixed', 336184, 2), ('vcf_fixed', 644558, 39), ('vcf_level6', 828164, 64),
    ('vcf_level6', 484489, 88), ('vcf_level6', 941539, 8), ('vcf_level6', 711752, 84), ('vcf_level9', 291760, 2),
    ('vcf_level9', 960192, 145), ('vcf_level9', 64886, 128), ('vcf_level9', 185693, 173), ('vcf_stored', 301660, 16),
    ('vcf_stored', 456263, 24), ('vcf_stored', 720394, 2), ('vcf_stored', 117539, 193), ('vcf_full_flush', 398653, 128),
    ('vcf_full_flush', 128151, 93), ('vcf_full_flush', 496375, 1), ('vcf_full_flush', 730773, 101), ('vcf_huffman_only', 885667, 2),
    ('vcf_huffman_only', 838211, 124), ('vcf_huffman_only', 742619, 2), ('vcf_huffman_only', 1004563, 156),
)


# ---- the CRC scheme of vrx_bgzf.h in NumPy ---------------------------------------------------------------------------
CRC_CHUNK, CRC_LANES = 1024, 64


def _crc_tables():
    table = np.zeros(256, np.uint32)
    for i in range(256):
        r = i
        for _ in range(8):
            r = (r >> 1) ^ (0xEDB88320 if r & 1 else 0)
        table[i] = r
    shift = np.zeros((6, 32), np.uint32)
    for b in range(32):
        r = 1 << b
        for _ in range(CRC_CHUNK):
            r = int(table[r & 0xff]) ^ (r >> 8)
        shift[0, b] = r
    for j in range(1, 6):
        for b in range(32):
            shift[j, b] = _apply(shift[j - 1], int(shift[j - 1, b]))
    return table, shift


def _apply(m, x):
    y = 0
    for k in range(32):
        if (x >> k) & 1:
            y ^= int(m[k])
    return y


_TABLES = None


def crc_by_lanes(text, chunk=CRC_CHUNK):
    """CRC32 of text (at most 64 chunks) by the scheme of vrx_bgzf_crc: end-aligned chunks, a fixed combine tree"""
    global _TABLES
    assert chunk == CRC_CHUNK and len(text) <= CRC_CHUNK * CRC_LANES
    if _TABLES is None:
        _TABLES = _crc_tables()
    table, shift = _TABLES
    n = len(text)
    if n == 0:
        return 0
    reg = [0] * CRC_LANES
    for lane in range(CRC_LANES):
        end = n - (CRC_LANES - 1 - lane) * chunk
        if end <= 0:
            continue
        beg = end - chunk
        r = 0
        if beg <= 0:
            beg, r = 0, 0xFFFFFFFF
        for x in text[beg:end]:
            r = int(table[(r ^ x) & 0xff]) ^ (r >> 8)
        reg[lane] = r
    for j in range(6):
        s = 1 << j
        for lane in range(2 * s - 1, CRC_LANES, 2 * s):
            reg[lane] = _apply(shift[j], reg[lane - s]) ^ reg[lane]
    return reg[-1] ^ 0xFFFFFFFF


def gzip_raises(image):
    try:
        gzip.decompress(image)
    except (gzip.BadGzipFile, zlib.error, EOFError):
        return True
    return False
