"""A seeded corpus of mutated VCF text, shared by tests/golden/make_vcf_mutation_golden.py (what the real reference
does with every file), tests/test_vcf_mutation_cpu.py (the host path against that record) and
tests/test_gpu_vcf_mutation.py (the device path against the host path).  Pure Python and NumPy: a file is a function
of (kind, index) alone, its text is made in memory and written under a directory of the caller's at run time.

Base files.  Donor layout: FORMAT GT:PL:GP, every fifth line GT only, every seventh multi-allelic, S in DONOR_S, 12 to
40 lines, with the cell-variant list of every other id plus five absent ones, permuted.  Cell layout: cellSNP's
GT:AD:DP:OTH:PL:ALL with both missing forms, S in CELL_S -- the last one about 1100 mostly-missing fields, so that the
sample region crosses one SEGMENT boundary.  Every other base file pads INFO so that line lengths sit one byte below,
at and one byte above a multiple of CHUNK.

Mutations.  One to three per file (cell files mostly one or two: any change to FORMAT makes the reference exit), each
recorded as (operator, line, region, token).  Byte operators insert, delete or replace a byte, or replace a whole
field or a whole ':'-subfield, with a token of tokens(kind) (two in five a digit; outside the field-only files one in
four a control or non-UTF-8 byte); structural operators change the line structure.  A file is
*field-only* when every mutation lies inside a sample field of a kept, tagged, matched line and uses printable ASCII;
half of every corpus is field-only by construction, every S among them.

The grammar the device accepts (vrx_vcf.h, vrx_cellvcf.h) is restated in donor_repairs / cell_repairs, which say for
a field-only file how many of its lines the device has to hand to the host."""
import gzip
import hashlib
import os

import numpy as np

CHUNK, SEGMENT = 64, 2048          # vrx_vcf_chunk(), vrx_cellvcf_segment(): the CPU test holds them to the library
SEED = 20240611
N_FILES, GROUP = 200, 25
DONOR_S, CELL_S = (1, 2, 5, 65), (1, 3, 70, 1100)
TAGS = ("GT", "PL", "GP")
COLS = "CHROM POS ID REF ALT QUAL FILTER INFO FORMAT".split()
HEAD = ["##fileformat=VCFv4.2", "##contig=<ID=1>", "##source=test"]
CELL_FORMAT = "GT:AD:DP:OTH:PL:ALL"
BLANK = {"donor": ".:.:.", "cell": ".:.:.:.:.:."}
STR_SPACE = " \t\n\r\x0b\x0c\x1c\x1d\x1e\x1f"                     # what str.rstrip() removes, ASCII

_COMMON = ([bytes([c]) for c in b"0123456789"] + [bytes([c]) for c in b".,:/|+-eE_x"] + [b" ", b"\t", b""]
           + [b"\r", b"\n", b"\x0b", b"\x1c", b"\x85", b"\xff"]                    # \xff: never valid in UTF-8
           + [b"00", b"4095", b"4096", b"1e1", b"inf", b"nan"]
           + [b"1.23456789012345", b"1.234567890123456"]                           # 15 and 16 significant digits
           + [b"0." + b"0" * 21 + b"7", b"0." + b"0" * 22 + b"7"]                  # 22 and 23 fractional digits
           + [b"123456789", b"1234567890", b".:.", b"./.", b".|.", b"::", b",,", b"\t\t"])


CONTROL = [b"\r", b"\n", b"\x0b", b"\x1c", b"\x85", b"\xff", b"\t", b"\r"]


def tokens(kind):
    """the fixed token set: the common ones, then one dot more and one dot fewer than the kind's blank form"""
    blank = BLANK[kind].encode()
    return _COMMON + [blank + b":.", blank[:-2]]


def printable(token):
    return all(0x20 <= c <= 0x7e for c in token)


class File:
    """one corpus file: name, kind, S, samples, head (bytes lines), lines (bytes), final_newline, mutations, field_only
    and, for a donor file, cells (the cell-variant list); base_ids are the ids of the unmutated lines"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def text(self):
        body = b"\n".join(self.head + self.lines)
        return body + (b"\n" if self.final_newline else b"")

    @property
    def sha256(self):
        return hashlib.sha256(self.text).hexdigest()

    def write(self, directory):
        path = os.path.join(str(directory), self.name + ".vcf.gz")
        with gzip.GzipFile(path, "wb", compresslevel=1, mtime=0) as fh:
            fh.write(self.text)
        return path


# ---- base files -----------------------------------------------------------------------------------------------------
def _donor_code(rng, tag):
    if rng.integers(8) == 0:
        return [".", "./.", ".|."][rng.integers(3)]
    if tag == "GT":
        return ["0/0", "0/1", "1/0", "1/1", "0|1", "1|1", "0", "1", "0/0/1", "1|0|1"][rng.integers(10)]
    if tag == "PL":
        v = [int(x) for x in rng.integers(0, 4096, 3)]
        if rng.integers(3) == 0:
            v[rng.integers(3)] = min(v)
        return ",".join(str(x) for x in v)
    out = []
    for _ in range(3):
        n = int(rng.integers(1, 16))
        digits = "".join(str(x) for x in rng.integers(0, 10, n))
        cut = int(rng.integers(0, n))
        out.append(str(int(digits)) if cut == 0 else (digits[:n - cut].lstrip("0") or "0") + "." + digits[n - cut:])
    return ",".join(out)


def _cell_entry(rng):
    a = int(rng.integers(0, 30))
    ad = [str(a), "0,%d" % a, "3,0,%d" % a, "."][(0, 0, 0, 0, 1, 1, 2, 3)[rng.integers(8)]]
    dp = str(a + int(rng.integers(0, 40))) if rng.integers(10) else "."
    return "%s:%s:%s:%d:%d,%d,%d:%d,%d,%d,%d,%d" % ((["0/0", "1/0", "1/1"][rng.integers(3)], ad, dp, rng.integers(3))
                                                    + tuple(rng.integers(0, 300, 3)) + tuple(rng.integers(0, 9, 5)))


def _pad(fields_of, i, edges):
    """the line with INFO '.', or padded so that its length is 64 k - 1, 64 k or 64 k + 1 in turn"""
    text = fields_of(".")
    if edges and i % 4:
        want = (len(text) + CHUNK + 1) // CHUNK * CHUNK + (i % 3 - 1)
        text = fields_of("I" * (want - len(text) + 1))
        assert len(text) == want
    return text


def _base(kind, rng, S, n, edges):
    """-> (lines, ids, eligible): eligible[i] says that line i is kept by the biallelic filter and, in a donor file,
    names all three tags"""
    lines, ids, eligible = [], [], []
    rate, blank = {1: (0.6, 0.8), 3: (0.5, 0.8), 70: (0.25, 0.6)}.get(S, (0.012, 0.04))
    for i in range(n):
        ref, alt = "ACGT"[rng.integers(4)], "ACGT"[rng.integers(4)]
        if kind == "donor":
            pos = str(100 + 13 * i)
            if i % 7 == 3:
                alt += ",C"
            fmt = "GT" if i % 5 == 4 else "GT:PL:GP"
            fields = [":".join(_donor_code(rng, t) for t in fmt.split(":")) for _ in range(S)]
            eligible.append(i % 7 != 3 and i % 5 != 4)
        else:
            pos = str(100 + 7 * i)
            if i % 9 == 4:
                alt += ",T"
            if i % 13 == 6:
                ref += "T"
            fmt = CELL_FORMAT
            u = rng.random(S)
            fields = [_cell_entry(rng) if x < rate else (BLANK["cell"] if x < blank else ".") for x in u]
            eligible.append(i % 9 != 4 and i % 13 != 6)
        lines.append(_pad(lambda info: "\t".join(["1", pos, ".", ref, alt, ".", "PASS", info, fmt] + fields), i, edges))
        ids.append("_".join(("1", pos, ref, alt)))
    return lines, ids, eligible


def cell_list(ids, rng, extra=5):
    some = [x for k, x in enumerate(ids) if k % 2 == 0] + ["9_%d_A_C" % k for k in range(extra)]
    return [str(x) for x in rng.permutation(some)]


# ---- mutations ------------------------------------------------------------------------------------------------------
def _sample_fields(line):
    """[(start, end)] of the sample fields of a line: what lies behind its ninth tab, cut at the tabs"""
    tabs = [k for k, c in enumerate(line) if c == 9]
    if len(tabs) < 9:
        return []
    cuts = tabs[8:] + [len(line)]
    return [(cuts[k] + 1, cuts[k + 1]) for k in range(len(cuts) - 1)]


def _near_boundary(rng, line, spans):
    """a sample field and a byte in it within two bytes of a chunk or segment boundary of the sample region, which the
    device walks from the ninth tab: (field index, byte position)"""
    start = spans[0][0] - 1
    length = len(line) - start
    if length > SEGMENT and rng.integers(2):
        at = SEGMENT
    else:
        at = CHUNK * int(rng.integers(1, max(2, length // CHUNK + 1)))
    at = min(max(start + at + int(rng.integers(-2, 3)), spans[0][0]), len(line) - 1)
    for k, (a, b) in enumerate(spans):
        if a <= at <= b:                                            # on the tab behind the field: its last byte
            return k, min(at, max(a, b - 1))
    return len(spans) - 1, spans[-1][0]


def _byte_edit(rng, line, a, b, token, op, at=None):
    """one byte operator inside line[a:b]; -> the new line"""
    line = bytearray(line)
    if op in ("delete", "replace") and b == a:
        op = "insert"
    if op == "insert":
        p = int(rng.integers(a, b + 1)) if at is None else at
        line[p:p] = token
    elif op == "delete":
        p = int(rng.integers(a, b)) if at is None else at
        del line[p]
    elif op == "replace":
        p = int(rng.integers(a, b)) if at is None else at
        line[p:p + 1] = token
    elif op == "field":
        line[a:b] = token
    else:                                                           # a whole ':'-subfield
        parts = bytes(line[a:b]).split(b":")
        parts[int(rng.integers(len(parts)))] = token
        line[a:b] = b":".join(parts)
    return bytes(line)


BYTE_OPS = ("insert", "delete", "replace", "field", "subfield")
STRUCT_OPS = ("no_final_newline", "trailing_blanks", "duplicate_line", "late_comment", "delete_chrom",
              "permute_format", "truncate")


def _structural(rng, f, op):
    i = int(rng.integers(len(f.lines)))
    if op == "no_final_newline":
        f.final_newline, i = False, -1
    elif op == "trailing_blanks":
        f.lines[i] += [b" ", b"  ", b"\t", b" \t ", b"\r", b"\x1c\x0b"][rng.integers(6)]
    elif op == "duplicate_line":
        f.lines.insert(int(rng.integers(len(f.lines) + 1)), f.lines[i])
    elif op == "late_comment":
        i = int(rng.integers(1, len(f.lines) + 1))
        f.lines.insert(i, b"##late comment")
    elif op == "delete_chrom":
        f.head, i = [x for x in f.head if not x.startswith(b"#CHROM")], -1
    elif op == "permute_format":
        cols = f.lines[i].split(b"\t")
        if len(cols) > 8:
            names = cols[8].split(b":")
            order = rng.permutation(len(names))
            cols[8] = b":".join(names[k] for k in order)
            if rng.integers(2):                                     # the entries follow their names
                for k in range(9, len(cols)):
                    parts = cols[k].split(b":")
                    if len(parts) == len(names):
                        cols[k] = b":".join(parts[j] for j in order)
            f.lines[i] = b"\t".join(cols)
    else:
        f.lines[i] = b"\t".join(f.lines[i].split(b"\t")[:int(rng.integers(7, 10))])
    return (op, i, "structure", "")


def _mutate(rng, f, eligible, field_only):
    toks = tokens(f.kind)
    if field_only:
        toks = [t for t in toks if printable(t)]
        i = int(rng.choice(eligible))
    elif rng.integers(5) == 0:
        return _structural(rng, f, STRUCT_OPS[rng.integers(len(STRUCT_OPS))])
    else:
        i = int(rng.integers(len(f.lines)))
    line = f.lines[i]
    op = BYTE_OPS[(0, 0, 1, 1, 2, 2, 2, 3, 4, 4)[rng.integers(10)]]            # a whole field least often
    token = toks[rng.integers(10 if rng.integers(5) < 2 else len(toks))]       # two in five a digit: the first ten
    if not field_only and rng.integers(4) == 0:                    # one in four a control or a non-UTF-8 byte
        token = CONTROL[rng.integers(len(CONTROL))]
    spans = _sample_fields(line)
    if not spans or (not field_only and rng.integers(3) == 0):     # the fixed columns, FORMAT among them
        tabs = [k for k, c in enumerate(line) if c == 9][:9]
        cuts = [-1] + tabs + ([len(line)] if len(tabs) < 9 else [])
        k = int(rng.integers(len(cuts) - 1))
        a, b = (cuts[k] + 1, cuts[k + 1]) if op in ("field", "subfield") else (0, cuts[-1])
        f.lines[i] = _byte_edit(rng, line, a, b, token, op)
        return (op, i, "fixed", token.decode("latin-1"))
    at = None
    if f.S > 1000 and rng.integers(3) == 0:                           # the wide base: on the edges the device walks by
        k, at = _near_boundary(rng, line, spans)
    elif f.kind == "cell" and rng.integers(6):                    # an entry where the line has one: most fields are blank
        entries = [k for k, (a, b) in enumerate(spans) if b - a > len(BLANK["cell"])]
        k = int(rng.choice(entries)) if entries else int(rng.integers(len(spans)))
    else:
        k = int(rng.integers(len(spans)))
    a, b = spans[k]
    if not field_only and rng.integers(3) == 0 and op in ("insert", "delete", "replace"):
        a, b, at = spans[0][0] - 1, len(line), None                 # anywhere behind FORMAT, the tabs included
    if at is not None and op == "delete" and b == a:
        at = None
    f.lines[i] = _byte_edit(rng, line, a, b, token, op, at)
    return (op, i, "sample", token.decode("latin-1"))


def make_file(kind, index):
    """file `index` of the corpus of `kind` ('donor' | 'cell'): a function of the two alone"""
    rng = np.random.default_rng([SEED, 0 if kind == "donor" else 1, index])
    sizes = DONOR_S if kind == "donor" else CELL_S
    S = sizes[index % len(sizes)]
    n = int(rng.integers(12, 41))
    lines, ids, ok = _base(kind, rng, S, n, edges=(index // 8) % 2 == 0)
    samples = ["s%d" % k for k in range(S)]
    f = File(name="%s%03d" % (kind, index), kind=kind, S=S, samples=samples, base_ids=ids, final_newline=True,
             head=[x.encode() for x in HEAD + ["#" + "\t".join(COLS + samples)]], lines=[x.encode() for x in lines],
             field_only=(index // 4) % 2 == 0, mutations=[])
    if kind == "donor":
        f.cells = cell_list(ids, rng)
        eligible = [i for i in range(n) if ok[i] and i % 2 == 0]
        count = (1, 1, 1, 2, 2, 3)[rng.integers(6)]
    else:
        eligible = [i for i in range(n) if ok[i]]
        count = (1, 1, 1, 1, 1, 1, 2, 2, 2, 3)[rng.integers(10)]
    for _ in range(count):
        f.mutations.append(_mutate(rng, f, eligible, f.field_only))
    f.eligible = eligible
    return f


_made = {}


def corpus(kind):
    if kind not in _made:
        _made[kind] = [make_file(kind, k) for k in range(N_FILES)]
    return _made[kind]


def groups():
    return [range(g, min(g + GROUP, N_FILES)) for g in range(0, N_FILES, GROUP)]


# ---- the device's grammar, restated ----------------------------------------------------------------------------------
def _digits(text, most=None):
    return text.isascii() and text.isdigit() and (most is None or len(text) <= most)


def _donor_code_ok(code, tag):
    if code in (".", "./.", ".|."):
        return True
    if tag == "GT":
        return len(code) >= 1 and _digits(code[0] + code[-1]) and int(code[0]) + int(code[-1]) <= 2
    parts = code.split(",")
    if len(parts) != 3:
        return False
    if tag == "PL":
        return all(_digits(p, 9) and int(p) <= 4095 for p in parts)
    for p in parts:                                                 # digits[.digits], 15 significant, 22 fractional
        whole, dot, frac = p.partition(".")
        if not _digits(whole) or (dot and not _digits(frac)) or len(frac) > 22 or int(whole + frac) >= 10 ** 15:
            return False
    return True


def donor_repairs(f, tag):
    """how many matched lines of a field-only donor file the device flags for the host under `tag`: rstrip() removed
    something, a sample-field count other than S, a missing subfield or a code outside the grammar"""
    assert f.field_only and f.kind == "donor"
    wanted, count = set(f.cells), 0
    for i in f.eligible:
        raw = f.lines[i].decode("ascii")
        cols = raw.rstrip(STR_SPACE).split("\t")
        assert "_".join((cols[0], cols[1], cols[3], cols[4])) in wanted
        k = cols[8].split(":").index(tag)
        fields = [x.split(":") for x in cols[9:]]
        bad = len(cols[9:]) != f.S or any(len(x) <= k or not _donor_code_ok(x[k], tag) for x in fields)
        count += bad or raw != raw.rstrip(STR_SPACE)
    return count


def cell_repairs(f):
    """how many kept lines of a field-only cell file the device flags for the host: an entry whose AD or DP text
    after the last comma is neither '.' nor 1-9 digits.  None: an entry with fewer subfields than FORMAT has names,
    which sends the whole file to the host (where it raises)"""
    assert f.field_only and f.kind == "cell"
    count = 0
    for i in f.eligible:
        bad = False
        for field in f.lines[i].decode("ascii").rstrip(STR_SPACE).split("\t")[9:]:
            if field in (".", BLANK["cell"]):
                continue
            parts = field.split(":")
            if len(parts) < 6:
                return None
            for text in (parts[1].split(",")[-1], parts[2].split(",")[-1]):
                bad |= not (text == "." or _digits(text, 9))
        count += bad
    return count


# ---- records ---------------------------------------------------------------------------------------------------------
def outcome(fn):
    """('ok', result) or ('raise', class name, message): SystemExit is what the reference's exit() raises"""
    try:
        return ("ok", fn())
    except (Exception, SystemExit) as e:                            # noqa: BLE001
        return ("raise", type(e).__name__, str(e))


def _sha(parts):
    h = hashlib.sha256()
    for p in parts:
        if isinstance(p, np.ndarray):
            p = str(p.dtype).encode() + b"|" + np.ascontiguousarray(p).tobytes()
        elif not isinstance(p, bytes):
            p = repr(p).encode()
        h.update(b"%d:" % len(p) + p)
    return h.hexdigest()


def donor_digest(keep, line, GPb, samples, n_lines, n_tagged):
    """one SHA-256 over keep, the matched lines, GPb's shape and bytes, the samples and the two line counts"""
    return _sha([np.asarray(keep, dtype=np.int64), np.asarray(line, dtype=np.int64), tuple(int(x) for x in GPb.shape),
                 np.asarray(GPb, dtype=np.float64), [str(x) for x in samples], int(n_lines), int(n_tagged)])


def cell_digest(AD, DP, variants, samples, n_SNP_tagged):
    """one SHA-256 over the shape, indptr / indices / data of AD and DP with their dtypes, the variant ids, the samples
    and n_SNP_tagged"""
    parts = [tuple(int(x) for x in AD.shape)]
    for m in (AD, DP):
        parts += [m.indptr, m.indices, m.data]
    return _sha(parts + [[str(x) for x in variants], [str(x) for x in samples], np.asarray(n_SNP_tagged)])
