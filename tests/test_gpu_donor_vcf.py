"""load_donor_GPb on the GPU (vrx_vcf.h): the donor VCF read, matched to the cell variants and converted in one pass
over the text.  The yardstick is the host composition load_VCF -> match_SNPs -> parse_donor_GPb (force_host=True),
which is held to the real reference on the CPU: to its numbers on the well-formed fixtures in
tests/test_donor_vcf_cpu.py, and to its result or its exception's class on every file of a corpus of mutated text in
tests/test_vcf_mutation_cpu.py (the device meets the same corpus in tests/test_gpu_vcf_mutation.py).  Every comparison
is np.array_equal on indices and tobytes() on GPb -- there is no tolerance, every device value is a constant, a table
entry made by NumPy or a correctly rounded quotient."""
import functools
import gzip
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "donor_vcf")
DATA = os.path.join(ROOT, "tests", "golden", "data")
TAGS = ("GT", "PL", "GP")
HEAD = "##fileformat=VCFv4.2\n##source=test\n"


@pytest.fixture(scope="module")
def vcf():
    import __graft_entry__ as entry
    entry.build()
    import vireo_amd
    from vireo_amd import _lib
    _lib.require_gpu()
    return vireo_amd.vcf


def chunk():
    from vireo_amd import _lib
    return int(_lib.lib().vrx_vcf_chunk())


def code(rng, tag):
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


@functools.lru_cache(maxsize=None)
def pool(tag):
    """997 codes of a tag: the lines draw from them"""
    rng = np.random.default_rng(len(tag) + ord(tag[1]))
    return [code(rng, tag) for _ in range(997)]


def make_lines(n, S, seed, edges=True, chrom="1", first_pos=100):
    """-> (lines, ids): FORMAT GT:PL:GP (every fifth line lacks PL and GP, every seventh is multi-allelic); with
    ``edges`` the INFO field pads the line so that its length sits one byte below, at or above a multiple of the
    chunk the line walker reads, in turn"""
    rng = np.random.default_rng(seed)
    W = chunk()
    lines, ids = [], []
    for i in range(n):
        pos = str(first_pos + 13 * i)
        ref, alt = "ACGT"[rng.integers(4)], "ACGT"[rng.integers(4)]
        if i % 7 == 3:
            alt += ",C"
        fmt = ["GT"] if i % 5 == 4 else ["GT", "PL", "GP"]
        fields = [":".join(pool(t)[k] for t, k in zip(fmt, row)) for row in rng.integers(0, 997, (S, 3))]

        def line(info):
            return "\t".join([chrom, pos, ".", ref, alt, ".", "PASS", info, ":".join(fmt)] + fields)
        text = line(".")
        if edges and i % 4:
            want = (len(text) + W + 1) // W * W + (i % 3 - 1)             # 64 k - 1, 64 k, 64 k + 1
            text = line("I" * (want - len(text) + 1))
            assert len(text) == want
        lines.append(text)
        ids.append("_".join((chrom, pos, ref, alt)))
    return lines, ids


def write_vcf(path, samples, lines, last_newline=True, head=HEAD):
    text = head + "#" + "\t".join("CHROM POS ID REF ALT QUAL FILTER INFO FORMAT".split() + samples) + "\n"
    text += "\n".join(lines) + ("\n" if last_newline and lines else "")
    with gzip.open(path, "wb") as fh:
        fh.write(text.encode())
    return path


def cell_list(ids, seed, extra=5):
    rng = np.random.default_rng(seed)
    some = [x for k, x in enumerate(ids) if k % 2 == 0] + ["9_%d_A_C" % k for k in range(extra)]
    return [str(x) for x in rng.permutation(some)]


def same(a, b):
    assert a["samples"] == b["samples"]
    assert np.array_equal(a["keep"], b["keep"]) and np.array_equal(a["line"], b["line"])
    assert a["GPb"].shape == b["GPb"].shape and a["GPb"].tobytes() == b["GPb"].tobytes()
    assert (a["n_lines"], a["n_tagged"]) == (b["n_lines"], b["n_tagged"])


def both(vcf, path, tag, variants, **kw):
    with np.errstate(invalid="ignore", divide="ignore"):
        dev = vcf.load_donor_GPb(path, tag, variants, **kw)
        host = vcf.load_donor_GPb(path, tag, variants, force_host=True)
    same(dev, host)
    return dev, host


@pytest.mark.parametrize("name", ("plain", "chr"))
def test_fixtures_on_the_device(vcf, name):
    gold = np.load(os.path.join(GOLD, name + ".npz"))
    path = os.path.join(GOLD, name + ".vcf.gz")
    for tag in TAGS:
        for lname in ("inorder", "shuffled", "nomatch", "other_side"):
            dev, _ = both(vcf, path, tag, [str(x) for x in gold["list_" + lname]])
            assert dev["path"] == "device" and dev["reason"] is None and dev["n_repaired"] == 0
            want = {k: gold["%s_%s_%s" % (tag, lname, k)] for k in ("GPb", "keep", "samples", "n_lines", "n_tagged")}
            assert dev["GPb"].tobytes() == want["GPb"].tobytes() and np.array_equal(dev["keep"], want["keep"])
            assert dev["samples"] == list(want["samples"])
            assert (dev["n_lines"], dev["n_tagged"]) == (int(want["n_lines"]), int(want["n_tagged"]))
            assert set(dev["seconds"]) == {"inflate", "upload", "kernels", "download", "host"}


@pytest.mark.parametrize("S", (1, 2, 63, 64, 65, 130))
def test_sample_counts_line_lengths_and_line_counts(vcf, S, tmp_path):
    samples = ["s%d" % k for k in range(S)]
    n_checked = 0
    for n in (0, 1, 300):
        lines, ids = make_lines(n, S, seed=S * 1000 + n)
        if n == 300 and S <= 2:                     # short enough for the first boundary: 63, 64 and 65 bytes exactly
            assert {len(x) for x in lines} >= {chunk() - 1, chunk(), chunk() + 1}
        for last_newline in (True, False):
            path = write_vcf(str(tmp_path / ("s%d_n%d_%d.vcf.gz" % (S, n, last_newline))), samples, lines, last_newline)
            for tag in TAGS:
                dev, _ = both(vcf, path, tag, cell_list(ids, 3))
                assert dev["path"] == "device" and dev["n_repaired"] == 0
                assert dev["n_lines"] == sum(1 for x in lines if "," not in x.split("\t")[4])
                n_checked += len(dev["keep"])
    assert n_checked > 600


def test_slabs_do_not_change_a_bit(vcf, tmp_path):
    lines, ids = make_lines(300, 16, seed=4)
    long_lines, long_ids = make_lines(3, 1100, seed=5, chrom="2")      # each longer than the slab
    assert min(len(x) for x in long_lines) > 4096 > max(len(x) for x in lines)
    samples16, samples2k = ["s%d" % k for k in range(16)], ["s%d" % k for k in range(1100)]
    p16 = write_vcf(str(tmp_path / "a.vcf.gz"), samples16, lines)
    wide, wide_ids = make_lines(10, 1100, seed=6, edges=False)
    mixed = wide[:5] + long_lines + wide[5:]
    p2k = write_vcf(str(tmp_path / "b.vcf.gz"), samples2k, mixed, last_newline=False)
    for path, all_ids in ((p16, ids), (p2k, wide_ids + long_ids)):
        for tag in TAGS:
            cells = cell_list(all_ids, 8)
            with np.errstate(invalid="ignore"):
                one = vcf.load_donor_GPb(path, tag, cells)
                many = vcf.load_donor_GPb(path, tag, cells, slab_bytes=4096)
                tiny = vcf.load_donor_GPb(path, tag, cells, slab_bytes=1)     # every line a slab of its own
            assert one["path"] == many["path"] == tiny["path"] == "device"
            same(one, many)
            same(one, tiny)
            assert len(one["keep"]) >= 5
    both(vcf, p2k, "PL", cell_list(wide_ids + long_ids, 8), slab_bytes=4096)


def flagged_file(tmp_path, tag, extra):
    """300 regular lines with S = 5; `extra` maps a line number to a function of its fields -> the new fields"""
    lines, ids = make_lines(300, 5, seed=21, edges=False)
    for i, fn in extra.items():
        assert "," not in lines[i].split("\t")[4] and i % 5 != 4 and i % 2 == 0      # kept, tagged and matched
        lines[i] = "\t".join(fn(lines[i].split("\t")))
    return write_vcf(str(tmp_path / ("flagged_%s_%d.vcf.gz" % (tag, len(extra)))), ["s%d" % k for k in range(5)],
                     lines), ids


def cells_regular_first(ids):
    """parse_donor_GPb sizes its result by the first row in cell order: a regular one"""
    return [ids[0]] + [x for x in cell_list(ids, 9) if x != ids[0]]


def test_flagged_rows_are_repaired_on_the_host(vcf, tmp_path):
    def sub(f, k, text):                        # sample k's PL / GP subfields replaced
        parts = f[9 + k].split(":")
        return f[:9 + k] + [":".join([parts[0], text, text])] + f[10 + k:]
    other = dict(PL="5000,0,10", GP="1.,.5,0.25")
    kinds = {
        12: lambda f: sub(f, 2, other[tag]),                   # another code: above 4095 / not digits[.digits]
        20: lambda f: sub(f, 0, "1e1,0,3"),
        30: lambda f: sub(f, 4, "+7,0.5e0,3"),
        60: lambda f: f[:-1] + [f[-1] + "\r"],                  # what rstrip() removes: \r\n, blanks, a tab
        70: lambda f: f[:-1] + [f[-1] + "  "],
        82: lambda f: f + [""],
    }
    for tag in ("PL", "GP"):
        path, ids = flagged_file(tmp_path, tag, kinds)
        dev, host = both(vcf, path, tag, cells_regular_first(ids))
        assert dev["path"] == "device" and dev["n_repaired"] == len(kinds)
        assert not np.isnan(host["GPb"]).any()
    # GT: the codes float() takes are the device's too; the structural kinds remain
    path, ids = flagged_file(tmp_path, "GT", {k: kinds[k] for k in (60, 70, 82)})
    dev, _ = both(vcf, path, "GT", cells_regular_first(ids))
    assert dev["path"] == "device" and dev["n_repaired"] == 3
    # a row with fewer sample fields than the first row in cell order: the reference sizes its result by the first row
    # and indexes every row up to there (vcf_utils.py:328-331), so both paths raise IndexError as it does
    short = {40: lambda f: f[:9],                               # fewer than 10 fields
             50: lambda f: f[:-1]}                              # a sample-field count other than S
    for tag in TAGS:
        for k in short:
            path, ids = flagged_file(tmp_path, "%s_short%d" % (tag, k), {k: short[k]})
            for kw in (dict(), dict(force_host=True)):
                with pytest.raises(IndexError):
                    vcf.load_donor_GPb(path, tag, cells_regular_first(ids), **kw)


def test_a_short_first_row_and_dos_line_ends(vcf, tmp_path):
    """parse_donor_GPb sizes its result by the first row in cell order: when that row lacks a sample field the whole
    call is the host's, and the result has the first row's four donors -- the reference's loop never looks at the
    fifth code of the later rows (vcf_utils.py:328-331); a file with \\r\\n line ends has every matched row repaired
    and the same values"""
    path, ids = flagged_file(tmp_path, "GT", {12: lambda f: f[:-1]})
    cells = [ids[12]] + [x for x in cell_list(ids, 9) if x != ids[12]]
    regular, _ = flagged_file(tmp_path, "GT_regular", {})
    for tag in TAGS:
        dev, host = both(vcf, path, tag, cells)
        assert dev["path"] == "host" and "first row" in dev["reason"] and host["GPb"].shape[1] == 4
        with np.errstate(invalid="ignore", divide="ignore"):
            want = vcf.load_donor_GPb(regular, tag, cells, force_host=True)
        assert host["GPb"].tobytes() == want["GPb"][:, :4].tobytes() and np.array_equal(host["keep"], want["keep"])
    lines, ids = make_lines(60, 5, seed=60)                    # one sample name more than the rows have fields
    named6 = write_vcf(str(tmp_path / "named6.vcf.gz"), ["s%d" % k for k in range(6)], lines)
    dev, host = both(vcf, named6, "PL", cell_list(ids, 9))
    assert dev["path"] == "host" and "first row" in dev["reason"] and host["GPb"].shape[1] == 5
    lines, ids = make_lines(60, 5, seed=61)
    dos = write_vcf(str(tmp_path / "dos.vcf.gz"), ["s%d" % k for k in range(5)], [x + "\r" for x in lines],
                    head=HEAD.replace("\n", "\r\n"))
    for tag in TAGS:
        dev, _ = both(vcf, dos, tag, cell_list(ids, 62), slab_bytes=2000)
        assert dev["path"] == "device" and dev["n_repaired"] == len(dev["keep"]) > 20


@pytest.mark.parametrize("what,error", (("code", ValueError), ("subfield", IndexError), ("sum", IndexError)))
def test_both_paths_raise_the_same(vcf, tmp_path, what, error):
    def bad(f):
        if what == "code":
            return f[:9] + ["0/1:x,1,2:0.1,0.2,zz"] + f[10:]
        if what == "subfield":
            return f[:9] + ["0/1"] + f[10:]
        return f[:9] + ["2/1:x,1,2:0.1,0.2,zz"] + f[10:]
    for tag in (("GT",) if what == "sum" else ("PL", "GP")):
        path, ids = flagged_file(tmp_path, tag, {12: bad})
        for kw in (dict(), dict(force_host=True)):
            with pytest.raises(error):
                vcf.load_donor_GPb(path, tag, cells_regular_first(ids), **kw)


def test_sample_fields_beyond_the_first_rows_are_ignored(vcf, tmp_path):
    """a row with more sample fields than the first row in cell order: the reference's loop ends at the first row's
    count (vcf_utils.py:328-331), so it returns what the file without the extra fields gives, whatever their codes
    are (load_VCF still splits them: they have their subfields); both paths do"""
    for tag in TAGS:
        regular, ids = flagged_file(tmp_path, tag + "_regular", {})
        want, _ = both(vcf, regular, tag, cells_regular_first(ids))
        for name, more in (("one", lambda f: f + f[-1:]), ("junk", lambda f: f + ["x:y:z", ""])):
            path, ids = flagged_file(tmp_path, "%s_%s" % (tag, name), {12: more})
            dev, host = both(vcf, path, tag, cells_regular_first(ids))
            assert dev["path"] == "device" and dev["n_repaired"] == 1 and host["GPb"].shape[1] == 5
            same(dev, want)


def test_a_short_field_on_a_line_nobody_matches(vcf, tmp_path):
    """load_VCF splits every sample field of every kept line and indexes the tag's subfield (vcf_utils.py:60-65)
    before anything is matched: a field without it raises IndexError wherever the line stands, on both paths; a line
    the biallelic filter drops is never split"""
    lines, ids = make_lines(300, 5, seed=21, edges=False)
    cells = cells_regular_first(ids)

    def swap(i, field):
        f = lines[i].split("\t")
        assert len(f[8].split(":")) == 3 and ids[i] not in cells
        return write_vcf(str(tmp_path / ("short_%d_%d.vcf.gz" % (i, len(field)))), ["s%d" % k for k in range(5)],
                         lines[:i] + ["\t".join(f[:12] + [field] + f[13:])] + lines[i + 1:])
    for field, raises in (("0/1", ("PL", "GP")), ("0/1:1,2,3", ("GP",)), ("", ("PL", "GP"))):
        path = swap(13, field)                                  # kept, tagged, not in the cell list
        for tag in TAGS:
            if tag in raises:
                for kw in (dict(), dict(slab_bytes=1), dict(force_host=True)):
                    with pytest.raises(IndexError):
                        vcf.load_donor_GPb(path, tag, cells, **kw)
            else:
                dev, _ = both(vcf, path, tag, cells)
                assert dev["path"] == "device" and dev["n_repaired"] == 0
    path = swap(3, "0/1")                                       # multi-allelic: dropped before it is split
    for tag in TAGS:
        dev, _ = both(vcf, path, tag, cells)
        assert dev["path"] == "device" and dev["n_repaired"] == 0


def test_duplicates_take_the_host_path(vcf, tmp_path):
    lines, ids = make_lines(300, 3, seed=31)
    samples = ["a", "b", "c"]
    kept = [k for k in range(300) if k % 7 != 3]
    twice = write_vcf(str(tmp_path / "twice.vcf.gz"), samples, lines + [lines[kept[4]]])
    cells = [ids[k] for k in kept[:40]]
    dev, _ = both(vcf, twice, "GT", cells)
    assert dev["path"] == "host" and "repeats" in dev["reason"]
    unmatched_twice, _ = both(vcf, twice, "GT", [ids[k] for k in kept[10:40]])
    assert unmatched_twice["path"] == "device"                  # a repeated line nobody asks for changes nothing
    once = write_vcf(str(tmp_path / "once.vcf.gz"), samples, lines)
    dev, _ = both(vcf, once, "PL", cells + [cells[3]])
    assert dev["path"] == "host" and "equal ids" in dev["reason"]
    late = write_vcf(str(tmp_path / "late.vcf.gz"), samples, lines[:100] + ["##late comment"] + lines[100:])
    dev, _ = both(vcf, late, "GP", cells)
    assert dev["path"] == "host" and "'#' line" in dev["reason"]


def test_no_variants_is_the_whole_file(vcf, tmp_path):
    lines, ids = make_lines(300, 7, seed=41)
    path = write_vcf(str(tmp_path / "all.vcf.gz"), ["s%d" % k for k in range(7)], lines)
    for tag in TAGS:
        with np.errstate(invalid="ignore"):
            dev = vcf.load_donor_GPb(path, tag, None, slab_bytes=10000)
            v = vcf.load_VCF(path, biallelic_only=True, sparse=False, format_list=[tag])
            want = vcf.parse_donor_GPb(v["GenoINFO"][tag], tag)
        assert dev["path"] == "device" and dev["n_lines"] == len(v["variants"]) == len(dev["keep"])
        assert dev["GPb"].tobytes() == want.tobytes()
        assert np.array_equal(dev["keep"], np.arange(len(want))) and np.array_equal(dev["line"], dev["keep"])
        every = vcf.load_donor_GPb(path, tag, None, biallelic_only=False)
        assert every["n_lines"] == 300 and every["GPb"].shape == (300, 7, 3)


def test_a_row_depends_on_its_line_only(vcf, tmp_path):
    lines, ids = make_lines(120, 9, seed=51)
    others, _ = make_lines(200, 9, seed=52, chrom="7")
    rng = np.random.default_rng(53)
    samples = ["s%d" % k for k in range(9)]
    alone = write_vcf(str(tmp_path / "alone.vcf.gz"), samples, lines)
    order = rng.permutation(320)
    pool = lines + others
    among = write_vcf(str(tmp_path / "among.vcf.gz"), samples, [pool[k] for k in order])
    cells = cell_list(ids, 54)
    for tag in TAGS:
        with np.errstate(invalid="ignore"):
            a = vcf.load_donor_GPb(alone, tag, cells)
            b = vcf.load_donor_GPb(among, tag, cells, slab_bytes=3000)
        assert a["path"] == b["path"] == "device" and np.array_equal(a["keep"], b["keep"])
        assert a["GPb"].tobytes() == b["GPb"].tobytes() and not np.array_equal(a["line"], b["line"])


@pytest.mark.parametrize("tag", ("GT", "PL"))
def test_command_is_the_same_on_both_paths(vcf, tmp_path, tag):
    """python -m vireo_amd.vireo -c cellSNP_mat -d donors.cellSNP.vcf.gz -t TAG (no -N), once as it is and once
    under VIREO_DONOR_VCF=host: every output file byte for byte.  --randSeed fixes the initial assignment, without
    which two runs of one path differ; the module is run as __main__ through runpy, which is what -m does, so that
    the child can leave DONOR_LOAD of its module beside the outputs without printing a line."""
    prog = ("import json, runpy, sys\nside = sys.argv[1]\nsys.argv = ['vireo'] + sys.argv[2:]\n"
            "g = runpy.run_module('vireo_amd.vireo', run_name='__main__')\n"
            "json.dump({k: g['DONOR_LOAD'].get(k) for k in ('path', 'reason', 'n_repaired')}, open(side, 'w'))\n")
    outs, logs = {}, {}
    for how in ("device", "host"):
        out = str(tmp_path / how)
        env = dict(os.environ, PYTHONPATH=ROOT)
        env.pop("VIREO_DONOR_VCF", None)
        if how == "host":
            env["VIREO_DONOR_VCF"] = "host"
        p = subprocess.run([sys.executable, "-c", prog, out + ".json", "-c", DATA + "/cellSNP_mat", "-d",
                            DATA + "/donors.cellSNP.vcf.gz", "-t", tag, "-o", out, "--randSeed", "2", "--noPlot"],
                           env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert p.returncode == 0, p.stderr[-2000:]
        outs[how] = {name: open(os.path.join(out, name), "rb").read() for name in sorted(os.listdir(out))}
        logs[how] = (json.load(open(out + ".json")), [x for x in p.stdout.split("\n") if "All done" not in x])
    assert logs["device"][0]["path"] == "device" and logs["host"][0] == dict(path="host", reason="forced", n_repaired=0)
    assert logs["device"][1] == logs["host"][1]
    assert "_log.txt" in outs["device"] and sorted(outs["device"]) == sorted(outs["host"])
    for name in outs["device"]:
        assert outs["device"][name] == outs["host"][name], name
