"""read_cellVCF on the GPU (vrx_cellvcf.h): cellSNP's cells.vcf.gz -> sparse AD / DP in one pass over the text.  The
yardstick is the host composition load_VCF -> read_sparse_GeneINFO (force_host=True) and the reference's own arrays in
tests/golden/c1_cell_vcf.npz.  The host path is held to the real reference on the CPU: to its numbers on the well-formed
files in tests/test_cell_vcf_cpu.py, and to its result or its exception's class on every file of a corpus of mutated
text in tests/test_vcf_mutation_cpu.py (the device meets the same corpus in tests/test_gpu_vcf_mutation.py).  Every
comparison is np.array_equal on indptr / indices / data with their dtypes and == on the lists -- there is no tolerance,
every device value is an integer below 10^9."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import cellvcf_util as U

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rd():
    import __graft_entry__ as entry
    entry.build()
    import vireo_amd
    from vireo_amd import _lib
    _lib.require_gpu()
    return vireo_amd.read_cellVCF


def segment():
    from vireo_amd import _lib
    return int(_lib.lib().vrx_cellvcf_segment())


def chunk():
    from vireo_amd import _lib
    return int(_lib.lib().vrx_vcf_chunk())


def outcome(fn):
    try:
        return "ok", fn()
    except (Exception, SystemExit) as e:                              # noqa: BLE001  (the host path may exit)
        return "raise", type(e), str(e)


def both(rd, path, biallelic_only=True, **kw):
    """the device path and the host path on one file: the same result, or the same exception"""
    dev = outcome(lambda: rd(path, biallelic_only=biallelic_only, **kw))
    host = outcome(lambda: rd(path, biallelic_only=biallelic_only, force_host=True))
    assert dev[0] == host[0], (dev, host)
    if dev[0] == "raise":
        assert dev[1:] == host[1:]
        return dev
    U.same(dev[1], host[1])
    return dev[1]


def region(line):
    """the sample region of a line as the device cuts it: from the ninth tab to the end"""
    return "\t" + line.split("\t", 9)[9]


def offsets(line):
    """(tab offset behind the ninth tab, field) of every sample field"""
    out, at = [], 0
    for f in line.split("\t")[9:]:
        out.append((at, f))
        at += len(f) + 1
    return out


def test_demo_file_equals_the_reference(rd):
    dev = rd(U.DEMO)
    assert dev["path"] == "device" and dev["reason"] is None and dev["n_repaired"] == 0
    U.check_golden(dev, "demo__1")
    assert dev["AD"].nnz == 73046 and int((dev["AD"].data == 0).sum()) == 40602


@pytest.mark.parametrize("biallelic_only", (True, False))
@pytest.mark.parametrize("name", U.SMALL)
def test_crafted_files_equal_the_reference(rd, name, biallelic_only):
    dev = rd(U.small_path(name), biallelic_only=biallelic_only)
    U.check_golden(dev, "%s__%d" % (name, biallelic_only))
    if name == "permuted":
        assert dev["path"] == "host" and "FORMAT" in dev["reason"]
    else:
        assert dev["path"] == "device" and (dev["n_repaired"] > 0) == (name == "odd")


@pytest.mark.parametrize("S", (1, 2, 63, 64, 65, 130, 1000))
def test_sample_counts(rd, S, tmp_path):
    rng = np.random.default_rng(S)
    n_entries = 0
    for last in (True, False):
        lines = [U.make_line(i, U.random_fields(rng, S, 0.3), alt="C,T" if i % 7 == 3 else "C") for i in range(40)]
        lines.append(U.make_line(40, [U.entry(1, 2)] * S))                         # every cell an entry
        lines.append(U.make_line(41, ["."] * S))                                   # none
        path = U.write_vcf(tmp_path / ("s%d_%d.vcf.gz" % (S, last)), S, lines, last=last)
        for bi in (True, False):
            dev = both(rd, path, biallelic_only=bi)
            assert dev["path"] == "device" and dev["n_repaired"] == 0 and dev["n_lines"] == (36 if bi else 42)
            assert dev["AD"].shape == (dev["n_lines"], S)
            n_entries += dev["AD"].nnz
    assert n_entries >= 4 * S


def craft(S, length, entries):
    """S sample fields, entries in the cells `entries`, whose region is `length` bytes: '.' turned into the long
    missing form ten bytes at a time, the rest as leading zeros of the entries' values"""
    fields = ["."] * S
    for j in entries:
        fields[j] = U.entry(3, 5)
    need = length - sum(len(f) + 1 for f in fields)
    assert need >= 0
    free = [j for j in range(S) if j not in entries]
    for j in free[:need // 10]:
        fields[j] = U.BLANK
    rest = need % 10
    fields[entries[0]] = U.entry("0" * min(rest, 8) + "3", "0" * (rest - min(rest, 8)) + "5")
    assert sum(len(f) + 1 for f in fields) == length
    return fields


def test_lines_around_the_segment_length(rd, tmp_path):
    seg = segment()
    for mult in (1, 2):
        S = (mult * seg - 80) // 2
        lines, want = [], []
        for i, d in enumerate((-2, -1, 0, 1, 2)):
            for entries in ([0, S - 1], [S // 2], [0], [S - 1]):                 # an entry first and last in the line
                lines.append(U.make_line(len(lines), craft(S, mult * seg + d, entries)))
                want.append(entries)
        assert {len(region(x)) - mult * seg for x in lines} == {-2, -1, 0, 1, 2}
        path = U.write_vcf(tmp_path / ("seg%d.vcf.gz" % mult), S, lines)
        dev = both(rd, path)
        assert dev["path"] == "device" and dev["n_repaired"] == 0
        for r, entries in enumerate(want):
            assert dev["AD"][r].indices.tolist() == entries and dev["DP"][r].data.tolist() == [5.0] * len(entries)


def place(S, t, what, target):
    """S sample fields; the tab (what = 'tab') or the first byte ('byte') of field `target` lies t bytes behind the
    ninth tab; the first field is an entry, the fields between are '.'"""
    tab = t if what == "tab" else t - 1
    first = U.entry(3, 5)
    if (tab - len(first) - 1) % 2:
        first = U.entry("03", 5)
    j = 1 + (tab - len(first) - 1) // 2
    assert 1 <= j < S
    return [first] + ["."] * (j - 1) + [target] + ["."] * (S - j - 1), j


def test_fields_on_chunk_and_segment_boundaries(rd, tmp_path):
    seg, W = segment(), chunk()
    S = seg + 60
    more = U.BLANK + ":."                                               # one dot more than the missing form: an entry
    lines, want = [], []
    for t in (W - 1, W, seg - 1, seg, 2 * seg - 1, 2 * seg):
        for what in ("tab", "byte"):
            for target in (U.entry("0,7", 21), U.BLANK, more, "."):
                fields, j = place(S, t, what, target)
                line = U.make_line(len(lines), fields)
                assert offsets(line)[j] == ((t if what == "tab" else t - 1), target)
                lines.append(line)
                want.append([0] + ([j] if target not in (U.BLANK, ".") else []))
    # the long missing form and the entry one dot longer across the end of a segment, byte by byte
    for k in range(1, len(more) + 1):
        for target in (U.BLANK, more):
            fields, j = place(S, seg - k, "tab", target)
            lines.append(U.make_line(len(lines), fields))
            want.append([0] + ([j] if target == more else []))
    path = U.write_vcf(tmp_path / "edges.vcf.gz", S, lines)
    dev = both(rd, path)
    assert dev["path"] == "device" and dev["n_repaired"] == 0
    for r, cells in enumerate(want):
        assert dev["AD"][r].indices.tolist() == cells, r
    same_small = rd(path, slab_bytes=3 * seg)
    U.same(dev, same_small)


def test_missing_forms(rd, tmp_path):
    more, fewer = U.BLANK + ":.", U.BLANK[:-2]
    lines = [U.make_line(0, [".", U.BLANK, more, U.entry(4, 9)]), U.make_line(1, [more, ".", U.BLANK, "."]),
             U.make_line(2, [U.BLANK, U.BLANK, ".", more])]
    dev = both(rd, U.write_vcf(tmp_path / "forms.vcf.gz", 4, lines))
    assert dev["path"] == "device" and dev["n_repaired"] == 0
    assert dev["AD"].indices.tolist() == [2, 3, 0, 3] and dev["AD"].data.tolist() == [0.0, 4.0, 0.0, 0.0]
    assert dev["DP"].data.tolist() == [0.0, 9.0, 0.0, 0.0] and dev["n_SNP_tagged"].tolist() == [4] * 6
    two = [U.make_line(i, f, fmt="AD:DP") for i, f in enumerate(([".", ".:.", "3:5", ".:.:."], ["0,2:7:9", ".", ".:.", "."]))]
    dev = both(rd, U.write_vcf(tmp_path / "two.vcf.gz", 4, two))
    assert dev["path"] == "device" and dev["AD"].indices.tolist() == [2, 3, 0] and dev["AD"].data.tolist() == [3.0, 0.0, 2.0]
    for k, bad in enumerate((fewer, "1/0:3:5", "")):                    # fewer subfields than FORMAT has names
        short = lines[:2] + [U.make_line(2, [".", bad, U.BLANK, "."])] + lines[2:]
        got = both(rd, U.write_vcf(tmp_path / ("short%d.vcf.gz" % k), 4, short))
        assert got[0] == "raise" and got[1] is IndexError


def test_value_forms(rd, tmp_path):
    lines = [U.make_line(0, [U.entry(".", 17), ".", U.entry("0,3,45", "1,2,48"), U.entry("123456789", "999999999")]),
             U.make_line(1, [U.BLANK, U.entry("007", "0012"), ".", U.entry(".", ".")])]
    dev = both(rd, U.write_vcf(tmp_path / "values.vcf.gz", 4, lines))
    assert dev["path"] == "device" and dev["n_repaired"] == 0
    assert dev["AD"].data.tolist() == [0.0, 45.0, 123456789.0, 7.0, 0.0]
    assert dev["DP"].data.tolist() == [17.0, 48.0, 999999999.0, 12.0, 0.0]
    odd = lines + [U.make_line(2 + k, [".", U.entry(*v), U.BLANK, U.entry(1, 2)])
                   for k, v in enumerate((("1234567890", 3), (3, "+5"), ("1e3", 2000), (" 7", 8), ("1.0", 4), ("0,-0", 1)))]
    dev = both(rd, U.write_vcf(tmp_path / "odd.vcf.gz", 4, odd))
    assert dev["path"] == "device" and dev["n_repaired"] == 6
    assert dev["AD"].data.tolist()[5:] == [1234567890.0, 1.0, 3.0, 1.0, 1000.0, 1.0, 7.0, 1.0, 1.0, 1.0, -0.0, 1.0]
    long_field = lines + [U.make_line(2, [".", "1/0:3:5:0:" + ",".join(["1"] * 700) + ":0", ".", U.entry(1, 2)])]
    dev = both(rd, U.write_vcf(tmp_path / "long.vcf.gz", 4, long_field))
    assert dev["path"] == "device" and dev["n_repaired"] == 1 and dev["AD"].data.tolist()[5:] == [3.0, 1.0]
    for k, v in enumerate((("abc", 3), ("3,", 3), (3, ""), ("1 2", 3))):
        bad = odd + [U.make_line(20, [".", ".", U.entry(*v), "."])]
        got = both(rd, U.write_vcf(tmp_path / ("bad%d.vcf.gz" % k), 4, bad))
        assert got[0] == "raise" and got[1] is ValueError


def test_line_structure(rd, tmp_path):
    rng = np.random.default_rng(7)
    S = 9
    lines = [U.make_line(i, U.random_fields(rng, S, 0.3), ref="AT" if i % 5 == 2 else "G", alt="C,T" if i % 7 == 3 else "C")
             for i in range(60)]
    tails = ["", " ", "  ", "\t", " \t ", "\x1c\x0b"]
    blank = U.write_vcf(tmp_path / "blank.vcf.gz", S, [x + tails[i % 6] for i, x in enumerate(lines)])
    dos = U.write_vcf(tmp_path / "dos.vcf.gz", S, lines, eol="\r\n")
    open_end = U.write_vcf(tmp_path / "open.vcf.gz", S, lines, last=False)
    dos_open = U.write_vcf(tmp_path / "dos_open.vcf.gz", S, lines, eol="\r\n", last=False)
    plain = both(rd, U.write_vcf(tmp_path / "plain.vcf.gz", S, lines))
    for path in (blank, dos, open_end, dos_open):
        for bi in (True, False):
            dev = both(rd, path, biallelic_only=bi, slab_bytes=2000)
            assert dev["path"] == "device" and dev["n_repaired"] == 0
            assert dev["n_lines"] == (sum(1 for i in range(60) if i % 5 != 2 and i % 7 != 3) if bi else 60)
        U.same(both(rd, path), plain)


def test_slab_cuts_do_not_change_a_bit(rd, tmp_path):
    rng = np.random.default_rng(8)
    S = 130
    lines = [U.make_line(i, U.random_fields(rng, S, 0.2), alt="C,T" if i % 6 == 0 else "C") for i in range(80)]
    lines[10] = U.make_line(10, [U.entry("1e2", 400)] + U.random_fields(rng, S - 1, 0.2))       # a flagged line
    lines[11] = U.make_line(11, U.random_fields(rng, S - 1, 0.2) + [U.entry(3, "+9")])
    path = U.write_vcf(tmp_path / "slabs.vcf.gz", S, lines, last=False)
    one = both(rd, path)
    assert one["path"] == "device" and one["n_repaired"] == 2 and one["n_lines"] == 66     # (the first line is dropped)
    for slab_bytes in (1, 1000, 5000):
        cut = rd(path, slab_bytes=slab_bytes)
        assert cut["path"] == "device" and cut["n_repaired"] == 2
        U.same(one, cut)


def test_a_row_depends_on_its_line_only(rd, tmp_path):
    rng = np.random.default_rng(9)
    S = 70
    mine = [U.make_line(i, U.random_fields(rng, S, 0.25)) for i in range(50)]
    others = [U.make_line(1000 + i, U.random_fields(rng, S, 0.5), alt="G" if i % 4 else "G,A") for i in range(90)]
    pool = mine + others
    alone = rd(U.write_vcf(tmp_path / "alone.vcf.gz", S, mine))
    among = rd(U.write_vcf(tmp_path / "among.vcf.gz", S, [pool[k] for k in rng.permutation(140)]), slab_bytes=3000)
    assert alone["path"] == among["path"] == "device"
    where = {v: r for r, v in enumerate(among["variants"])}
    assert [where[v] for v in alone["variants"]] != list(range(50))
    for r, v in enumerate(alone["variants"]):
        for key in ("AD", "DP"):
            a, b = alone[key][r], among[key][where[v]]
            assert np.array_equal(a.indices, b.indices) and np.array_equal(a.data, b.data)


def test_files_for_the_host_path(rd, tmp_path):
    rng = np.random.default_rng(10)
    S = 12
    lines = [U.make_line(i, U.random_fields(rng, S, 0.3)) for i in range(30)]

    def swap(i, **kw):
        f = lines[i].split("\t")
        return lines[:i] + [U.make_line(i, kw.pop("fields", f[9:]), **kw)] + lines[i + 1:]

    def permuted(field):
        p = field.split(":")
        return field if len(p) != 6 else ":".join([p[1], p[0], p[5], p[2], p[4], p[3]])
    cases = {
        "permuted": (swap(7, fmt="AD:GT:ALL:DP:PL:OTH", fields=[permuted(x) for x in lines[7].split("\t")[9:]]), "FORMAT"),
        "other_set": (swap(7, fmt="GT:AD:DP:OTH:PL:XX"), "FORMAT"),
        "shorter_format": (swap(7, fmt="GT:AD:DP"), "FORMAT"),
        "one_more": (swap(9, fields=lines[9].split("\t")[9:] + ["."]), "sample-field count"),
        "one_more_entry": (swap(9, fields=lines[9].split("\t")[9:] + [U.entry(1, 2)]), "sample-field count"),
        "one_fewer": (swap(9, fields=lines[9].split("\t")[9:-1]), "sample-field count"),
        "first_fewer": (swap(0, fields=lines[0].split("\t")[9:-1]), "sample-field count"),
        "no_samples": (swap(9, fields=[]), "sample-field count"),
        "comment": (lines[:5] + ["##late"] + lines[5:], "'#' line"),
        "non_ascii": (swap(3, info="X=\xc3\xa9"), "non-ASCII"),
        "lone_cr": (swap(3, info="X=1\rY=2"), "carriage return"),
        "eight_fields": (lines[:4] + ["\t".join(lines[4].split("\t")[:8])] + lines[5:], "fewer than 9"),
        "empty_line": (lines[:4] + [""] + lines[4:], "fewer than 9"),
        "no_lines": ([], "no kept lines"),
        "none_kept": ([U.make_line(i, ["."] * S, alt="C,G") for i in range(3)], "no kept lines"),
    }
    seen = set()
    for name, (text, reason) in cases.items():
        path = U.write_vcf(tmp_path / (name + ".vcf.gz"), S, text)
        got = both(rd, path)
        if isinstance(got, tuple):
            seen.add((name, got[1].__name__))
        else:
            assert got["path"] == "host" and reason in got["reason"], (name, got["reason"])
    assert ("other_set", "SystemExit") in seen and ("no_lines", "TypeError") in seen and ("none_kept", "TypeError") in seen
    assert not {n for n, _ in seen} & {"permuted", "one_more", "one_fewer", "comment", "non_ascii"}
    dev = rd(U.write_vcf(tmp_path / "kept_all.vcf.gz", S, cases["none_kept"][0]), biallelic_only=False)
    assert dev["path"] == "device" and dev["AD"].nnz == 0 and dev["AD"].shape == (3, S)


def test_too_few_tags_prints_the_reference_line(rd, tmp_path, capsys):
    S = 5
    lines = [U.make_line(i, ["."] * S) for i in range(30)] + [U.make_line(30, [".", U.entry(2, 3), ".", ".", "."])]
    path = U.write_vcf(tmp_path / "few.vcf.gz", S, lines)
    dev = rd(path)
    out_dev = capsys.readouterr().out
    host = rd(path, force_host=True)
    assert out_dev == capsys.readouterr().out and out_dev.startswith("[vireo] Warning: too few variants with tags! GT: 1\t")
    assert dev["path"] == "device"
    U.same(dev, host)


def test_command_is_the_same_on_both_paths(rd, tmp_path):
    """python -m vireo_amd.vireo -c cells.cellSNP.vcf.gz -N 4, once as it is and once under VIREO_CELL_VCF=host: every
    output file byte for byte.  --randSeed fixes the restarts; the module is run as __main__ through runpy so that
    the child can leave CELL_LOAD of its module beside the outputs without printing a line."""
    prog = ("import json, runpy, sys\nside = sys.argv[1]\nsys.argv = ['vireo'] + sys.argv[2:]\n"
            "g = runpy.run_module('vireo_amd.vireo', run_name='__main__')\n"
            "json.dump({k: g['CELL_LOAD'].get(k) for k in ('path', 'reason', 'n_repaired', 'n_lines')}, open(side, 'w'))\n")
    outs, logs = {}, {}
    for how in ("device", "host"):
        out = str(tmp_path / how)
        env = dict(os.environ, PYTHONPATH=ROOT)
        env.pop("VIREO_CELL_VCF", None)
        if how == "host":
            env["VIREO_CELL_VCF"] = "host"
        p = subprocess.run([sys.executable, "-c", prog, out + ".json", "-c", U.DEMO, "-N", "4", "-o", out,
                            "--randSeed", "2", "--noPlot"], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert p.returncode == 0, p.stderr[-2000:]
        outs[how] = {name: open(os.path.join(out, name), "rb").read() for name in sorted(os.listdir(out))}
        logs[how] = (json.load(open(out + ".json")), [x for x in p.stdout.split("\n") if "All done" not in x])
    assert logs["device"][0] == dict(path="device", reason=None, n_repaired=0, n_lines=3784)
    assert logs["host"][0] == dict(path="host", reason="forced", n_repaired=0, n_lines=3784)
    assert logs["device"][1] == logs["host"][1]
    assert "donor_ids.tsv" in outs["device"] and sorted(outs["device"]) == sorted(outs["host"])
    for name in outs["device"]:
        assert outs["device"][name] == outs["host"][name], name
