"""Progress-ordered issue priority of the LDS passes, read in the ISA (no GPU: hipcc cross-compiles gfx950).

A wave of `vrx_spmm_lds` sets its priority once at the head of every round of a slab visit -- min(3, NR - 1 - r)
for round r of NR (VRX_WAVE_PRIO in vrx_kernels.h) -- and goes back to the round-0 value before the next visit's
first slab barrier.  Nothing else may change: the `-DVRX_WAVE_PRIO=0` build is the same kernel line for line once
the `s_setprio` statements are taken out, with the same registers, so the results cannot differ.
"""
import functools
import os
import re
import subprocess
import tempfile

import pytest

from tests.device_isa import CSRC, HIPCC, ROOT, compile_unit
from tests.test_kernel_build_cpu import _instances


def _map(nr):
    """the immediates of a visit in program order: the reset in front of the first slab barrier, then the rounds"""
    rounds = [min(3, nr - 1 - r) for r in range(nr)]
    return [rounds[0]] + rounds


@functools.lru_cache(maxsize=None)
def _compile_without():
    """vrx_engine.hip with the flags of tests/device_isa.compile_unit and -DVRX_WAVE_PRIO=0"""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    with tempfile.TemporaryDirectory(prefix="isa_") as d:
        asm = os.path.join(d, "unit.s")
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                            "--cuda-device-only", "-S", "-o", asm, "vrx_engine.hip", "-DVRX_WAVE_PRIO=0",
                            "-Rpass-analysis=kernel-resource-usage"], cwd=CSRC, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
        return open(asm).read(), r.stderr


def _kernels(isa):
    """{kernel: (resource report block, body lines)} of every kernel of the unit"""
    asm, report = isa
    out = {}
    for block in re.split(r"remark: [^\n]*Function Name: ", report)[1:]:
        name = block.split()[0]
        body = asm[asm.index("\n" + name + ":"):]
        out[name] = (block, body[:body.index("s_endpgm")].split("\n"))
    return out


def _prio(body):
    return [int(l.split()[1]) for l in body if re.match(r"\s*s_setprio\b", l)]


def _without_prio(body):
    """the body with every `s_setprio` statement (the instruction and its inline-assembly markers) taken out"""
    out, i = [], 0
    while i < len(body):
        if (i + 2 < len(body) and body[i].strip() == ";;#ASMSTART" and re.match(r"\s*s_setprio\b", body[i + 1])
                and body[i + 2].strip() == ";;#ASMEND"):
            i += 3
            continue
        out.append(body[i])
        i += 1
    return out


@pytest.fixture(scope="module")
def default():
    return compile_unit("vrx_engine.hip")


@pytest.fixture(scope="module")
def without():
    return _compile_without()


def test_every_instance_steps_its_priority_down_round_by_round(default):
    inst = _instances(default[1])
    kernels = _kernels(default)
    assert len(inst) == 24 and {v["rw"] for v in inst.values()} == {32, 64, 96}, sorted(inst)
    for name, v in inst.items():
        nr = v["rw"] // (64 // v["lpe"])
        body = kernels[name][1]
        # one per round and the reset, in round order: none of them sits in a trip loop, none is duplicated
        assert _prio(body) == _map(nr), (name, _prio(body))
        # the reset comes before the visit's first barrier, round 0's behind the second one
        bars = [i for i, l in enumerate(body) if re.match(r"\s*s_barrier", l)]
        at = [i for i, l in enumerate(body) if re.match(r"\s*s_setprio\b", l)]
        assert len(bars) == 2 and at[0] < bars[0] < bars[1] < at[1], (name, bars, at)
    assert _map(6) == [3, 3, 3, 3, 2, 1, 0] and _map(4) == [3, 3, 2, 1, 0] and _map(2) == [1, 1, 0]


def test_no_other_kernel_sets_a_priority(default):
    inst = _instances(default[1])
    for name, (_, body) in _kernels(default).items():
        if name not in inst:
            assert _prio(body) == [], name
    asm = default[0]
    assert len(re.findall(r"\n\s*s_setprio\b", asm)) == sum(len(_map(v["rw"] // 16)) for v in inst.values())


def test_build_without_the_knob_holds_none(without):
    assert not re.search(r"\bs_setprio\b", without[0])


def test_the_two_builds_are_the_same_kernel_line_for_line(default, without):
    a, b = _kernels(default), _kernels(without)
    assert sorted(a) == sorted(b)
    # The six pair-word instances at RW 64 are the exception the compiler makes: the same instructions in the
    # same order on the same vector registers, but a few values of the round head (the round's stream bounds)
    # live in other SCALAR registers, because the statement splits their live ranges elsewhere.  For them the
    # comparison masks the scalar register numbers; the byte-for-byte output comparison on the GPU
    # (profiles/r08_ab_wave_prio.txt, c5 runs these instances) carries the rest of the proof.
    sgpr = lambda lines: [re.sub(r"\bs\d+\b|\bs\[\d+:\d+\]", "s#", l) for l in lines]      # noqa: E731
    renamed = []
    for name, v in _instances(default[1]).items():
        body = _without_prio(a[name][1])
        assert not any("s_setprio" in l for l in body), name
        if body != b[name][1]:
            renamed.append((v["form"], v["rw"]))
            assert sgpr(body) == sgpr(b[name][1]), name
    assert all(k == (0, 64) for k in renamed), renamed


def test_the_priority_costs_no_register(default, without):
    a, b = _instances(default[1]), _instances(without[1])
    assert a == b       # VGPRs, VGPR / SGPR spills, scratch and occupancy of every instance
    for name, v in a.items():
        assert (v["spill"], v["sgpr_spill"], v["scratch"]) == (0, 0, 0), (name, v)
        if v["form"] != 0:
            assert v["vgprs"] == {32: 94, 96: 128}[v["rw"]], (name, v)
