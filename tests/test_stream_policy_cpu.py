"""Cache policy of the LDS passes' loads, read in the ISA (no GPU: hipcc cross-compiles gfx950).

Every entry word is read by exactly one wave, once per pass, so the LDS-DMA that feeds a wave's ring is
issued non-temporally (`nt`, VRX_STREAM_NT in vrx_kernels.h): the stream then does not push the data a pass
does re-use -- the slab operand every tile stages again, the partial planes -- out of L2 and the Infinity
Cache.  The slab prefetch must NOT take that policy (its rows are fetched again by every tile), and the policy
bit must cost the walk nothing: same registers as before it, no spill.
"""
import re

import pytest

from tests.device_isa import compile_unit
from tests.test_kernel_build_cpu import _instances

# VGPRs of the AD/BD instances by rows per wave, as they stood before the stream took a cache policy
# (profiles/r04_spmm_lds_resource_usage.txt): RW 96 fills the 128 registers of a 1024-thread workgroup
VGPRS = {32: 94, 96: 128}


@pytest.fixture(scope="module")
def isa():
    return compile_unit("vrx_engine.hip")


def _bodies(isa):
    asm, report = isa
    inst = _instances(report)
    out = {}
    for name, v in inst.items():
        body = asm[asm.index("\n" + name + ":"):]
        out[name] = (v, body[:body.index("s_endpgm")].split("\n"))
    return out


def test_entry_stream_is_loaded_non_temporally(isa):
    bodies = _bodies(isa)
    hot = {k: b for k, b in bodies.items() if b[0]["form"] != 0}
    assert len(hot) == 6, sorted(hot)
    for name, (v, body) in bodies.items():        # the pair-word instances walk the same ring
        dma = [l.strip() for l in body if re.match(r"\s*global_load_lds_dwordx4\b", l)]
        # the chunk issued ahead of the walk + the one every ring event issues (the walk's rounds share it or
        # hold a copy each: at least two, and every one of them carries the policy)
        assert len(dma) >= 2, (name, dma)
        assert all(re.search(r"\bnt\b", l) for l in dma), (name, dma)
        assert not any(re.search(r"\b(sc0|sc1)\b", l) for l in dma), (name, dma)


def test_slab_prefetch_keeps_the_default_policy(isa):
    for name, (v, body) in _bodies(isa).items():
        if v["form"] == 0:
            continue
        unit = r"\s*global_load_dwordx2\b" if v["padk"] == 1 else r"\s*global_load_dwordx4\b"
        pf = [l.strip() for l in body if re.match(unit, l)]
        assert pf, name
        assert not any(re.search(r"\b(nt|sc0|sc1)\b", l) for l in pf), (name, pf)
        # the per-slab records (bnd words, the rows a wave stages) were measured with `nt` too: slower, left alone
        rec = [l.strip() for l in body if re.match(r"\s*global_load_dword\b", l)]
        assert rec and not any(re.search(r"\bnt\b", l) for l in rec), (name, rec)


def test_policy_costs_the_ad_bd_instances_no_register(isa):
    for name, (v, body) in _bodies(isa).items():
        if v["form"] == 0:
            continue
        assert v["vgprs"] == VGPRS[v["rw"]], (name, v)
        assert (v["spill"], v["sgpr_spill"], v["scratch"]) == (0, 0, 0), (name, v)
