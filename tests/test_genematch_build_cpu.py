"""Build-time check of the gene matching unit (vrx_genematch.h; no GPU: hipcc cross-compiles gfx950): the two
matching passes and the four gene-count kernels keep their registers -- no spill, no scratch -- and the matching
passes hold exactly one gene tile of (start, stop) pairs in LDS (plus the word of the workgroup vote).
Resource usage only."""
import re

import pytest

from tests.device_isa import CSRC, compile_unit

OURS = ("vrx_gm_pass1", "vrx_gm_pass2", "vrx_gc_count", "vrx_gc_emit", "vrx_gc_heads", "vrx_gc_reduce")


@pytest.fixture(scope="module")
def report():
    return compile_unit("vrx_genematch.hip")[1]


def test_genematch_kernels_do_not_spill_and_hold_one_tile(report):
    tile = int(re.search(r"VRX_GM_TILE = (\d+);", open(CSRC + "/vrx_genematch.h").read()).group(1))
    found = {}
    for block in re.split(r"remark: [^\n]*Function Name: ", report)[1:]:
        name = block.split()[0]
        ours = [k for k in OURS if k in name]
        if not ours:
            continue                                                 # the scan and sort kernels of the library
        get = lambda key: int(re.search(key + r": (\d+)", block).group(1))      # noqa: E731
        found[ours[0]] = dict(vgpr_spill=get("VGPRs Spill"), sgpr_spill=get("SGPRs Spill"),
                              scratch=get(r"ScratchSize \[bytes/lane\]"), lds=get(r"LDS Size \[bytes/block\]"))
    assert sorted(found) == sorted(OURS), sorted(found)
    for name, r in found.items():
        assert (r["vgpr_spill"], r["sgpr_spill"], r["scratch"]) == (0, 0, 0), (name, r)
        if name.startswith("vrx_gm_pass"):
            assert 8 * tile <= r["lds"] <= 8 * tile + 512, (name, r)
        else:
            assert r["lds"] == 0, (name, r)
