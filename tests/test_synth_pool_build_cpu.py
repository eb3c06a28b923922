"""Build-time check of the pooling unit (vrx_pool.h; no GPU: hipcc cross-compiles gfx950): the two passes over the
pooled columns and the three scan kernels keep their registers -- no spill, no scratch -- and hold nothing in LDS
but the per-wavefront totals of a workgroup.  The thresholds the GPU tests size their cases by are the header's.
Resource usage only."""
import re

import pytest

from tests.device_isa import CSRC, compile_unit

OURS = ("vrx_pool_passILb0", "vrx_pool_passILb1", "vrx_pool_scan_local", "vrx_pool_scan_blocks", "vrx_pool_scan_add")


@pytest.fixture(scope="module")
def report():
    return compile_unit("vrx_pool.hip")[1]


def test_pool_kernels_do_not_spill(report):
    found = {}
    for block in re.split(r"remark: [^\n]*Function Name: ", report)[1:]:
        name = block.split()[0]
        ours = [k for k in OURS if k in name]
        if not ours:
            continue
        get = lambda key: int(re.search(key + r": (\d+)", block).group(1))      # noqa: E731
        found[ours[0]] = dict(vgpr_spill=get("VGPRs Spill"), sgpr_spill=get("SGPRs Spill"),
                              scratch=get(r"ScratchSize \[bytes/lane\]"), lds=get(r"LDS Size \[bytes/block\]"))
    assert sorted(found) == sorted(OURS), sorted(found)
    for name, r in found.items():
        assert (r["vgpr_spill"], r["sgpr_spill"], r["scratch"]) == (0, 0, 0), (name, r)
        assert r["lds"] <= 64, (name, r)


def test_exported_thresholds_are_the_headers():
    import __graft_entry__ as entry
    entry.build()
    from vireo_amd import _lib
    text = open(CSRC + "/vrx_pool.h").read()
    block = int(re.search(r"VRX_POOL_BLOCK = (\d+);", text).group(1))
    items = int(re.search(r"VRX_POOL_SCAN_ITEMS = (\d+);", text).group(1))
    limit = int(re.search(r"VRX_POOL_WAVE_LIMIT = (\d+);", text).group(1))
    assert _lib.lib().vrx_pool_wave_limit() == limit and limit % 64 == 0
    assert _lib.lib().vrx_pool_scan_block() == block * items
