"""Build-time check of the cell VCF kernels (vrx_cellvcf.h, compiled in vrx_vcf.hip; no GPU: hipcc cross-compiles
gfx950): the line kernel, the two passes over the segments and the row kernel keep their registers -- no spill, no
scratch -- and use no LDS.  The segment length the GPU tests size their lines by is the header's.  Resource usage only."""
import re

import pytest

from tests.device_isa import CSRC, compile_unit

OURS = ("vrx_cellvcf_lines", "vrx_cellvcf_count", "vrx_cellvcf_emit", "vrx_cellvcf_rows")


@pytest.fixture(scope="module")
def report():
    return compile_unit("vrx_vcf.hip")[1]


def test_cell_vcf_kernels_do_not_spill(report):
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
        assert (r["vgpr_spill"], r["sgpr_spill"], r["scratch"], r["lds"]) == (0, 0, 0, 0), (name, r)


def test_exported_segment_is_the_headers():
    import __graft_entry__ as entry
    entry.build()
    from vireo_amd import _lib
    text = open(CSRC + "/vrx_cellvcf.h").read()
    seg = int(re.search(r"#define VRX_CELLVCF_SEGMENT (\d+)", text).group(1))
    assert _lib.lib().vrx_cellvcf_segment() == seg and seg % _lib.lib().vrx_vcf_chunk() == 0
