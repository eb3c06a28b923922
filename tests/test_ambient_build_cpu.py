"""Build-time check of the ambient-RNA kernels (vrx_ambient.h; no GPU: hipcc cross-compiles gfx950):
every one of them keeps its registers -- no VGPR / SGPR spill, no scratch."""
import re

import pytest

from tests.device_isa import compile_unit


@pytest.fixture(scope="module")
def report():
    return compile_unit("vrx_engine.hip")[1]


def test_ambient_kernels_do_not_spill(report):
    found = {}
    for block in re.split(r"remark: [^\n]*Function Name: ", report)[1:]:
        name = block.split()[0]
        if "vrx_amb_" not in name:
            continue
        get = lambda key: int(re.search(key + r": (\d+)", block).group(1))      # noqa: E731
        found[name] = dict(vgpr_spill=get("VGPRs Spill"), sgpr_spill=get("SGPRs Spill"),
                           scratch=get(r"ScratchSize \[bytes/lane\]"))
    for kernel in ("vrx_amb_gain", "vrx_amb_count", "vrx_amb_scatter", "vrx_amb_em"):
        assert any(kernel in n for n in found), (kernel, sorted(found))
    assert len([n for n in found if "vrx_amb_count" in n]) == 3          # one per entry format
    for name, r in found.items():
        assert r == dict(vgpr_spill=0, sgpr_spill=0, scratch=0), (name, r)
