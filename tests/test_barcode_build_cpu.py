"""Build-time check of the barcode-selection kernels (vrx_barcode.h; no GPU: hipcc cross-compiles gfx950):
every instance keeps its registers -- no VGPR / SGPR spill, no scratch (the class counters and the eight
accumulators of the sum rule are arrays in the source and must stay registers)."""
import re

import pytest

from tests.device_isa import compile_unit

KERNELS = ("vrx_barcode_entropy", "vrx_barcode_max", "vrx_barcode_max2", "vrx_barcode_flag", "vrx_barcode_gather",
           "vrx_barcode_median", "vrx_barcode_flag_ge")


@pytest.fixture(scope="module")
def report():
    return compile_unit("vrx_barcode.hip")[1]


def test_barcode_kernels_do_not_spill(report):
    found = {}
    for block in re.split(r"remark: [^\n]*Function Name: ", report)[1:]:
        name = block.split()[0]
        if "vrx_barcode_" not in name:
            continue
        get = lambda key: int(re.search(key + r": (\d+)", block).group(1))      # noqa: E731
        found[name] = dict(vgpr_spill=get("VGPRs Spill"), sgpr_spill=get("SGPRs Spill"),
                           scratch=get(r"ScratchSize \[bytes/lane\]"))
    for kernel in KERNELS:
        assert any(re.match(r"_Z\d+%s(I|[a-zP])" % kernel, n) for n in found), (kernel, sorted(found))
    # the instance for at most 3 categories and the one for at most 10
    assert sorted(n for n in found if "vrx_barcode_entropyILi" in n) == sorted(
        n for n in found if "vrx_barcode_entropyILi3E" in n or "vrx_barcode_entropyILi10E" in n)
    assert len([n for n in found if "vrx_barcode_entropyILi" in n]) == 2
    assert len(found) == len(KERNELS) + 1
    for name, r in found.items():
        assert r == dict(vgpr_spill=0, sgpr_spill=0, scratch=0), (name, r)
