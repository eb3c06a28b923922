"""Build-time check of the per-variant mixture kernel (vrx_varmix.h; no GPU: hipcc cross-compiles gfx950): every
instance keeps its registers -- no VGPR / SGPR spill, no scratch (the 3 K + 2 accumulators and the K-wide
softmax of an entry are arrays in the source and must stay registers).  Resource usage only.

The report names kernels only: the theta step, vrx_vm_theta<K>, is a called function and has no entry of its
own.  It is covered through its callers -- a kernel's ScratchSize includes the stack of everything it calls,
and "Dynamic Stack: False" says that size is known -- so a callee that grows a stack fails here too."""
import re

import pytest

from tests.device_isa import compile_unit


@pytest.fixture(scope="module")
def report():
    return compile_unit("vrx_varmix.hip")[1]


def test_varmix_kernels_do_not_spill(report):
    found = {}
    for block in re.split(r"remark: [^\n]*Function Name: ", report)[1:]:
        name = block.split()[0]
        get = lambda key: int(re.search(key + r": (\d+)", block).group(1))      # noqa: E731
        found[name] = dict(vgpr_spill=get("VGPRs Spill"), sgpr_spill=get("SGPRs Spill"),
                           scratch=get(r"ScratchSize \[bytes/lane\]"),
                           dynamic_stack=re.search(r"Dynamic Stack: (\w+)", block).group(1))
    # one kernel per number of components, 2 ... 8, and no other kernel in the unit
    want = sorted("vrx_varmix_fit_kILi%dE" % K for K in range(2, 9))
    assert sorted(re.search(r"vrx_varmix_fit_kILi\dE", n).group(0) for n in found) == want, sorted(found)
    for name, r in found.items():
        assert r == dict(vgpr_spill=0, sgpr_spill=0, scratch=0, dynamic_stack="False"), (name, r)
