"""The device-only compile the build-time checks share (no GPU: hipcc cross-compiles gfx950): one unit of
vireo_amd/csrc/ with the build's flags, once per unit and process."""
import functools
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vireo_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@functools.lru_cache(maxsize=None)
def compile_unit(unit):
    """(gfx950 assembly, -Rpass-analysis=kernel-resource-usage report) of csrc/<unit>; skips without hipcc"""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    with tempfile.TemporaryDirectory(prefix="isa_") as d:
        asm = os.path.join(d, "unit.s")
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                            "--cuda-device-only", "-S", "-o", asm, unit, "-Rpass-analysis=kernel-resource-usage"],
                           cwd=CSRC, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
        return open(asm).read(), r.stderr
