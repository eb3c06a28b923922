"""Both VCF readers on the GPU against their host paths on the mutation corpus of tests/vcf_mutate.py: for every file
the device path gives the host path's result bit for bit, or raises the same exception with the same message, under
every slab setting.  The host path itself is held to the real reference on the same corpus in
tests/test_vcf_mutation_cpu.py, so the device stands two exact steps from the reference.  A field-only file (every
mutation inside a sample field of a kept, tagged, matched line, printable ASCII) must be read on the device, and where
its text leaves the device's grammar -- restated in vcf_mutate.donor_repairs / cell_repairs -- at least one of its lines
must come back flagged for the host.  Reads the generator only: no golden file, no reference."""
import contextlib
import io

import numpy as np
import pytest

from tests import cellvcf_util as U
from tests import vcf_mutate as M
from tests.test_gpu_donor_vcf import same

pytestmark = pytest.mark.gpu

DONOR_SLABS = (None, 4096, 1)         # the default slab, several lines a slab, every line a slab of its own
CELL_SLABS = (None, 1)                # the default slab and one that cuts between every two lines
TEXT_ERRORS = ("IndexError", "ValueError", "SystemExit", "UnicodeDecodeError", "UnboundLocalError", "TypeError")


@pytest.fixture(scope="module")
def readers():
    import __graft_entry__ as entry
    entry.build()
    import vireo_amd
    from vireo_amd import _lib
    _lib.require_gpu()
    assert _lib.lib().vrx_vcf_chunk() == M.CHUNK and _lib.lib().vrx_cellvcf_segment() == M.SEGMENT
    return vireo_amd.vcf.load_donor_GPb, vireo_amd.read_cellVCF


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("vcf_mutation")
    return {kind: [f.write(tmp) for f in M.corpus(kind)] for kind in ("donor", "cell")}


def run(fn, **kw):
    kw = {k: v for k, v in kw.items() if v is not None}
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all="ignore"):
        return M.outcome(lambda: fn(**kw))


def differ(dev, host, equal):
    """why the device's outcome is not the host's, or None"""
    if dev[0] == "raise" and dev[1] not in TEXT_ERRORS:             # the library or the GPU, not the text: stop here
        pytest.fail("the device path raised %s: %s" % dev[1:])
    if dev[0] != host[0] or (dev[0] == "raise" and dev[1:] != host[1:]):
        return "device %r, host %r" % tuple(x if x[0] == "raise" else "returns" for x in (dev, host))
    if dev[0] == "ok":
        try:
            equal(dev[1], host[1])
        except AssertionError as e:
            return "results differ: %s" % (str(e).split("\n")[0],)
    return None


@pytest.mark.parametrize("group", range(len(M.groups())))
def test_donor_files(readers, paths, group):
    load = readers[0]
    bad = []
    for k in M.groups()[group]:
        f, path = M.corpus("donor")[k], paths["donor"][k]
        for tag in M.TAGS:
            host = run(load, vcf_file=path, tag=tag, variants=f.cells, force_host=True)
            for slab in DONOR_SLABS:
                dev = run(load, vcf_file=path, tag=tag, variants=f.cells, slab_bytes=slab)
                why = differ(dev, host, same)
                if why is None and f.field_only and dev[0] == "ok":
                    if dev[1]["path"] != "device":
                        why = "a field-only file read on the host: %s" % dev[1]["reason"]
                    elif M.donor_repairs(f, tag) and dev[1]["n_repaired"] < 1:
                        why = "text outside the grammar and no line flagged"
                if why:
                    bad.append((f.name, tag, slab, why, f.mutations))
    assert not bad, "%d disagreements, the first: %r" % (len(bad), bad[:4])


@pytest.mark.parametrize("group", range(len(M.groups())))
def test_cell_files(readers, paths, group):
    read = readers[1]
    bad = []
    for k in M.groups()[group]:
        f, path = M.corpus("cell")[k], paths["cell"][k]
        for bi in (True, False):
            host = run(read, vcf_file=path, biallelic_only=bi, force_host=True)
            for slab in CELL_SLABS:
                dev = run(read, vcf_file=path, biallelic_only=bi, slab_bytes=slab)
                why = differ(dev, host, U.same)
                if why is None and f.field_only:
                    repairs = M.cell_repairs(f)
                    if repairs is None:
                        why = None if dev[:2] == ("raise", "IndexError") else "a short entry that does not raise"
                    elif dev[0] == "ok" and dev[1]["path"] != "device":
                        why = "a field-only file read on the host: %s" % dev[1]["reason"]
                    elif dev[0] == "ok" and repairs and dev[1]["n_repaired"] < 1:
                        why = "text outside the grammar and no line flagged"
                if why:
                    bad.append((f.name, bi, slab, why, f.mutations))
    assert not bad, "%d disagreements, the first: %r" % (len(bad), bad[:4])
