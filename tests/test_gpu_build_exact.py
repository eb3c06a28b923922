"""Both problem builders against the input itself, exactly, case by case.

Every kernel of the EM is held to an extended-precision reference, but on a built problem taken on
trust: the packed entries and gather tables the gather kernels read, the tiled streams
``vrx_spmm_lds`` reads.  Here every case of tests/build_cases.py is built by the host builder
(``VIREO_BUILD=host``) and by the device builder (``VIREO_BUILD=device``: vrx_build.h), and

* **the path** is asserted first -- ``build_info()``'s ``device_built`` and balanced flags,
  ``entry_format()``, and ``info()`` of a ``DeviceModel`` on the counts (the LDS-resident passes, the
  stream forms, the rows cut into pieces) against the case's declaration -- so a builder that
  declines without a word fails the case instead of passing it as the host builder's twin;
* **builder against builder**: digest words 0-4 and 6-10 (packed entries, stream words, boundaries,
  wave starts, row maps of both orientations), ``n_vars()`` -- also against ``(DP > 0).sum(0)`` --
  and ``binom_const()``; a balanced build: the same digest from the device greedy, the host greedy,
  a second build and the orientations one after the other;
* **builder against the input**: with the integer operands of build_cases.py a pass is exact integer
  arithmetic in float64 whatever its order (the CPU twin asserts the 2^53 bound), so every entry of
  ``donor_reads(ID)`` and of ``vrx_problem_cell_loglik`` at one class must EQUAL the SciPy int64
  product: on the streams of both builds and of the balanced build (``VIREO_LDS=1``), and on the host
  build's packed entries and gather tables (``VIREO_LDS=0``) at each entry format.

There is no tolerance in this file.  VIREO_BUILD_EXACT_OUT=<file> writes the table of the run
(profiles/build_exact_cases.txt).
"""
import math
import os

import numpy as np
import pytest

from tests import build_cases as B

pytestmark = pytest.mark.gpu

_ROWS = {}
INFO_K = 5          # the column count of the model whose ``info()`` is read


@pytest.fixture(scope="module")
def va():
    import vireo_amd
    from vireo_amd import _lib
    _lib.require_gpu()          # fail loudly: there is no CPU fallback
    yield vireo_amd
    path = os.environ.get("VIREO_BUILD_EXACT_OUT")
    if path:
        _write_table(path)


def _write_table(path):
    with open(path, "w") as f:
        f.write("# tests/test_gpu_build_exact.py: both problem builders against the int64 products of the input\n"
                "# forms: cell / variant stream (1 / 3: AD/BD words, 0: pair words); fmt: entry format variant / cell;\n"
                "# tiles, ranges, +pieces: variant / cell orientation, as info() reports them on the device build\n"
                "# (a declared fall-back: on the host build); dev: device_built under VIREO_BUILD=device; bal: balanced\n"
                "# streams; digests: host == device build (balanced: == every other route), -: not compared;\n"
                "# builds: problems built and checked; cells: product cells compared; bad: cells that differ\n")
        f.write("%-24s %7s %5s %5s %7s %9s %9s %3s %3s %7s %6s %9s %4s  %s\n"
                % ("case", "nnz", "forms", "fmt", "tiles", "ranges", "+pieces", "dev", "bal", "digests", "builds",
                   "cells", "bad", "tags"))
        for name in B.CASES:
            if name in _ROWS:
                f.write("%-24s %7d %5s %5s %7s %9s %9s %3d %3d %7s %6d %9d %4d  %s\n" % _ROWS[name])
        rows = list(_ROWS.values())
        seen = {t for name, r in _ROWS.items() if r[7] for t in B.CASES[name].tags}
        f.write("\n# %d cases, %d builds, %d product cells compared, %d differ\n"
                % (len(rows), sum(r[10] for r in rows), sum(r[11] for r in rows), sum(r[12] for r in rows)))
        f.write("# feature tags not seen on a device-built case: %s\n"
                % (", ".join(t for t in B.TAGS if t not in seen) or "none"))


def _build(monkeypatch, spec, build, balance=False, **more):
    from vireo_amd.counts import DeviceCounts
    for k in B.ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in B.case_env(spec, build, **more).items():
        monkeypatch.setenv(k, v)
    shape, colptr, rowidx, ad, dp = B.merged(spec.data)
    return DeviceCounts.from_merged(shape, colptr, rowidx, ad, dp, balance=balance)


def _path(counts, spec, m, device_built, balanced, lds, env):
    """what was built, against the declaration -> ``info()``"""
    from vireo_amd import _lib
    from vireo_amd.engine import DeviceModel
    built = counts.build_info()
    assert built["device_built"] == device_built, (built, spec.declines)
    assert (built["balanced_variant"], built["balanced_cell"]) == (balanced, balanced), built
    assert counts.entry_format() == B.expected_format(m, env)
    dm = DeviceModel(counts, _lib.KIND_VIREO, INFO_K)
    info = dm.info()
    dm.close()
    assert (info["lds_variant"], info["lds_cell"]) == (lds, lds), info
    assert (info["fmt_variant"], info["fmt_cell"]) == counts.entry_format()
    if lds:
        assert (info["cell_form"], info["var_form"]) == (spec.cell_form, spec.var_form), info
        want = B.expected_pieces(m, env, spec.var_form)
        assert (info["extra_pieces_variant"], info["extra_pieces_cell"]) == want, (info, want)
        for side, cut in zip(("variant", "cell"), spec.pieces):
            assert cut is None or cut == (info["extra_pieces_" + side] > 0), (side, info)
    return info


def _cell_loglik(counts, GT, psi):
    """as tests/test_gpu_postfit_exact.py calls it: no prior, no posterior"""
    from vireo_amd import _lib
    from vireo_amd._lib import dptr, f64
    GT, psi = f64(GT), [f64(x) for x in psi]
    L = np.full((counts.n_cell, GT.shape[1]), -7.0)
    _lib.check(_lib.lib().vrx_problem_cell_loglik(
        counts.handle, GT.shape[1], GT.shape[2], dptr(GT), dptr(psi[0]), dptr(psi[1]), dptr(psi[2]),
        psi[0].shape[0], None, 0, dptr(L), None))
    return L


def _against_input(counts, op, want, what, tally):
    """every product of the input on one built problem: cells compared, cells that differ, and where"""
    def hold(got, ref, tag):
        n = B.mismatches(got, ref)
        tally["cells"] += ref.size
        tally["bad"] += n
        if n:
            tally["where"].append("%s: %s: %d of %d cells differ" % (what, tag, n, ref.size))

    for K, ID in op.ID.items():
        for got, ref, tag in zip(counts.donor_reads(ID), want["reads", K], ("AD", "DP")):
            hold(got, ref, "%s @ ID of %d columns" % (tag, K))
    for tag, (GT, psi) in op.cell.items():
        hold(_cell_loglik(counts, GT, psi), want["cell", tag], "cell_loglik %s" % tag)
    tally["builds"] += 1


def _same(a, b):
    return a == b or (math.isnan(a) and math.isnan(b))


@pytest.mark.parametrize("name", B.CASES)
def test_builders_against_the_input(va, monkeypatch, name):
    spec = B.CASES[name]
    m = B.merged(spec.data)
    AD, DP = B.matrices(m)
    op = B.operands(name, B.GPU_SEED)
    want = B.products(m, op)
    tally = dict(cells=0, bad=0, builds=0, where=[])

    # ---- the path, before anything else
    host = _build(monkeypatch, spec, "host")
    _path(host, spec, m, False, False, spec.host_lds, spec.env)
    dev = _build(monkeypatch, spec, "device", balance=spec.balance)
    info = _path(dev, spec, m, spec.device_built, spec.balance, spec.device_built or spec.host_lds, spec.env)
    assert host.entry_format() == dev.entry_format() == spec.entry_format

    # ---- builder against builder
    n_vars = np.asarray((DP > 0).sum(0)).ravel()
    for c in (host, dev):
        assert np.array_equal(c.n_vars(), n_vars)
    assert _same(float(host.binom_const()), float(dev.binom_const()))
    digests = "-"
    if spec.device_built and not spec.balance:
        dh, dd = host.digest(), dev.digest()
        assert dd[5] == 0 and dd[11] == 0               # device build: no gather segment tables
        differ = [k for k in (0, 1, 2, 3, 4, 6, 7, 8, 9, 10) if dh[k] != dd[k]]
        assert not differ, "digest words %s differ" % differ
        digests = "equal"
    elif spec.balance:
        plain = _build(monkeypatch, spec, "device", balance=False)
        assert not plain.build_info()["balanced_cell"] and plain.digest() != dev.digest()
        assert plain.digest()[0] == dev.digest()[0] and plain.digest()[6] == dev.digest()[6]     # (packed entries)
        plain.close()
        greedy = "device" if spec.env.get("VIREO_BALANCE_GREEDY") == "host" else "host"
        for more in (dict(), dict(VIREO_BALANCE_GREEDY=greedy), dict(VIREO_BUILD_CONCURRENT="0")):
            again = _build(monkeypatch, spec, "device", balance=True, **more)
            assert again.build_info()["balanced_variant"] and again.build_info()["balanced_cell"]
            assert again.digest() == dev.digest(), more
            again.close()
        digests = "equal"

    # ---- builder against the input: the streams of both builds (VIREO_LDS=1, as built) ...
    _against_input(host, op, want, "host build, streams", tally)
    _against_input(dev, op, want, "balanced build" if spec.balance else "device build", tally)
    host.close()
    dev.close()
    # ... and the host build's packed entries and gather tables, at each entry format that holds the counts
    # (a case that sets the format itself: at that one)
    own = "VIREO_ENTRY_FMT" in spec.env
    for fmt in [spec.entry_format[0]] if own else range(spec.entry_format[0], 3):
        env = dict(spec.env, VIREO_LDS="0", VIREO_ENTRY_FMT=str(fmt))
        gather = _build(monkeypatch, spec, "host", VIREO_LDS="0", VIREO_ENTRY_FMT=str(fmt))
        _path(gather, spec, m, False, False, False, env)
        assert gather.entry_format() == (fmt, fmt)
        _against_input(gather, op, want, "host build, gather kernels, format %d" % fmt, tally)
        gather.close()

    _ROWS[name] = (name, m[2].size, "%d/%d" % (spec.cell_form, spec.var_form), "%d/%d" % spec.entry_format,
                   "%d/%d" % (info["tiles_variant"], info["tiles_cell"]),
                   "%d/%d" % (info["ranges_variant"], info["ranges_cell"]),
                   "%d/%d" % (info["extra_pieces_variant"], info["extra_pieces_cell"]),
                   int(spec.device_built), int(spec.balance), digests, tally["builds"], tally["cells"], tally["bad"],
                   ",".join(spec.tags))
    assert tally["cells"] == tally["builds"] * B.count_cells(want)
    assert tally["bad"] == 0, "\n".join(tally["where"])


@pytest.mark.parametrize("name,build", [("zeros", "host"), ("zeros", "device"), ("top2048", "device"),
                                        ("top2047", "device"), ("heavy", "device")])
def test_a_damaged_input_is_seen_on_the_device(va, monkeypatch, name, build):
    """the comparison above can fail: a problem built from a copy of the input with one planted defect of
    build_cases.py (an entry dropped or doubled, two row indices swapped, ad and dp exchanged, the last entry
    lost, a count of 2048 wrapped) differs from the clean input's products on the device as it does in NumPy"""
    from vireo_amd.counts import DeviceCounts
    spec = B.CASES[name]
    m = B.merged(spec.data)
    op = B.operands(name, B.GPU_SEED)
    want = B.products(m, op)
    for k in B.ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in B.case_env(spec, build).items():
        monkeypatch.setenv(k, v)
    applied = 0
    for what, damage in B.DEFECTS.items():
        bad = damage(m, np.random.default_rng(len(what)))
        if bad is None:
            continue
        applied += 1
        counts = DeviceCounts.from_merged(*bad, balance=spec.balance)
        assert counts.build_info()["device_built"] == (build == "device")
        tally = dict(cells=0, bad=0, builds=0, where=[])
        _against_input(counts, op, want, what, tally)
        counts.close()
        in_numpy = sum(B.mismatches(x.astype(np.float64), y) for k, v in B.products(bad, op).items()
                       for x, y in zip(v if isinstance(v, tuple) else (v,),
                                       want[k] if isinstance(v, tuple) else (want[k],)))
        assert tally["bad"] == in_numpy > 0, (what, tally["bad"], in_numpy)
    assert applied == (6 if name == "top2048" else 5)
