"""The LDS passes with progress-ordered wave priority (VRX_WAVE_PRIO, vrx_kernels.h) on the GPU.

A wave of `vrx_spmm_lds` lowers its issue priority round by round inside a slab visit, so the waves of a SIMD
advance through a visit unequally on purpose -- and still every wave executes the same instructions on the same
data in the same order.  On the suite's "many" shape (tests/exact_cases.py: 2 600 x 2 300, density 0.03: several
tiles and several slabs per orientation), forced onto the LDS passes, with K = 16 (the flat hot instance), 6
(16-byte units) and 5 (element-wise staging), one and many contracted ranges, default and balanced builds, with
and without rows cut into pieces: three iterations run twice from the same uploaded state give the same trace and
the same end state byte for byte, and the first iteration agrees with the oracle within the parity tests'
tolerance (tests/test_gpu_parity.py: RTOL 1e-5, ATOL 1e-290).
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import vireo_oracle as O
from tests import exact_cases as EC
from tests.test_gpu_parity import ATOL, RTOL

pytestmark = pytest.mark.gpu

T = 3
# (K, VIREO_LDS_BLOCKS, balanced, VIREO_LDS_SPLIT_X10 or None)
CASES = [(K, blocks, balanced, None) for K in (16, 6, 5) for blocks in (1, 16) for balanced in (False, True)]
# VIREO_LDS_SPLIT_X10 is ten times the piece cap in units of the mean row (at least 64 entries): 60 is the setting
# of the suite's balanced cases, which leaves this data's rows whole; 5 caps a piece at 64 entries of the ~70 a
# row holds here, so most rows are cut
CASES += [(16, 16, True, "60"), (16, 16, True, "5"), (6, 16, False, "5")]


@functools.lru_cache(maxsize=None)
def _problem(K):
    """the "many" data with the state and priors of tests/exact_cases.py's cases, and the oracle's first iteration"""
    AD, DP = EC.data("many")
    N, M = AD.shape
    rng = np.random.default_rng(2000 + K)
    g = np.linspace(0.01, 0.99, T)[None, :]
    spec = SimpleNamespace(learn_gt=True, ase=False, fix=False)
    s = SimpleNamespace(ID=O.unit_sum(rng.random((M, K))), GT=O.unit_sum(rng.random((N, K, T))),
                        mu=np.ones((1, T)) * np.linspace(0.01, 0.99, T), sm=np.full((1, T), 50.0))
    pri = SimpleNamespace(ID_prior=None, GT_prior=None, th1=g * 50.0, th2=(1 - g) * 50.0)
    p = SimpleNamespace(spec=spec, AD=AD, DP=DP, N=N, M=M, K=K, T=T, kind="vireo", states=[s], s0=s, pri=pri)
    p.first = EC.OracleBackend(p).run(0, 1)
    return p


@pytest.fixture(scope="module")
def lib():
    from vireo_amd import _lib
    _lib.require_gpu()          # fail loudly: there is no CPU fallback
    return _lib


def _run(dm, s, n):
    dm.set_state(s.ID, s.GT, s.mu, s.sm)
    trace, _ = dm.run_iters(n, 0)
    return (trace,) + tuple(dm.get_state())


@pytest.mark.parametrize("K,blocks,balanced,split", CASES,
                         ids=["K%d-blocks%d-%s%s" % (K, b, "balanced" if bal else "default", "-split%s" % sp if sp else "")
                              for K, b, bal, sp in CASES])
def test_unequal_waves_same_bits(lib, monkeypatch, K, blocks, balanced, split):
    from vireo_amd.counts import DeviceCounts
    from vireo_amd.engine import DeviceModel
    p = _problem(K)
    monkeypatch.setenv("VIREO_LDS", "1")
    monkeypatch.setenv("VIREO_LDS_BLOCKS", str(blocks))
    if balanced:
        monkeypatch.setenv("VIREO_BUILD", "device")
    if split:
        monkeypatch.setenv("VIREO_LDS_SPLIT_X10", split)
    counts = DeviceCounts(p.AD, p.DP, balance=balanced)
    binfo = counts.build_info()
    assert bool(binfo["balanced_variant"]) == bool(binfo["balanced_cell"]) == balanced, binfo
    dm = DeviceModel(counts, lib.KIND_VIREO, K, n_gt=T)
    dm.set_prior(p.pri.ID_prior, p.pri.GT_prior, p.pri.th1, p.pri.th2)
    info = dm.info()
    print("K %d: %s" % (K, info))
    # the AD/BD instances of the kernel (a tile is at most 16 waves x 96 rows: both orientations have several);
    # many contracted ranges unless one workgroup has them all
    assert info["lds_variant"] and info["lds_cell"] and (info["cell_form"], info["var_form"]) == (1, 3), info
    assert min(p.N, p.M) > 16 * 96
    assert (info["ranges_variant"] > 1 and info["ranges_cell"] > 1) == (blocks > 1), info
    if split:
        assert (info["extra_pieces_variant"] > 0 and info["extra_pieces_cell"] > 0) == (split == "5"), info

    a, b = _run(dm, p.s0, 3), _run(dm, p.s0, 3)
    for name, x, y in zip(("trace", "ID_prob", "GT_prob", "beta_mu", "beta_sum"), a, b):
        assert x.tobytes() == y.tobytes(), name
    assert np.isfinite(a[0]).all()

    one, ref = _run(dm, p.s0, 1), p.first
    for name, x, y in zip(("ELBO", "ID_prob", "GT_prob", "beta_mu", "beta_sum"), one,
                          (ref.trace, ref.ID, ref.GT, ref.mu, ref.sm)):
        np.testing.assert_allclose(np.asarray(x), np.asarray(y), rtol=RTOL, atol=ATOL, err_msg=name)
    assert np.array_equal(one[1].argmax(1), ref.ID.argmax(1))
    np.testing.assert_allclose(a[0][0], ref.trace[0], rtol=RTOL)
