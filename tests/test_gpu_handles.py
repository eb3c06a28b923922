"""Every Python wrapper of a library handle on its smallest valid input: one real call equals, bit for bit, the
same call on a second, fresh object; ``close()`` may be called twice; a method of the closed object raises
``VrxError`` in Python -- no stale pointer is ever handed to the library.  The readers and the gene calls, which
hold their handle for one ``with`` block, are called twice and their owner is closed on the library's own create."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    entry.build()
    from vireo_amd import _lib
    _lib.require_gpu()
    return _lib


def same(a, b):
    """bit for bit, through dicts, sequences, arrays and sparse matrices (wall-clock fields left out)"""
    assert type(a) is type(b), (type(a), type(b))
    if isinstance(a, dict):
        assert a.keys() == b.keys()
        for k in a:
            if k not in ("seconds", "kernel_ms"):
                same(a[k], b[k])
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            same(x, y)
    elif sp.issparse(a):
        assert a.shape == b.shape
        for k in ("data", "indices", "indptr"):
            same(getattr(a, k), getattr(b, k))
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape
        assert a.tobytes() == b.tobytes() if a.dtype != object else list(a) == list(b)
    elif isinstance(a, float):
        assert np.float64(a).tobytes() == np.float64(b).tobytes()
    else:
        assert a == b


def closes(lib, obj, call):
    obj.close()
    obj.close()
    with pytest.raises(lib.VrxError, match="is closed"):
        call(obj)


def counts_8x6():
    rng = np.random.default_rng(5)
    at = rng.choice(48, size=12, replace=False)
    DP = np.zeros(48, dtype=np.int64)
    DP[at] = rng.integers(1, 9, size=12)
    AD = (DP * rng.random(48)).astype(np.int64)
    return sp.csc_matrix(AD.reshape(8, 6)), sp.csc_matrix(DP.reshape(8, 6))


def test_device_counts(lib):
    from vireo_amd.counts import DeviceCounts
    AD, DP = counts_8x6()
    ID = np.random.default_rng(0).dirichlet(np.ones(2), size=6)

    def call(c):
        return c.n_vars(), c.donor_reads(ID), c.binom_const(), c.digest()

    a, b = DeviceCounts(AD, DP), DeviceCounts(AD, DP)
    assert a.nnz == 12 and a.handle is a._h
    same(call(a), call(b))
    b.close()
    closes(lib, a, lambda c: c.n_vars())
    with pytest.raises(lib.VrxError, match="DeviceCounts is closed"):
        a.handle


def test_device_model(lib):
    from vireo_amd.counts import DeviceCounts
    from vireo_amd.engine import DeviceModel
    AD, DP = counts_8x6()
    rng = np.random.default_rng(1)
    ID, GT = rng.dirichlet(np.ones(2), size=6), rng.dirichlet(np.ones(3), size=(8, 2))
    mu, sm = np.array([[0.01, 0.5, 0.99]]), np.array([[50.0, 50.0, 50.0]])

    def call(m):
        m.set_state(ID, GT, mu, sm)
        m.set_prior(None, None, np.array([[0.3, 3.0, 29.7]]), np.array([[29.7, 3.0, 0.3]]))
        trace, it, flags = m.fit(4, 2, 1e-2)
        return trace, it, flags, m.get_state()

    counts = DeviceCounts(AD, DP)
    a, b = (DeviceModel(counts, lib.KIND_VIREO, 2) for _ in range(2))
    same(call(a), call(b))
    b.close()
    closes(lib, a, lambda m: m.get_state())
    assert len(counts.n_vars()) == 6                    # (the problem outlives its models)
    counts.close()


def bulk_4x2x3():
    rng = np.random.default_rng(2)
    DP = rng.integers(5, 40, size=4).astype(np.float64)
    return np.floor(DP * rng.random(4)), DP, rng.dirichlet(np.ones(3), size=(4, 2))


def test_bulk_data(lib):
    from vireo_amd.vireo_bulk import BulkData
    AD, DP, GT = bulk_4x2x3()

    def call(d):
        return d.fit([0.5, 0.5], [0.01, 0.5, 0.99], max_iter=10), d.loglik([[0.3, 0.7], [0.5, 0.5]], [0.01, 0.5, 0.99])

    a, b = BulkData(AD, DP, GT), BulkData(AD, DP, GT)
    ra, rb = call(a), call(b)
    same((ra[0][:4], ra[1]), (rb[0][:4], rb[1]))            # (the fifth value of a fit is its device time)
    b.close()
    closes(lib, a, lambda d: d.info())


def test_variant_mixtures(lib):
    from vireo_amd.variant_mixture import VariantMixtures
    DP = np.array([[4, 0, 7, 2, 9], [0, 3, 0, 0, 5], [6, 6, 1, 0, 0]])
    AD = np.array([[1, 0, 7, 0, 2], [0, 3, 0, 0, 0], [3, 0, 1, 0, 0]])
    a, b = VariantMixtures(AD, DP), VariantMixtures(AD, DP)
    same(a.fit(n_clone=2, max_iter=20, min_iter=2), b.fit(n_clone=2, max_iter=20, min_iter=2))
    b.close()
    closes(lib, a, lambda v: v.fit(n_clone=2, max_iter=20, min_iter=2))


def test_barcode_rounds(lib):
    from vireo_amd.variant_select import BarcodeRounds
    GT = np.array([[0, 1, 2], [1, 1, 0], [0, 0, 0], [2, 1, 0]])

    def call(r):
        return r.round(), r.pick(0), r.entropies()

    a, b = BarcodeRounds(GT, var_count=[3.0, 9.0, 1.0, 9.0]), BarcodeRounds(GT, var_count=[3.0, 9.0, 1.0, 9.0])
    same(call(a), call(b))
    b.close()
    closes(lib, a, lambda r: r.round())


def test_device_pool(lib):
    from vireo_amd.synth_pool import DevicePool, PoolPlan
    DP = sp.csc_matrix(np.array([[2, 0, 1], [0, 4, 4], [3, 1, 0], [0, 0, 6]]))
    AD = sp.csc_matrix(np.array([[1, 0, 1], [0, 0, 3], [3, 1, 0], [0, 0, 2]]))
    plan = PoolPlan(["a", "b"], [0, 1], [2, -1], [3])
    a, b = DevicePool([(AD, DP)]), DevicePool([(AD, DP)])
    ra = a.run(plan, merged=True)
    assert ra[0] == (4, 2) and int(ra[1][-1]) == len(ra[2])
    same(ra, b.run(plan, merged=True))
    b.close()
    closes(lib, a, lambda p: p.run(plan, merged=True))


def owner_closes(lib, name, create, destroy):
    """the owner of a one-call handle, on the library's own create and destroy"""
    with lib.Handle(name, create, destroy) as h:
        assert h.ptr.value
    closes(lib, h, lambda x: x.ptr)


def test_gene_match_and_gene_counts(lib):
    from vireo_amd import gene_match as gm
    snps = dict(CHROM=["1", "1", "2"], POS=[150, 1000000, 40])
    genes = dict(chrom=["1", "2"], start=[100, 10], stop=[200, 90], gene=np.array(["G1", "G2"]))
    first, second = gm.snp_gene_match(snps, genes), gm.snp_gene_match(snps, genes)
    same(first, second)
    gene_list, flags = first
    assert [list(g) for g in gene_list] == [["G1"], [], ["G2"]] and flags[1] == 4
    AD, DP = counts_8x6()
    AD, DP = AD[:3], DP[:3]
    same(gm.gene_counts(AD, DP, gene_list), gm.gene_counts(AD, DP, gene_list))
    L = lib.lib()
    i64, i32 = np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int32)
    p64, p32 = i64.ctypes.data_as(lib._I64), i32.ctypes.data_as(lib._I32)
    owner_closes(lib, "the gene table", lambda out: L.vrx_genematch_create(0, 0, 0, p64, p32, p32, p32, out),
                 L.vrx_genematch_destroy)
    n_out, ms = C.c_int64(0), C.c_double(0.0)
    owner_closes(lib, "the gene counts",                    # (nothing to count: the handle without a stream)
                 lambda out: L.vrx_genecount_create(0, 0, 0, 0, p64, p32, p32, p32, p64, p32, out, C.byref(n_out),
                                                    C.byref(ms)), L.vrx_genecount_destroy)


def test_cell_vcf_reader(lib):
    from vireo_amd.io_utils import read_cellVCF
    path = os.path.join(GOLD, "cell_vcf", "plain.vcf.gz")
    first, second = read_cellVCF(path), read_cellVCF(path)
    assert first["path"] == "device" and first["reason"] is None
    same(first, second)
    L = lib.lib()
    owner_closes(lib, "the cell VCF reader", lambda out: L.vrx_cellvcf_create(0, 1, 1, out), L.vrx_cellvcf_destroy)


def test_donor_vcf_reader(lib):
    from vireo_amd.vcf_utils import load_donor_GPb
    path = os.path.join(GOLD, "donor_vcf", "chr.vcf.gz")
    variants = [str(x) for x in np.load(os.path.join(GOLD, "donor_vcf", "chr.npz"))["list_inorder"]]
    with np.errstate(invalid="ignore", divide="ignore"):
        first, second = load_donor_GPb(path, "GT", variants), load_donor_GPb(path, "GT", variants)
    assert first["path"] == "device" and first["reason"] is None
    same(first, second)
    L = lib.lib()
    owner_closes(lib, "the donor VCF reader", lambda out: L.vrx_vcf_create(0, 0, 1, 1, -1, None, None, None, out),
                 L.vrx_vcf_destroy)


@pytest.mark.parametrize("wrapper", ("DeviceCounts", "BulkData"))
def test_200_create_close_rounds(lib, wrapper):
    if wrapper == "DeviceCounts":
        from vireo_amd.counts import DeviceCounts
        AD, DP = counts_8x6()
        make, call = (lambda: DeviceCounts(AD, DP)), (lambda c: int(c.n_vars().sum()))
    else:
        from vireo_amd.vireo_bulk import BulkData
        AD, DP, GT = bulk_4x2x3()
        make, call = (lambda: BulkData(AD, DP, GT)), (lambda d: float(d.loglik([0.5, 0.5], [0.01, 0.5, 0.99])))
    want = None
    for _ in range(200):
        obj = make()
        got = call(obj)
        obj.close()
        want = got if want is None else want
        assert got == want
