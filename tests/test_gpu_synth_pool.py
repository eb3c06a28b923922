"""pool_counts / synth_pool on the GPU (vrx_pool.h).  Everything is an integer and compared with ==: the wanted
matrices are ``X_all @ P`` in SciPy int64 for the 0/1 source x pooled matrix P, and ``(got != want).nnz == 0``;
indices are sorted and neither matrix stores a zero.

Shapes are the smallest at which the kernels can go wrong.  W = vrx_pool_wave_limit() (a pooled column whose
sources hold more entries goes from a wavefront to a workgroup), B = vrx_pool_scan_block() (pooled columns per
workgroup of the offset scan), n_var = W + 70: column lengths 0 ... W + 1 alone and in every pair, the row
patterns of a pair, pooled-cell counts around B, sub-plans, the 2^31 error, the input formats, the c1 counts
pooled by every committed plan of the reference, vireo_wrap on the result, and the command as a child process."""
import functools
import gzip
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
from scipy.sparse import csc_matrix, csr_matrix, hstack

from tests import gold
from tests import synthpool_np as SN

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sp():
    import __graft_entry__ as entry
    entry.build()
    from vireo_amd import _lib, synth_pool
    _lib.require_gpu()
    return synth_pool


def limits():
    from vireo_amd import _lib
    return int(_lib.lib().vrx_pool_wave_limit()), int(_lib.lib().vrx_pool_scan_block())


def columns(n_var, rows, rng, ad_zero=False):
    """(AD, DP) int64 CSC with the given row sets as columns: dp in 1 ... 5, ad binomial (zeros included)"""
    indptr = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in rows], out=indptr[1:])
    idx = np.concatenate([np.asarray(r, dtype=np.int32) for r in rows]) if rows else np.zeros(0, dtype=np.int32)
    dp = rng.integers(1, 6, idx.size)
    ad = np.zeros_like(dp) if ad_zero else rng.binomial(dp, 0.4)
    DP = csc_matrix((dp, idx, indptr), shape=(n_var, len(rows)))
    AD = csc_matrix((ad, idx.copy(), indptr.copy()), shape=(n_var, len(rows)))
    AD.eliminate_zeros()
    return AD, DP


def canonical(X):
    chk = X.copy()
    chk.has_canonical_format = False
    chk.sum_duplicates()
    return chk.nnz == X.nnz and np.array_equal(chk.indices, X.indices) and np.array_equal(chk.indptr, X.indptr)


def check(sp, samples, plan):
    """device == SciPy on both matrices, in both return forms -> (AD, DP, merged)"""
    A_all = hstack([csc_matrix(s[0]).astype(np.int64) for s in samples], format="csc")
    D_all = hstack([csc_matrix(s[1]).astype(np.int64) for s in samples], format="csc")
    P = plan.matrix()
    wantA, wantD = (A_all @ P).tocsc(), (D_all @ P).tocsc()
    AD, DP = sp.pool_counts(samples, plan)
    for got, want in ((AD, wantA), (DP, wantD)):
        assert isinstance(got, csc_matrix) and got.dtype == np.int64 and got.shape == want.shape
        assert (got != want).nnz == 0
        assert got.has_sorted_indices and canonical(got) and not np.any(got.data == 0)
        want.eliminate_zeros()
        assert got.nnz == want.nnz
    shape, colptr, rowidx, ad, dp = merged = sp.pool_counts(samples, plan, merged=True)
    assert shape == wantD.shape and colptr.dtype == np.int64 and colptr[0] == 0 and colptr[-1] == rowidx.size
    assert rowidx.dtype == ad.dtype == dp.dtype == np.int32
    union = ((wantA + wantD) != 0).tocsc()
    union.sort_indices()
    assert np.array_equal(colptr, union.indptr) and np.array_equal(rowidx, union.indices)
    assert (csc_matrix((dp.astype(np.int64), rowidx, colptr), shape=shape) != wantD).nnz == 0
    assert (csc_matrix((ad.astype(np.int64), rowidx, colptr), shape=shape) != wantA).nnz == 0
    return AD, DP, merged


def names(n):
    return np.array(["CELL%06d-1" % i for i in range(n)])


def test_column_lengths_alone_and_in_every_pair(sp):
    W, _ = limits()
    n_var = W + 70
    lens = [0, 1, 2, 63, 64, 65, 127, 128, 129, W - 1, W, W + 1]
    rng = np.random.default_rng(1)
    one = columns(n_var, [np.sort(rng.choice(n_var, n, replace=False)) for n in lens], rng)
    two = columns(n_var, [np.sort(rng.choice(n_var, n, replace=False)) for n in lens], rng)
    L = len(lens)
    src0 = list(range(2 * L)) + [a for a in range(L) for b in range(L)]
    src1 = [-1] * (2 * L) + [L + b for a in range(L) for b in range(L)]
    order = rng.permutation(len(src0))                                # long and short columns interleaved
    plan = sp.PoolPlan(names(len(src0)), np.array(src0)[order], np.array(src1)[order], [L, L])
    AD, DP, merged = check(sp, [one, two], plan)
    got = np.diff(DP.indptr)[np.argsort(order)]
    assert got[:L].tolist() == lens and got[L:2 * L].tolist() == lens
    pair = got[2 * L:].reshape(L, L)
    assert pair[0].tolist() == lens and pair[:, 0].tolist() == lens   # an empty partner
    assert pair[-1, -1] <= n_var < 2 * (W + 1)                        # long columns overlap


@pytest.mark.parametrize("big", [False, True], ids=["wavefront", "workgroup"])
def test_row_patterns_of_a_pair(sp, big):
    W, _ = limits()
    n_var = W + 70
    n = W // 2 + 30 if big else 37                                    # a pair holds 2 n entries: above / below W
    assert (2 * n > W) == big and 4 * n + 2 <= 2 * n_var
    rng = np.random.default_rng(2)
    base = np.sort(rng.choice(n_var, n, replace=False))
    even, odd = np.arange(0, 2 * n, 2), np.arange(1, 2 * n, 2)
    low, high = np.arange(n), np.arange(n_var - n, n_var)
    first_a, first_b = np.arange(5, 5 + n), np.concatenate([[5], np.arange(5 + n, 4 + 2 * n)])
    last_a, last_b = np.arange(n_var - n, n_var), np.concatenate([np.arange(n - 1), [n_var - 1]])
    rows = [base, base.copy(), even, odd, low, high, first_a, first_b, last_a, last_b, np.zeros(0, dtype=np.int64)]
    AD, DP = columns(n_var, rows, rng)
    zero_ad = columns(n_var, [base, odd], rng, ad_zero=True)          # ad = 0 where dp > 0
    E = len(rows) - 1
    pairs = [(0, 1), (2, 3), (3, 2), (4, 5), (5, 4), (6, 7), (7, 6), (8, 9), (9, 8), (0, E), (E, 0), (E, E), (E, -1),
             (0, 0), (0, -1), (0, 2), (0, 3), (0 + len(rows), 1 + len(rows)), (0, len(rows)), (2, 1 + len(rows))]
    plan = sp.PoolPlan(names(len(pairs)), [p[0] for p in pairs], [p[1] for p in pairs], [len(rows), 2])
    gotA, gotD, _ = check(sp, [(AD, DP), zero_ad], plan)
    lens = np.diff(gotD.indptr).tolist()
    assert lens[:9] == [n, 2 * n, 2 * n, 2 * n, 2 * n, 2 * n - 1, 2 * n - 1, 2 * n - 1, 2 * n - 1]
    assert lens[9:15] == [n, n, 0, 0, n, n]
    assert np.array_equal(gotD[:, 13].toarray(), 2 * DP[:, 0].toarray())      # a source pooled with itself
    assert gotA[:, 17].nnz == 0 and gotD[:, 17].nnz == lens[17] > n           # ad stays 0 where only dp adds
    assert gotA[:, 18].nnz == AD[:, 0].nnz and lens[18] == n                  # identical rows, one side without ad


def test_pooled_cell_counts_around_the_scan_block(sp):
    _, B = limits()
    rng = np.random.default_rng(3)
    n_var, n_src = 23, 50
    rows = [np.sort(rng.choice(n_var, rng.integers(0, 4), replace=False)) for _ in range(n_src)]
    sample = columns(n_var, rows, rng)
    for n in (0, 1, B - 1, B, B + 1, 3 * B + 5):
        src0 = rng.integers(0, n_src, n)
        src1 = np.where(rng.random(n) < 0.5, rng.integers(0, n_src, n), -1)
        AD, DP, merged = check(sp, [sample], sp.PoolPlan(names(n), src0, src1, [n_src]))
        assert DP.shape == (n_var, n) and merged[1].size == n + 1


def test_a_sub_plan_gives_the_same_columns(sp):
    W, _ = limits()
    n_var = W + 70
    rng = np.random.default_rng(4)
    lens = rng.choice([0, 3, 70, 700, W // 2 + 5, W + 1], 40)
    sample = columns(n_var, [np.sort(rng.choice(n_var, n, replace=False)) for n in lens], rng)
    n = 90
    src0 = rng.integers(0, 40, n)
    src1 = np.where(rng.random(n) < 0.6, rng.integers(0, 40, n), -1)
    plan = sp.PoolPlan(names(n), src0, src1, [40])
    pool = sp.DevicePool([sample])
    shape, colptr, rowidx, ad, dp = pool.run(plan, merged=True)
    again = pool.run(plan, merged=True)
    assert all(np.array_equal(a, b) for a, b in zip((colptr, rowidx, ad, dp), again[1:]))    # run to run
    for pick in (np.arange(0, n, 7), rng.permutation(n)[:31], np.array([n - 1])):
        s_shape, s_colptr, s_rowidx, s_ad, s_dp = pool.run(plan.subset(pick), merged=True)
        assert s_shape == (n_var, pick.size)
        for k, j in enumerate(pick):
            a, b = slice(colptr[j], colptr[j + 1]), slice(s_colptr[k], s_colptr[k + 1])
            assert np.array_equal(rowidx[a], s_rowidx[b]) and np.array_equal(ad[a], s_ad[b])
            assert np.array_equal(dp[a], s_dp[b])
    pool.close()


def test_a_sum_of_two_to_the_31_is_an_error_naming_the_barcode(sp):
    big = 2 ** 30
    DP = np.zeros((5, 4), dtype=np.int64)
    DP[1, 0] = DP[1, 1] = big
    DP[3, 2] = big
    DP[3, 3] = big - 1
    DP[0, 0] = DP[4, 3] = 7
    AD = DP // 2
    ok = sp.PoolPlan(["good-1", "fine-1"], [2, 0], [3, -1], [4])
    gotA, gotD, _ = check(sp, [(AD, DP)], ok)
    assert gotD[3, 0] == 2 ** 31 - 1 and gotD.dtype == np.int64 and gotD[1, 1] == big
    bad = sp.PoolPlan(["good-1", "toomuch-1D", "fine-1"], [2, 0, 0], [3, 1, -1], [4])
    with pytest.raises(ValueError, match="'toomuch-1D'"):
        sp.pool_counts([(AD, DP)], bad)
    less = DP.copy()
    less[1, 1] -= 1                                                  # dp adds up to 2^31 - 1, ad alone to 2^31
    with pytest.raises(ValueError, match="'toomuch-1D'"):
        sp.pool_counts([(DP, less)], sp.PoolPlan(["toomuch-1D"], [0], [1], [4]))


def test_input_formats_give_the_same_result(sp):
    rng = np.random.default_rng(5)
    n_var = 300
    rows = [np.sort(rng.choice(n_var, n, replace=False)) for n in (0, 5, 64, 130, 299, 300)]
    A1, D1 = columns(n_var, rows, rng)
    A2, D2 = columns(n_var, rows[::-1], rng)
    plan = sp.PoolPlan(names(5), [0, 7, 2, 3, 11], [6, 1, -1, 9, 5], [6, 6])
    refA, refD, ref_m = check(sp, [(A1, D1), (A2, D2)], plan)
    for conv in (lambda X: csr_matrix(X).astype(np.float64), lambda X: X.toarray(),
                 lambda X: X.astype(np.int32)):
        gotA, gotD = sp.pool_counts([(conv(A1), conv(D1)), (A2, conv(D2))], plan)
        assert (gotA != refA).nnz == 0 and (gotD != refD).nnz == 0 and gotD.nnz == refD.nnz
        m = sp.pool_counts([(conv(A1), conv(D1)), (conv(A2), conv(D2))], plan, merged=True)
        assert all(np.array_equal(a, b) for a, b in zip(m[1:], ref_m[1:]))
    from vireo_amd import _lib
    with pytest.raises(_lib.VrxError, match="strictly increasing"):  # rejected by the library, as from_merged
        sp.DevicePool([((3, 1), np.array([0, 2]), np.array([1, 1], dtype=np.int32), np.ones(2, dtype=np.int32),
                        np.ones(2, dtype=np.int32))])
    with pytest.raises(_lib.VrxError, match="out of range"):
        sp.DevicePool([((3, 1), np.array([0, 1]), np.array([3], dtype=np.int32), np.ones(1, dtype=np.int32),
                        np.ones(1, dtype=np.int32))])


@functools.lru_cache(maxsize=None)
def c1():
    AD, DP = gold.c1()
    bc = SN.barcodes_all()
    assert AD.shape[1] == len(bc) == len(set(bc))
    return AD, DP, bc


def c1_case(sp, i):
    """case i on the c1 counts -> (samples, plan, wanted AD, wanted DP) from the committed cell_info.tsv"""
    AD, DP, bc = c1()
    how, n_cell, minor, seed, rate, suffix = SN.CASES[i]
    pool, origin, sid = SN.cell_info(i)
    col = {x: k for k, x in enumerate(bc)}
    cols = np.array([col[x] for x in origin])
    pooled, sources, truth = SN.plan_of(pool, sid)
    P = SN.pool_matrix(sources, len(pool))
    cuts = SN.split_columns(len(bc), how)
    samples = [(AD[:, c], DP[:, c]) for c in cuts]
    return samples, SN.split(bc, how), pooled, truth, (AD[:, cols] @ P).tocsc(), (DP[:, cols] @ P).tocsc()


@pytest.mark.parametrize("i", range(len(SN.CASES)))
def test_c1_counts_pooled_by_the_reference_plans(sp, i):
    how, n_cell, minor, seed, rate, suffix = SN.CASES[i]
    samples, barcodes, pooled, truth, wantA, wantD = c1_case(sp, i)
    if suffix:
        keep = [list(b) for b in barcodes]
        res = sp.synth_pool(samples, barcodes, n_cell=n_cell, minor_sample=minor, doublet_rate=rate, seed=seed)
        assert barcodes == keep
        gotA, gotD = res["AD"], res["DP"]
        assert res["barcodes"].tolist() == pooled and res["truth"].tolist() == truth
        pool, origin, sid = SN.cell_info(i)
        assert res["cell_info"] == list(zip(pool, origin, sid)) and res["plan"].n_pool == len(pooled)
    else:
        assert n_cell is None
        out = sp.pool_barcodes(barcodes, None, rate, sample_suffix=False, seed=seed)
        plan = sp.pool_plan(barcodes, out)
        assert plan.barcodes.tolist() == pooled
        gotA, gotD = sp.pool_counts(samples, plan)
    for got, want in ((gotA, wantA), (gotD, wantD)):
        assert got.shape == want.shape and (got != want).nnz == 0 and canonical(got) and not np.any(got.data == 0)


def test_vireo_wrap_on_the_pooled_counts(sp):
    import vireo_amd
    from vireo_amd import DeviceCounts
    samples, barcodes, pooled, truth, wantA, wantD = c1_case(sp, 0)
    how, n_cell, minor, seed, rate, suffix = SN.CASES[0]
    res = sp.synth_pool(samples, barcodes, n_cell=n_cell, minor_sample=minor, doublet_rate=rate, seed=seed)
    plan = res["plan"]
    bin_ = sp.sample_barcodes([list(b) for b in barcodes], n_cell, minor, seed)
    picked = []
    for (A, D), full, keep in zip(samples, barcodes, bin_):
        c = np.array([full.index(x) for x in keep])
        picked.append((A[:, c], D[:, c]))
    merged = sp.pool_counts(picked, plan, merged=True)
    counts = DeviceCounts.from_merged(*merged)
    kw = dict(n_donor=3, n_init=2, random_seed=4)
    dev = vireo_amd.vireo_wrap(counts, None, **kw)
    wantA.eliminate_zeros()
    ref = vireo_amd.vireo_wrap(wantA, wantD, **kw)
    assert sorted(dev) == sorted(ref)
    for k in ref:
        if isinstance(ref[k], np.ndarray):
            assert np.array_equal(dev[k], ref[k], equal_nan=True), k
    counts.close()


def test_command_round_trip_and_differing_variants(sp, tmp_path):
    from vireo_amd.io_utils import read_cellSNP
    from vireo_amd.synth import donor_workload, write_cellsnp_folder
    n_var = 400
    dirs, mats = [], []
    for k, m in enumerate((60, 45, 52)):
        w = donor_workload(n_var, m, 3, 0.08, seed=20 + k)
        d = str(tmp_path / ("s%d" % k))
        write_cellsnp_folder(w, d)
        dirs.append(d)
        mats.append((csc_matrix((w["ad"].astype(np.int64), w["rowidx"], w["colptr"]), shape=w["shape"]),
                     csc_matrix((w["dp"].astype(np.int64), w["rowidx"], w["colptr"]), shape=w["shape"])))
    out = str(tmp_path / "pool")
    cmd = [sys.executable, "-m", "vireo_amd.synth_pool", "-c", ",".join(dirs), "-o", out, "-d", "0.3", "--nCELL", "40",
           "--minorSAMPLE", "0.5", "--randomSEED", "9"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "[synth_pool]" in r.stdout and "RuntimeWarning" not in r.stderr
    pool, origin, sid = SN.read_cell_info(os.path.join(out, "cell_info.tsv"))
    assert len(pool) == 20 + 40 + 40 and sid == ["1"] * 20 + ["2"] * 40 + ["3"] * 40
    pooled, sources, truth = SN.plan_of(pool, sid)
    assert "doublet" in truth and max(len(s) for s in sources) == 2
    P = SN.pool_matrix(sources, len(pool))
    cols = [int(x[4:11]) for x in origin]                             # CELL0000012-1 is column 12 of its sample
    A_src = hstack([mats[int(s) - 1][0][:, [c]] for s, c in zip(sid, cols)], format="csc")
    D_src = hstack([mats[int(s) - 1][1][:, [c]] for s, c in zip(sid, cols)], format="csc")
    dat = read_cellSNP(out)
    assert dat["samples"].tolist() == pooled
    with open(os.path.join(out, "barcodes_pool.tsv")) as f, open(os.path.join(out, "cellSNP.samples.tsv")) as g:
        assert f.read() == g.read() == "".join(x + "\n" for x in pooled)
    for got, want in ((dat["AD"], (A_src @ P).tocsc()), (dat["DP"], (D_src @ P).tocsc())):
        want.eliminate_zeros()
        assert got.shape == want.shape and (got != want).nnz == 0 and got.nnz == want.nnz
    with open(os.path.join(out, "cellSNP.base.vcf.gz"), "rb") as f, \
            open(os.path.join(dirs[0], "cellSNP.base.vcf.gz"), "rb") as g:
        assert f.read() == g.read()
    # a folder whose variant list differs in one ALT allele
    other = str(tmp_path / "other")
    shutil.copytree(dirs[1], other)
    with gzip.open(os.path.join(dirs[1], "cellSNP.base.vcf.gz"), "rt") as f:
        text = f.read().split("\n")
    assert text[9].split("\t")[4] == "G"
    text[9] = text[9].replace("\tA\tG\t", "\tA\tT\t")
    with gzip.open(os.path.join(other, "cellSNP.base.vcf.gz"), "wt") as f:
        f.write("\n".join(text))
    out2 = str(tmp_path / "pool2")
    r = subprocess.run([sys.executable, "-m", "vireo_amd.synth_pool", "-c", ",".join([dirs[0], other]), "-o", out2],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "same variants" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])
    assert not os.path.exists(os.path.join(out2, "cellSNP.tag.AD.mtx"))
