"""Ambient-RNA estimation on the MI355X (predit_ambient, variant_ELBO_gain, vireo_wrap(check_ambient=True),
``vireo --callAmbientRNAs``) against the reference's fixtures (tests/golden/make_ambient_golden.py) and,
where the reference cannot run, the NumPy restatement tests/ambient_np.py."""
import os
import types

import numpy as np
import pytest

from tests import ambient_np as A
from tests import gold

pytestmark = pytest.mark.gpu
CLI = os.path.join(gold.GOLD, "cli")


def _vobj(g):
    return types.SimpleNamespace(ID_prob=g["ID_prob"], GT_prob=g["GT_prob"], beta_mu=g["beta_mu"],
                                 beta_sum=g["beta_sum"], n_donor=g["ID_prob"].shape[1])


def _run(g, AD, DP, counts=None):
    from vireo_amd import predit_ambient
    np.random.seed(int(g["seed"]))
    if counts is not None:
        return predit_ambient(_vobj(g), counts, None, nproc=1)
    return predit_ambient(_vobj(g), AD, DP, nproc=1)


def _close(psi, var, llr, want_psi, want_var, want_llr):
    assert np.array_equal(np.isnan(psi), np.isnan(want_psi))
    assert np.array_equal(np.isnan(llr), np.isnan(want_llr))
    np.testing.assert_allclose(psi, want_psi, rtol=0, atol=1e-12)
    np.testing.assert_allclose(var, want_var, rtol=1e-10)
    np.testing.assert_allclose(llr, want_llr, rtol=0, atol=1e-9)


def test_elbo_gain_matches_reference():
    from vireo_amd import variant_ELBO_gain
    g = gold.load("c1_ambient_step")
    AD, DP = gold.c1()
    gain = variant_ELBO_gain(g["ID_prob"], AD, DP)
    np.testing.assert_allclose(gain, g["gain"], rtol=1e-12, atol=1e-9)
    assert np.array_equal(gain >= g["threshold"], g["selected"])


def test_step_matches_fixture_a(capsys):
    from vireo_amd.vireo_doublet import LAST_AMBIENT
    g = gold.load("c1_ambient_step")
    AD, DP = gold.c1()
    psi, var, llr = _run(g, AD, DP)
    out = capsys.readouterr().out
    assert ("[vireo] %d out %d SNPs selected for ambient RNA detection: ELBO_gain > %.1f"
            % (g["selected"].sum(), len(g["selected"]), g["threshold"])) in out
    assert "[vireo] Ambient RNA time:" in out
    _close(psi, var, llr, g["psi"], g["var"], g["llr"])
    # iteration counts: those of the restatement from the same inits
    np.random.seed(int(g["seed"]))
    psi0 = np.random.dirichlet([1] * psi.shape[1], size=psi.shape[0])
    it = A.predict(A.theta_of(g["GT_prob"], g["beta_mu"]), g["selected"], AD, DP, psi0)[3]
    assert np.array_equal(LAST_AMBIENT["n_iter"], it)


def test_edge_fixture_nan_rows_and_one_entry_cell():
    g = gold.load("c1_ambient_edge")
    AD, DP = gold.unpack(g)
    psi, var, llr = _run(g, AD, DP)
    assert np.isnan(psi[:5]).all() and np.isnan(var[:5]).all() and np.isnan(llr[:5]).all()
    _close(psi, var, llr, g["psi"], g["var"], g["llr"])


@pytest.mark.parametrize("name,kw", [
    ("c1_ambient_wrap_seed2", dict(n_donor=4, n_init=2, random_seed=2)),
    ("c1_ambient_wrap_extra1", dict(n_donor=3, n_init=2, random_seed=2, n_extra_donor=1)),
    ("c1_ambient_wrap_prior", dict(n_donor=4, n_init=2, random_seed=2, GT_prior=True)),
])
def test_wrap_matches_fixture_b(name, kw, capsys):
    from vireo_amd import vireo_wrap
    g = gold.load(name)
    if kw.get("GT_prior") is True:
        kw = dict(kw, GT_prior=g["GT_prior"])
    AD, DP = gold.c1()
    rv = vireo_wrap(AD, DP, check_ambient=True, nproc=1, **kw)
    capsys.readouterr()
    np.testing.assert_allclose(rv["ID_prob"], g["ID_prob"], rtol=1e-6, atol=1e-8)
    _close(rv["ambient_Psi"], rv["Psi_var"], rv["Psi_LLRatio"], g["ambient_Psi"], g["Psi_var"],
           g["Psi_LLRatio"])


@pytest.mark.parametrize("mode,args", [
    ("ambient_mode1", ["-c", "cellSNP_mat", "-N", "4", "-M", "2"]),
    ("ambient_mode2", ["-c", "cells.cellSNP.vcf.gz", "-d", "donors.cellSNP.vcf.gz", "-N", "4"]),
])
def test_cli_call_ambient_rnas(mode, args, tmp_path, capsys):
    from vireo_amd.vireo import main
    data = os.path.join(gold.GOLD, "data")
    args = [os.path.join(data, a) if a.startswith(("cell", "donors")) else a for a in args]
    out = str(tmp_path / mode)
    main(args + ["-o", out, "--randSeed", "2", "--noPlot", "--callAmbientRNAs"])
    capsys.readouterr()
    ref = os.path.join(CLI, mode)
    got = [ln.split("\t") for ln in open(out + "/prop_ambient.tsv").read().splitlines()]
    want = [ln.split("\t") for ln in open(ref + "/prop_ambient.tsv").read().splitlines()]
    assert got[0] == want[0] and [r[0] for r in got] == [r[0] for r in want]
    for gr, wr in zip(got[1:], want[1:]):
        for x, y in zip(gr[1:-1], wr[1:-1]):
            x, y = float(x), float(y)
            assert (np.isnan(x) and np.isnan(y)) or abs(x - y) <= 1e-4 * max(abs(x), abs(y)) + 1e-300, (gr, wr)
        x, y = float(gr[-1]), float(wr[-1])
        assert (np.isnan(x) and np.isnan(y)) or abs(x - y) <= max(1e-4 * abs(y), 0.01 + 1e-9), (gr, wr)
    for f in ("donor_ids.tsv", "summary.tsv", "_log.txt"):
        assert open(os.path.join(out, f)).read() == open(os.path.join(ref, f)).read(), f
    import gzip
    for f in ("prob_singlet.tsv.gz", "prob_doublet.tsv.gz"):
        assert gzip.open(os.path.join(out, f)).read() == gzip.open(os.path.join(ref, f)).read(), f


def test_reproducible_and_same_on_every_build_route(monkeypatch):
    """the compaction reads every cell's entries from the problem's cell orientation: the gather-sized
    default build, the host builder, the device builder and the device builder with balanced slabs (several
    slabs per orientation here) give the same bits, and so do two runs on one problem"""
    from oracle import vireo_oracle as O
    from vireo_amd import predit_ambient
    from vireo_amd.counts import DeviceCounts, merge_counts
    AD, DP = O.synth_donor(2600, 2300, 6, 0.03, seed=3)
    merged = merge_counts(AD, DP)
    rng = np.random.default_rng(0)
    vobj = types.SimpleNamespace(ID_prob=rng.dirichlet(np.ones(6) * 0.3, 2300),
                                 GT_prob=rng.dirichlet(np.ones(3) * 0.3, (2600, 6)),
                                 beta_mu=np.array([[0.01, 0.5, 0.99]]), n_donor=6)
    monkeypatch.setenv("VIREO_LDS_SPLIT_X10", "60")
    results = {}
    for route, build, lds, balance in [("default", None, None, False), ("default_again", None, None, False),
                                       ("host", "host", None, False), ("device", "device", "1", False),
                                       ("device_balanced", "device", "1", True)]:
        for name, val in (("VIREO_BUILD", build), ("VIREO_LDS", lds)):
            if val is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, val)
        counts = DeviceCounts.from_merged(*merged, balance=balance)
        info = counts.build_info()
        assert info["device_built"] == (build == "device"), (route, info)
        assert info["balanced_cell"] == balance, (route, info)
        np.random.seed(4)
        results[route] = predit_ambient(vobj, counts, None)
        counts.close()
    base = results["default"]
    for route, res in results.items():
        for x, y in zip(res, base):
            assert np.array_equal(x, y, equal_nan=True), route
    sel = A.elbo_gain(vobj.ID_prob, AD, DP) >= np.sqrt(2300) / 3.0
    np.random.seed(4)
    psi0 = np.random.dirichlet([1] * 6, size=2300)
    cells = range(0, 2300, 37)
    p, v, l, it = A.predict(A.theta_of(vobj.GT_prob, vobj.beta_mu), sel, AD, DP, psi0, cells=cells)
    _close(base[0][cells], base[1][cells], base[2][cells], p, v, l)


def _planted_model(w, K, soft=0.98):
    GT = np.full((w["GT"].shape[0], K, 3), (1 - soft) / 2)
    np.put_along_axis(GT, w["GT"][:, :, None], soft, axis=2)
    ID = np.full((len(w["z"]), K), (1 - soft) / (K - 1))
    ID[np.arange(len(w["z"])), w["z"]] = soft
    return types.SimpleNamespace(ID_prob=ID, GT_prob=GT, beta_mu=np.array([[0.01, 0.5, 0.99]]),
                                 n_donor=K)


def test_c3_scale_sampled_cells_match_restatement(capsys):
    from scipy.sparse import csc_matrix
    from vireo_amd import predit_ambient, synth
    from vireo_amd.counts import DeviceCounts
    from vireo_amd.vireo_doublet import LAST_AMBIENT
    N, M, K, dens = synth.CONFIGS["c3"]
    w = synth.donor_workload(N, M, K, dens, seed=0)
    counts = DeviceCounts.from_merged(w["shape"], w["colptr"], w["rowidx"], w["ad"], w["dp"])
    vobj = _planted_model(w, K)
    np.random.seed(5)
    psi, var, llr = predit_ambient(vobj, counts, None)
    capsys.readouterr()
    n_iter = LAST_AMBIENT["n_iter"].copy()
    sel = np.zeros(N, bool)
    AD = csc_matrix((w["ad"], w["rowidx"], w["colptr"]), shape=w["shape"])
    DP = csc_matrix((w["dp"], w["rowidx"], w["colptr"]), shape=w["shape"])
    gain = A.elbo_gain(vobj.ID_prob, AD, DP)
    sel = gain >= np.sqrt(M) / 3.0
    assert sel.sum() == LAST_AMBIENT["n_selected"]
    np.random.seed(5)
    psi0 = np.random.dirichlet([1] * K, size=M)
    cells = np.random.default_rng(1).choice(M, 256, replace=False)
    p, v, l, it = A.predict(A.theta_of(vobj.GT_prob, vobj.beta_mu), sel, AD, DP, psi0, cells=cells)
    np.testing.assert_allclose(psi[cells], p, rtol=0, atol=1e-12)
    np.testing.assert_allclose(var[cells], v, rtol=1e-10)
    np.testing.assert_allclose(llr[cells], l, rtol=0, atol=1e-9)
    assert np.array_equal(n_iter[cells], it)


def test_recovers_a_planted_two_donor_mixture():
    """cells whose reads come from donor z1 and, with probability f, from donor z2: psi[z2] ~ f"""
    from vireo_amd import predit_ambient
    from vireo_amd.counts import DeviceCounts
    rng = np.random.default_rng(3)
    N, M, K, f = 3000, 200, 4, 0.2
    GT = rng.integers(0, 3, (N, K))
    z1 = rng.integers(0, K, M)
    z2 = (z1 + 1 + rng.integers(0, K - 1, M)) % K
    theta = np.array([0.01, 0.5, 0.99])
    colptr, rows, ads, dps = [0], [], [], []
    for c in range(M):
        r = np.sort(rng.choice(N, 600, replace=False))
        dp = 1 + rng.poisson(2.0, r.size)
        from_2 = rng.random((r.size, dp.max())) < f
        ad = np.zeros(r.size, np.int64)
        for j in range(r.size):
            src = np.where(from_2[j, :dp[j]], z2[c], z1[c])
            ad[j] = (rng.random(dp[j]) < theta[GT[r[j], src]]).sum()
        rows.append(r)
        ads.append(ad)
        dps.append(dp)
        colptr.append(colptr[-1] + r.size)
    counts = DeviceCounts.from_merged((N, M), np.array(colptr), np.concatenate(rows).astype(np.int32),
                                      np.concatenate(ads).astype(np.int32), np.concatenate(dps).astype(np.int32))
    vobj = _planted_model(dict(GT=GT, z=z1), K, soft=0.999)
    np.random.seed(0)
    psi, var, llr = predit_ambient(vobj, counts, None, min_ELBO_gain=0.0)
    est = psi[np.arange(M), z2]
    assert abs(np.median(est) - f) < 0.03, np.median(est)
    assert np.all(psi[np.arange(M), z1] > 0.6)
    assert np.all(np.isfinite(var)) and np.all(var > 0)
