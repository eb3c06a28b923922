"""Ambient-RNA step without a GPU: the NumPy restatement (tests/ambient_np.py) against the
reference's fixtures, the batched Dirichlet draws, and the prop_ambient.tsv writer."""
import os

import numpy as np

from tests import ambient_np as A
from tests import gold

CLI = os.path.join(gold.GOLD, "cli")


def _edge_counts(g):
    return gold.unpack(g)


def test_restatement_matches_fixture_a():
    g = gold.load("c1_ambient_step")
    AD, DP = gold.c1()
    gain = A.elbo_gain(g["ID_prob"], AD, DP)
    np.testing.assert_allclose(gain, g["gain"], rtol=1e-12, atol=1e-9)
    sel = gain >= g["threshold"]
    assert np.array_equal(sel, g["selected"])
    assert g["min_margin"] > 1e-6           # the selection is not decided by rounding
    np.random.seed(int(g["seed"]))
    psi0 = np.random.dirichlet([1] * g["ID_prob"].shape[1], size=AD.shape[1])
    psi, var, llr, it = A.predict(A.theta_of(g["GT_prob"], g["beta_mu"]), sel, AD, DP, psi0)
    np.testing.assert_allclose(psi, g["psi"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(var, g["var"], rtol=1e-10)
    np.testing.assert_allclose(llr, g["llr"], rtol=0, atol=1e-9)
    assert it.min() > 20 and it.max() < 199


def test_restatement_matches_edge_fixture():
    g = gold.load("c1_ambient_edge")
    AD, DP = _edge_counts(g)
    sel = A.elbo_gain(g["ID_prob"], AD, DP) >= g["threshold"]
    assert np.array_equal(sel, g["selected"])
    np.random.seed(int(g["seed"]))
    psi0 = np.random.dirichlet([1] * g["ID_prob"].shape[1], size=AD.shape[1])
    psi, var, llr, it = A.predict(A.theta_of(g["GT_prob"], g["beta_mu"]), sel, AD, DP, psi0,
                                  cells=range(12))
    assert np.array_equal(np.isnan(psi), np.isnan(g["psi"][:12]))
    assert np.isnan(g["psi"][:5]).all() and np.isnan(g["llr"][:5]).all() and (it[:5] == 199).all()
    np.testing.assert_allclose(psi, g["psi"][:12], rtol=0, atol=1e-12)
    np.testing.assert_allclose(var, g["var"][:12], rtol=1e-10)
    np.testing.assert_allclose(llr, g["llr"][:12], rtol=0, atol=1e-9)
    assert len(A.cell_entries(AD, DP, sel, 5)[0]) == 1      # the one-entry cell


def test_batched_dirichlet_equals_sequential():
    for K, n in ((4, 952), (16, 300), (1, 5)):
        np.random.seed(123)
        seq = np.array([np.random.dirichlet([1] * K) for _ in range(n)])
        after_seq = np.random.get_state()[1].copy()
        np.random.seed(123)
        batch = np.random.dirichlet([1] * K, size=n)
        assert np.array_equal(seq, batch)
        assert np.array_equal(np.random.get_state()[1], after_seq)


def test_write_donor_id_writes_prop_ambient(tmp_path):
    """write_donor_id on a golden result dict: prop_ambient.tsv byte-identical to the reference's"""
    from vireo_amd import io_utils
    ref = open(os.path.join(CLI, "ambient_mode1", "prop_ambient.tsv")).read().splitlines()
    header = ref[0].split("\t")
    donor_names = header[1:-1]
    cells = [ln.split("\t")[0] for ln in ref[1:]]
    g = gold.load("c1_ambient_wrap_seed2")       # a result dict of the reference's (psi, LLR)
    n = len(cells)
    K = len(donor_names)
    res = dict(ID_prob=np.full((n, K), 1.0 / K), doublet_prob=np.zeros((n, K * (K - 1) // 2)),
               doublet_LLR=np.zeros(n), LB_doublet=0.0, theta_shapes=np.ones((2, 3)),
               ambient_Psi=g["ambient_Psi"], Psi_var=g["Psi_var"], Psi_LLRatio=g["Psi_LLRatio"])
    io_utils.write_donor_id(str(tmp_path), donor_names, cells, np.full(n, 20), res)
    got = open(tmp_path / "prop_ambient.tsv").read()
    want = "\t".join(header) + "\n" + "".join(
        "\t".join([cells[i]] + ["%.4e" % x for x in g["ambient_Psi"][i]] + ["%.2f" % g["Psi_LLRatio"][i]]) + "\n"
        for i in range(n))
    assert got == want
    # the same writer on the reference command's own result reproduces its file byte for byte
    psi = np.array([[float(x) for x in ln.split("\t")[1:-1]] for ln in ref[1:]])
    llr = np.array([float(ln.split("\t")[-1]) for ln in ref[1:]])
    res.update(ambient_Psi=psi, Psi_LLRatio=llr)
    io_utils.write_donor_id(str(tmp_path), donor_names, cells, np.full(n, 20), res)
    assert open(tmp_path / "prop_ambient.tsv").read() == "\n".join(ref) + "\n"


def test_writer_skips_prop_ambient_without_result(tmp_path):
    from vireo_amd import io_utils
    n, K = 3, 2
    res = dict(ID_prob=np.full((n, K), 0.5), doublet_prob=np.zeros((n, 1)), doublet_LLR=np.zeros(n),
               LB_doublet=0.0, theta_shapes=np.ones((2, 3)), ambient_Psi=None)
    io_utils.write_donor_id(str(tmp_path), ["a", "b"], ["c0", "c1", "c2"], np.full(n, 20), res)
    assert not os.path.exists(tmp_path / "prop_ambient.tsv")
