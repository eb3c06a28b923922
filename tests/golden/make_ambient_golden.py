"""Ambient-RNA fixtures from the REAL reference (build container only, /root/reference):

    python tests/golden/make_ambient_golden.py

  c1_ambient_step.npz   (a) a fitted, doublet-updated model state (ID, GT, beta) and what
                        predit_ambient(..., nproc=1) returns for it from a given seed, with the
                        ELBO gain, the selection and the smallest |gain - threshold|
  c1_ambient_wrap_*.npz (b) vireo_wrap(check_ambient=True, nproc=1) on c1
  c1_ambient_edge.npz   (c) the state of (a) on counts with empty cells (NaN rows) and a cell
                        whose only selected entry is one variant
  cli/ambient_mode*/    (d) the reference command with --callAmbientRNAs

Pure data: arrays the reference returns and the text files its command writes.  Follows
make_golden.py / make_cli_golden.py (which it does not change)."""
import contextlib
import gzip
import io
import os
import shutil
import subprocess
import sys

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
DATA = os.path.join(HERE, "data")
sys.path.insert(0, REF)

import vireoSNP                                                  # noqa: E402
from vireoSNP import Vireo, vireo_wrap                           # noqa: E402
from vireoSNP.utils.vireo_doublet import predict_doublet, predit_ambient   # noqa: E402
from vireoSNP.utils.variant_select import variant_ELBO_gain      # noqa: E402
from scipy.io import mmread                                      # noqa: E402
from scipy.sparse import csc_matrix                              # noqa: E402


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def save(name, **arrs):
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **arrs)
    print("%-28s %8.1f KB" % (name, os.path.getsize(path) / 1024))


def gain_record(ID_prob, AD, DP):
    gain = np.asarray(variant_ELBO_gain(ID_prob, AD, DP)).ravel()
    thr = np.sqrt(AD.shape[1]) / 3.0
    return dict(gain=gain, selected=gain >= thr, threshold=np.float64(thr),
                min_margin=np.float64(np.min(np.abs(gain - thr))))


def step_case(name, vobj, AD, DP, seed, **extra):
    rec = gain_record(vobj.ID_prob, AD, DP)
    np.random.seed(seed)
    psi, var, llr = quiet(predit_ambient, vobj, AD, DP, nproc=1)
    save(name, ID_prob=vobj.ID_prob, GT_prob=vobj.GT_prob, beta_mu=vobj.beta_mu,
         beta_sum=vobj.beta_sum, seed=np.int64(seed), psi=psi, var=var, llr=llr, **rec, **extra)


def main():
    assert vireoSNP.__version__ == "0.5.9", vireoSNP.__version__
    AD = mmread(REF + "/data/cellSNP_mat/cellSNP.tag.AD.mtx").tocsc()
    DP = mmread(REF + "/data/cellSNP_mat/cellSNP.tag.DP.mtx").tocsc()
    N, M = AD.shape

    # ---- (a) the step alone, on a fitted and doublet-updated model -------------------------
    np.random.seed(2)
    m = Vireo(n_var=N, n_cell=M, n_donor=4)
    quiet(m.fit, AD, DP, min_iter=5, verbose=False)
    quiet(predict_doublet, m, AD, DP)
    step_case("c1_ambient_step", m, AD, DP, seed=7)

    # ---- (c) edge cells: five empty cells, one cell with a single selected entry ----------
    ADl, DPl = AD.tolil(copy=True), DP.tolil(copy=True)
    for c in range(5):
        ADl[:, c] = 0
        DPl[:, c] = 0
    eAD, eDP = csc_matrix(ADl), csc_matrix(DPl)
    sel = gain_record(m.ID_prob, eAD, eDP)["selected"]
    v = int(np.flatnonzero(sel & (np.asarray(eDP[:, 5].todense()).ravel() > 0))[0]) \
        if np.any(sel & (np.asarray(eDP[:, 5].todense()).ravel() > 0)) else int(np.flatnonzero(sel)[0])
    ADl, DPl = eAD.tolil(), eDP.tolil()
    for r in np.flatnonzero(sel):            # cell 5 keeps one selected entry (a = 1, d = 3)
        ADl[int(r), 5] = 0
        DPl[int(r), 5] = 0
    ADl[v, 5], DPl[v, 5] = 1, 3
    eAD, eDP = csc_matrix(ADl), csc_matrix(DPl)
    eAD.eliminate_zeros()
    eDP.eliminate_zeros()
    eAD.sort_indices()
    eDP.sort_indices()
    step_case("c1_ambient_edge", m, eAD, eDP, seed=11,
              AD_indptr=eAD.indptr.astype(np.int64), AD_indices=eAD.indices.astype(np.int32),
              AD_data=eAD.data.astype(np.int64), DP_indptr=eDP.indptr.astype(np.int64),
              DP_indices=eDP.indices.astype(np.int32), DP_data=eDP.data.astype(np.int64),
              shape=np.array(eDP.shape, np.int64), one_entry_variant=np.int64(v))

    # ---- (b) the whole wrapper ------------------------------------------------------------
    def wrap_case(name, **kw):
        rv = quiet(vireo_wrap, AD, DP, nproc=1, check_ambient=True, **kw)
        save(name, ID_prob=rv["ID_prob"], ambient_Psi=rv["ambient_Psi"], Psi_var=rv["Psi_var"],
             Psi_LLRatio=rv["Psi_LLRatio"], LB_doublet=np.float64(rv["LB_doublet"]),
             **{k: v for k, v in kw.items() if isinstance(v, np.ndarray)})
    wrap_case("c1_ambient_wrap_seed2", n_donor=4, n_init=2, random_seed=2)
    wrap_case("c1_ambient_wrap_extra1", n_donor=3, n_init=2, random_seed=2, n_extra_donor=1)
    # a genotype prior: one-hot genotypes of a converged fit, blurred (compresses to little)
    np.random.seed(3)
    m0 = Vireo(n_var=N, n_cell=M, n_donor=4)
    quiet(m0.fit, AD, DP, verbose=False)
    GTp = np.full(m0.GT_prob.shape, 0.05)
    np.put_along_axis(GTp, m0.GT_prob.argmax(2)[:, :, None], 0.9, axis=2)
    wrap_case("c1_ambient_wrap_prior", GT_prior=GTp, n_donor=4, n_init=2, random_seed=2)

    # ---- (d) the command --------------------------------------------------------------------
    modes = {"ambient_mode1": ["-c", DATA + "/cellSNP_mat", "-N", "4", "-M", "2"],
             "ambient_mode2": ["-c", DATA + "/cells.cellSNP.vcf.gz", "-d",
                               DATA + "/donors.cellSNP.vcf.gz", "-N", "4"]}
    for name, args in modes.items():
        tmp = "/tmp/vireo_cli_gold_" + name
        shutil.rmtree(tmp, ignore_errors=True)
        env = dict(os.environ, PYTHONPATH=REF, MPLBACKEND="Agg")
        subprocess.run([sys.executable, "-m", "vireoSNP.vireo"] + args +
                       ["-o", tmp, "--randSeed", "2", "--noPlot", "--callAmbientRNAs"],
                       env=env, check=True, stdout=subprocess.DEVNULL)
        dst = os.path.join(HERE, "cli", name)
        os.makedirs(dst, exist_ok=True)
        for f in ["donor_ids.tsv", "summary.tsv", "_log.txt", "prop_ambient.tsv"]:
            shutil.copy(os.path.join(tmp, f), os.path.join(dst, f))
        for f in ["prob_singlet.tsv.gz", "prob_doublet.tsv.gz"]:
            with gzip.open(os.path.join(tmp, f), "rt") as src, \
                    open(os.path.join(dst, f[:-3]), "w") as d:
                d.write(src.read())
            subprocess.run(["gzip", "-nf", os.path.join(dst, f[:-3])], check=True)
        print(name, sorted(os.listdir(dst)))


if __name__ == "__main__":
    main()
