"""``variant_gain`` command: score every variant of a cellSNP folder by ``variant_mixture_gain`` and write the
informative ones in the form the reference's clone notebooks load.

    python -m vireo_amd.variant_gain -c CELLSNP_DIR -o OUT_DIR [-K 2] [--minGain 0] [--minDP 1]
                                     [--maxIter 200] [--minIter 20] [--epsilon 0.01]

Written to OUT_DIR:
  variant_gain.tsv          one line per variant: id, n_covered, gain, elbo_one, elbo, n_iter, beta_mu_k ...,
                            size_k ...
  passed_ad.mtx, passed_dp.mtx, passed_variant_names.txt
                            the variants with gain > minGain, in input order -- the file names
                            examples/vireoSNP_clones.ipynb reads before BinomMixtureVB sees anything.
The score is the reference's VB bound of a per-variant binomial mixture against one component
(vireo_amd.variant_mixture); the numbers are not MQuad's.  Loading and writing are host work, every fit runs
on the GPU.
"""
import ctypes as C
import os
import sys
from optparse import OptionParser

import numpy as np
from scipy.sparse import csr_matrix

from . import _lib
from .io_utils import read_cellSNP
from .variant_mixture import VariantMixtures


def build_parser():
    parser = OptionParser()
    parser.add_option("--cellData", "-c", dest="cell_data", default=None, help="cellSNP output folder")
    parser.add_option("--outDir", "-o", dest="out_dir", default=None, help="folder for the output files")
    parser.add_option("--nClone", "-K", dest="n_clone", type=int, default=2,
                      help="components of the per-variant mixture, 2 ... 8 [default: %default]")
    parser.add_option("--minGain", dest="min_gain", type=float, default=0.0,
                      help="keep the variants with gain above this [default: %default]")
    parser.add_option("--minDP", dest="min_dp", type=int, default=1,
                      help="a cell covers a variant from this depth on [default: %default]")
    parser.add_option("--maxIter", dest="max_iter", type=int, default=200, help="[default: %default]")
    parser.add_option("--minIter", dest="min_iter", type=int, default=20, help="[default: %default]")
    parser.add_option("--epsilon", dest="epsilon", type=float, default=1e-2,
                      help="convergence threshold on the bound [default: %default]")
    return parser


def write_mtx(path, X):
    """X (scipy sparse, non-negative integer counts) as MatrixMarket coordinate integer, row-major"""
    X = csr_matrix(X)
    X.sum_duplicates()
    X.eliminate_zeros()
    coo = X.tocoo()
    r, c, v = (np.ascontiguousarray(a, dtype=np.int32) for a in (coo.row, coo.col, coo.data))
    i32 = C.POINTER(C.c_int32)
    _lib.check(_lib.lib().vrx_mtx_write(path.encode(), X.shape[0], X.shape[1], r.size, r.ctypes.data_as(i32),
                                        c.ctypes.data_as(i32), v.ctypes.data_as(i32)))


def main(argv=None):
    parser = build_parser()
    argv = sys.argv[1:] if argv is None else argv
    (opt, _args) = parser.parse_args(argv)
    if opt.cell_data is None or opt.out_dir is None:
        print("Error: need a cellSNP folder (-c) and an output folder (-o); -h for the arguments.")
        sys.exit(1)
    os.makedirs(opt.out_dir, exist_ok=True)
    dat = read_cellSNP(opt.cell_data)
    AD, DP = dat["AD"], dat["DP"]
    names = [str(x) for x in dat["variants"]]
    K = opt.n_clone
    vm = VariantMixtures(AD, DP, min_DP=opt.min_dp)
    try:
        fit = vm.fit(n_clone=K, max_iter=opt.max_iter, min_iter=opt.min_iter, epsilon_conv=opt.epsilon)
    finally:
        vm.close()
    gain = fit["gain"]
    with open(os.path.join(opt.out_dir, "variant_gain.tsv"), "w") as f:
        f.write("\t".join(["variant", "n_covered", "gain", "elbo_one", "elbo", "n_iter"] +
                          ["beta_mu_%d" % k for k in range(K)] + ["size_%d" % k for k in range(K)]) + "\n")
        for v, name in enumerate(names):
            f.write("\t".join([name, "%d" % fit["n_covered"][v], "%.17g" % gain[v], "%.17g" % fit["elbo_one"][v],
                               "%.17g" % fit["elbo"][v], "%d" % fit["n_iter"][v]] +
                              ["%.6g" % x for x in fit["beta_mu"][v]] + ["%.6g" % x for x in fit["size"][v]]) + "\n")
    rows = np.flatnonzero(gain > opt.min_gain)
    write_mtx(os.path.join(opt.out_dir, "passed_ad.mtx"), csr_matrix(AD)[rows])
    write_mtx(os.path.join(opt.out_dir, "passed_dp.mtx"), csr_matrix(DP)[rows])
    with open(os.path.join(opt.out_dir, "passed_variant_names.txt"), "w") as f:
        f.write("".join(names[v] + "\n" for v in rows))
    print("[variant_gain] %d of %d variants pass gain > %g (K = %d, %d covered entries, %d not converged)"
          % (rows.size, len(names), opt.min_gain, K, vm.nnz, int(np.sum((fit["warn"] & 2) != 0))))


if __name__ == "__main__":
    main()
