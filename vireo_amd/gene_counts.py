"""``gene_counts`` command: assign the SNPs of a cellSNP folder to genes and add their counts up per gene.

    python -m vireo_amd.gene_counts -c CELLSNP_DIR -g GENES_TSV -o OUT_DIR
                                    [--gaps 0,1000,10000,100000] [--maxFlag N] [--singleGene] [--geneKey gene]

GENES_TSV: tab-separated, a header line naming chrom, start, stop and the gene key.  Written to OUT_DIR:
  cellSNP.tag.AD.mtx, cellSNP.tag.DP.mtx   genes x cells
  cellSNP.samples.tsv                      copied
  genes.tsv                                the row names
  snp_gene.tsv                             one line per SNP: chrom, pos, flag, genes joined by commas
Matching and adding run on the GPU (vireo_amd.gene_match); loading and writing are host work.

As an attribute of the package, ``vireo_amd.gene_counts`` is the function of vireo_amd.gene_match; importing
this module by name keeps that true: the module is callable and forwards.
"""
import ctypes as C
import os
import shutil
import sys
import types
from optparse import OptionParser

import numpy as np

from . import _lib
from .gene_match import gene_counts, parse_genes, snp_gene_match
from .io_utils import read_cellSNP


class _CallableModule(types.ModuleType):
    def __call__(self, *args, **kwargs):
        return gene_counts(*args, **kwargs)


if __name__ != "__main__":
    sys.modules[__name__].__class__ = _CallableModule


def build_parser():
    parser = OptionParser()
    parser.add_option("--cellData", "-c", dest="cell_data", default=None, help="cellSNP output folder")
    parser.add_option("--genes", "-g", dest="genes", default=None, help="tab-separated gene table with a header")
    parser.add_option("--outDir", "-o", dest="out_dir", default=None, help="folder for the output files")
    parser.add_option("--gaps", dest="gaps", default="0,1000,10000,100000",
                      help="distances tried in turn, comma separated [default: %default]")
    parser.add_option("--maxFlag", dest="max_flag", type=int, default=None,
                      help="only SNPs matched by gap number <= this add to the counts [default: all matched]")
    parser.add_option("--singleGene", dest="single", action="store_true", default=False,
                      help="one gene per SNP also where it overlaps several")
    parser.add_option("--geneKey", dest="gene_key", default="gene", help="column of the gene names [default: %default]")
    return parser


def write_mtx(path, X):
    """X (canonical CSC without stored zeros, counts below 2^31) as MatrixMarket coordinate integer"""
    coo = X.tocoo()
    r, c, v = (np.ascontiguousarray(a, dtype=np.int32) for a in (coo.row, coo.col, coo.data))
    i32 = C.POINTER(C.c_int32)
    _lib.check(_lib.lib().vrx_mtx_write(path.encode(), X.shape[0], X.shape[1], r.size, r.ctypes.data_as(i32),
                                        c.ctypes.data_as(i32), v.ctypes.data_as(i32)))


def main(argv=None):
    parser = build_parser()
    argv = sys.argv[1:] if argv is None else argv
    (opt, _args) = parser.parse_args(argv)
    if opt.cell_data is None or opt.genes is None or opt.out_dir is None:
        print("Error: need a cellSNP folder (-c), a gene table (-g) and an output folder (-o); -h for the arguments.")
        sys.exit(1)
    gaps = [int(x) for x in opt.gaps.split(",") if x.strip() != ""]
    genes = parse_genes(opt.genes, opt.gene_key)
    dat = read_cellSNP(opt.cell_data)
    chrom, pos = dat["FixedINFO"]["CHROM"], dat["FixedINFO"]["POS"]
    gene_list, flag_list = snp_gene_match(dict(CHROM=chrom, POS=pos), genes, gene_key=opt.gene_key,
                                          multi_gene=not opt.single, gaps=gaps)
    if opt.max_flag is None:
        AD, DP, names = gene_counts(dat["AD"], dat["DP"], gene_list)
    else:
        AD, DP, names = gene_counts(dat["AD"], dat["DP"], gene_list, flag_list, opt.max_flag)
    os.makedirs(opt.out_dir, exist_ok=True)
    write_mtx(os.path.join(opt.out_dir, "cellSNP.tag.AD.mtx"), AD)
    write_mtx(os.path.join(opt.out_dir, "cellSNP.tag.DP.mtx"), DP)
    shutil.copyfile(os.path.join(opt.cell_data, "cellSNP.samples.tsv"), os.path.join(opt.out_dir, "cellSNP.samples.tsv"))
    with open(os.path.join(opt.out_dir, "genes.tsv"), "w") as f:
        f.write("".join(str(x) + "\n" for x in names))
    with open(os.path.join(opt.out_dir, "snp_gene.tsv"), "w") as f:
        f.write("chrom\tpos\tflag\tgenes\n")
        for c, p, k, g in zip(chrom, pos, flag_list, gene_list):
            f.write("%s\t%s\t%d\t%s\n" % (c, p, k, ",".join(str(x) for x in g)))
    print("[gene_counts] %d of %d SNPs matched, %d genes x %d cells, %d AD and %d DP entries"
          % (int(np.sum(np.asarray(flag_list) < len(gaps))), len(flag_list), AD.shape[0], AD.shape[1], AD.nnz, DP.nnz))


if __name__ == "__main__":
    main()
