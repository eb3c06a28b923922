"""``GTbarcode`` command: a minimal set of variants whose genotypes tell the samples of a VCF apart.

Same options, messages and output file as the reference command (vireoSNP/GTbarcode.py:16-121, registered
as ``GTbarcode`` in setup.py):

    python -m vireo_amd.GTbarcode -i DONOR_VCF [-o OUT.tsv] [-t GT|GP|PL] [--noHomoAlt] [--randSeed S]

Loading, filtering and writing are host work; the greedy selection runs on the GPU
(vireo_amd.variant_select).  Not carried over: the barcode figure -- ``--noPlot``, ``--figSize`` and
``--figFormat`` are accepted and nothing is drawn, as in the ``vireo`` command.
"""
import os
import sys
from optparse import OptionParser, OptionGroup

import numpy as np

from . import __version__
from .variant_select import variant_select
from .vcf_utils import load_VCF, parse_donor_GPb

# The reference's option surface (GTbarcode.py:21-41): same flags, destinations, types and defaults;
# the help texts are this package's own.   (flags, dest, kind, default, help)
_MAIN_OPTIONS = [
    (("--vcfFile", "-i"), "vcf_file", None, None, "VCF file with the genotypes of the samples"),
    (("--outFile", "-o"), "out_file", None, None, "output table [default: <folder of the VCF>/GTbarcode.tsv]"),
]
_OPTIONAL = [
    (("--genoTag", "-t"), "geno_tag", None, "GT",
     "FORMAT tag holding the genotypes: GT, GP or PL [default: %default]"),
    (("--noHomoAlt",), "no_homo_alt", "flag", False, "drop variants on which a sample is homozygous ALT"),
    (("--noPlot",), "no_plot", "flag", False, "accepted; vireo_amd never draws the barcode figure"),
    (("--figSize",), "fig_size", None, "4,2", "accepted and unused (no figure) [default: %default]"),
    (("--figFormat",), "fig_format", None, "png", "accepted and unused (no figure) [default: %default]"),
    (("--randSeed",), "rand_seed", int, None,
     "seed of the draw among variants with the same information gain [default: %default]"),
]
MIN_DEPTH = 20           # keep DP > 20
MAX_OTHER = 0.05         # and OTH / DP < 0.05


def build_parser():
    parser = OptionParser()

    def declare(target, table):
        for flags, dest, kind, default, text in table:
            extra = dict(action="store_true") if kind == "flag" else ({} if kind is None else dict(type=kind))
            target.add_option(*flags, dest=dest, default=default, help=text, **extra)

    declare(parser, _MAIN_OPTIONS)
    group = OptionGroup(parser, "Optional arguments")
    declare(group, _OPTIONAL)
    parser.add_option_group(group)
    return parser


def info_value(info, key):
    """the number after the first `key` (e.g. "DP=") of an INFO string, up to the next ';'; 0 if absent"""
    at = info.find(key)
    if at < 0:
        return 0
    return float(info[at + len(key):].split(";")[0])


def variant_mask(INFO, GT_vals, no_homo_alt=False):
    """(keep, AD, DP, OTH): variants with DP > 20 and OTH / DP < 0.05 (GTbarcode.py:76-98), and with
    --noHomoAlt those on which no sample has genotype 2"""
    AD = np.array([info_value(s, "AD=") for s in INFO])
    DP = np.array([info_value(s, "DP=") for s in INFO])
    OTH = np.array([info_value(s, "OTH=") for s in INFO])
    keep = (DP > MIN_DEPTH) * (OTH / DP < MAX_OTHER)
    if no_homo_alt:
        keep *= np.max(GT_vals, axis=1) < 2
    return keep, AD, DP, OTH


def main(argv=None):
    parser = build_parser()
    argv = sys.argv[1:] if argv is None else argv
    (options, _args) = parser.parse_args(argv)
    if len(argv) == 0:
        print("Welcome to GT barcode generator; Vireo v%s!\n" % __version__)
        print("use -h or --help for help on argument.")
        sys.exit(1)
    if options.vcf_file is None:
        print("Error: need genotype data in vcf file.")
        sys.exit(1)
    vcf_file = options.vcf_file
    if options.out_file is None:
        print("Warning: no outFile provided, we use $vcfFile/GTbarcode.tsv")
        out_file = os.path.dirname(os.path.abspath(vcf_file)) + "/GTbarcode.tsv"
    else:
        out_file = options.out_file
    if not os.path.exists(os.path.dirname(out_file)):
        os.mkdir(os.path.dirname(out_file))

    tag = options.geno_tag
    vcf = load_VCF(vcf_file, sparse=False, biallelic_only=True)
    GT_vals = np.argmax(parse_donor_GPb(vcf['GenoINFO'][tag], tag), axis=2)
    var_ids = np.array(vcf["variants"])
    samples = vcf['samples']

    keep, _AD, DP, _OTH = variant_mask(vcf["FixedINFO"]["INFO"], GT_vals, options.no_homo_alt)
    var_ids, GT_vals, DP = var_ids[keep], GT_vals[keep, :], DP[keep]

    _entropy, _barcodes, chosen = variant_select(GT_vals, DP, rand_seed=options.rand_seed)
    with open(out_file, "w") as out:
        out.write("\t".join(["variants"] + samples) + "\n")
        for i in chosen:
            out.write("\t".join([var_ids[i]] + ["%d" % g for g in GT_vals[i, :]]) + "\n")


if __name__ == "__main__":
    main()
