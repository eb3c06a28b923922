"""vireo_amd -- MI355X-native implementation of vireoSNP's variational-EM hot path.

Same names as the reference package surface (vireoSNP/__init__.py:7-15) for the path
that is in scope: ``Vireo``, ``BinomMixtureVB``, ``vireo_wrap``, ``VireoBulk`` / ``LikRatio_test`` and the helpers they use.
Host code is plain Python/NumPy; all per-iteration arithmetic runs in hand-written HIP
kernels for gfx950 behind a ctypes C ABI (include/vireo_hip.h).  There is no CPU
fallback and no PyTorch in the compute path.
"""
__version__ = "0.2.0"

from . import bgzf
from . import vcf_utils as vcf
from . import vireo_base as base
from . import vireo_model as model
from .counts import DeviceCounts, device_counts
from .vcf_utils import load_VCF, match_SNPs, match_VCF_samples, snp_gene_match
from .io_utils import read_cellSNP, read_cellVCF, read_vartrix
from .vireo_base import (normalize, tensor_normalize, loglik_amplify, get_binom_coeff,
                         binom_coeff_sum, beta_entropy, match, optimal_match, donor_select,
                         genotype_distance, donor_match)
from .vireo_model import Vireo
from .bmm_model import BinomMixtureVB
from .vireo_doublet import predict_doublet, add_doublet_GT, add_doublet_theta, predit_ambient
from .variant_select import variant_ELBO_gain, variant_select, barcode_entropy
from .variant_mixture import variant_mixture_gain, VariantMixtures
from .gene_match import gene_counts
from .vireo_wrap import vireo_wrap
from .vireo_bulk import VireoBulk, VireoBulkCohort, LikRatio_test, BulkData, device_bulk
from .base_utils import get_confusion

_POOL = ("sample_barcodes", "pool_barcodes", "pool_plan", "PoolPlan", "pool_counts", "DevicePool")


def __getattr__(name):
    # vireo_amd.synth_pool is also a command (python -m): its names are looked up on first use, so that running
    # the command does not find its module imported already
    if name in _POOL:
        from . import synth_pool
        return getattr(synth_pool, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))


def __dir__():
    return sorted(set(globals()) | set(_POOL))


__all__ = ["__version__", "Vireo", "BinomMixtureVB", "vireo_wrap", "predict_doublet",
           "predit_ambient", "variant_ELBO_gain", "variant_select", "barcode_entropy",
           "variant_mixture_gain", "VariantMixtures", "VireoBulk", "VireoBulkCohort", "LikRatio_test", "BulkData", "device_bulk",
           "DeviceCounts", "device_counts", "load_VCF", "match_SNPs", "read_cellSNP",
           "read_cellVCF", "read_vartrix", "normalize", "tensor_normalize", "loglik_amplify", "get_binom_coeff",
           "binom_coeff_sum", "beta_entropy", "match", "optimal_match", "donor_select",
           "genotype_distance", "donor_match", "match_VCF_samples", "snp_gene_match", "gene_counts",
           "get_confusion", "vcf", "base", "model", "bgzf"] + list(_POOL)
