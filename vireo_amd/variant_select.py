"""Variant selection by ELBO gain, drop-in for vireoSNP/utils/variant_select.py:66-106
(``variant_ELBO_gain``).  The products AD@ID_prob, DP@ID_prob and the row sums are one variant
pass on the GPU, and the digamma / logsumexp per variant is a small kernel after it
(``vrx_problem_elbo_gain``)."""
import numpy as np

from . import _lib
from ._lib import dptr, f64
from .counts import device_counts


def variant_ELBO_gain(ID_prob, AD, DP, pseudocount=0.5):
    """ELBO gain per variant of the model with the donors of ``ID_prob`` (M2) over one donor
    (M1): logsumexp_k of s1 digamma(s1) + s2 digamma(s2) - ss digamma(ss) with s1 = AD@ID + pc,
    s2 = BD@ID + pc, ss = DP@ID + 2 pc, minus the same on the row sums.  ``AD`` may be a
    ``DeviceCounts`` (then ``DP`` is None)."""
    counts = device_counts(AD, DP)
    ID = f64(ID_prob)
    if ID.ndim != 2 or ID.shape[0] != counts.n_cell:
        raise ValueError("ID_prob must be (n_cell, n_donor) = (%d, K), got %s"
                         % (counts.n_cell, ID.shape))
    gain = np.empty(counts.n_var)
    _lib.check(_lib.lib().vrx_problem_elbo_gain(counts.handle, ID.shape[1], dptr(ID),
                                                float(pseudocount), dptr(gain)))
    return gain
