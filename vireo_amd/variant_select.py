"""Variant selection, drop-in for vireoSNP/utils/variant_select.py.

``variant_ELBO_gain`` (:66-106): the products AD@ID_prob, DP@ID_prob and the row sums are one variant
pass on the GPU, and the digamma / logsumexp per variant is a small kernel after it
(``vrx_problem_elbo_gain``).

``variant_select`` (:22-62): the greedy choice of variants whose genotypes tell the samples apart.  Every
round scores all variants by the entropy of the barcodes they would give (``barcode_entropy``, :5-19) and
draws one of those tied at the maximum.  The reference decides by float equality, so the device pass
(csrc/vrx_barcode.h) reproduces its doubles bit for bit; the host keeps the class rank of every sample,
fills the small table of ``scipy.special.entr`` values the device reads instead of taking a logarithm, and
draws from NumPy's global generator exactly as the reference does."""
import ctypes as C

import numpy as np
from scipy.special import entr

from . import _lib
from ._lib import dptr, f64
from .counts import device_counts

MAX_DONORS = 128        # np.sum adds more than 128 terms by another rule
HALF_WIDTH = 32         # the table covers normalising sums within this many ulp of 1
_BITS_ONE = np.float64(1.0).view(np.int64)


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


def barcode_entropy(X, y=None):
    """Entropy (base 2) of a list of categorical barcodes, and the barcodes: ``X`` as strings, or each
    with the matching element of ``y`` appended.  Host helper with the reference's results: the class
    sizes are taken in the sorted order of the distinct barcodes, normalised twice and summed by
    ``np.sum``, as scipy.stats.entropy does."""
    if y is None:
        codes = [str(x) for x in X]
    elif len(X) != len(y):
        print("Error: X and y have different length in barcode_entropy.")
        return None, None
    else:
        codes = [str(x) + str(v) for x, v in zip(X, y)]
    sizes = np.unique(codes, return_counts=True)[1]
    p = sizes / np.sum(sizes)
    q = 1.0 * p / np.sum(p, axis=0, keepdims=True)
    return np.sum(entr(q), axis=0) / np.log(2), codes


def entr_table(n_donor, half_width=HALF_WIDTH):
    """T[j + H][c] = entr((c / n_donor) / s_j) for c = 0..n_donor, s_j the double whose bit pattern is that
    of 1.0 plus j, |j| <= H: every value the entropy of a variant can be made of while its normalising
    sum stays within H ulp of 1."""
    j = np.arange(-half_width, half_width + 1, dtype=np.int64)
    s = (_BITS_ONE + j).view(np.float64)
    p = np.arange(n_donor + 1, dtype=np.float64) / np.float64(n_donor)
    return np.ascontiguousarray(entr(p[None, :] / s[:, None]))


def _check_input(GT, var_count):
    """the limits of the device pass, before any device call: (GT uint8 [n_var][K], var_count or None)"""
    G = np.asarray(GT)
    if G.ndim != 2:
        raise ValueError("GT must be (n_var, n_donor), got shape %s" % (G.shape,))
    n_var, K = G.shape
    if n_var == 0:
        raise ValueError("GT has no variants")
    if K < 1 or K > MAX_DONORS:
        raise ValueError("variant_select: 1 <= n_donor <= %d, got %d" % (MAX_DONORS, K))
    if G.dtype == bool:
        G = G.astype(np.uint8)
    if G.dtype.kind not in "iuf":
        raise ValueError("GT must hold integer categories 0..9, got dtype %s" % G.dtype)
    if G.dtype.kind == "f" and not np.array_equal(G, np.floor(G)):     # (NaN and inf fail here too)
        raise ValueError("GT must hold integer categories 0..9: it has non-integer values")
    if G.min() < 0 or G.max() > 9:
        raise ValueError("GT must hold single-character categories 0..9, got values in [%s, %s]"
                         % (G.min(), G.max()))
    vc = None
    if var_count is not None:
        vc = np.ascontiguousarray(var_count, dtype=np.float64)
        if vc.shape != (n_var,):
            raise ValueError("var_count must have one entry per variant (%d), got shape %s" % (n_var, vc.shape))
        if not np.isfinite(vc).all():
            raise ValueError("var_count must be finite")
    return G.astype(np.uint8), vc


class BarcodeRounds(_lib.Handle):
    """The genotypes (and var_count) of one selection on the device, and the class ranks of the samples."""

    def __init__(self, GT, var_count=None, device=0):
        G, vc = _check_input(GT, var_count)
        self.n_var, self.n_donor = G.shape
        _lib.require_gpu()
        rows = np.ascontiguousarray(G.T)                       # donor-major: a wave reads neighbouring variants
        L = _lib.lib()
        super().__init__("BarcodeRounds", lambda out: L.vrx_barcode_create(
            device, self.n_var, self.n_donor, int(G.max()) + 1, rows.ctypes.data_as(C.POINTER(C.c_uint8)), dptr(vc),
            out), L.vrx_barcode_destroy)
        self.rank = np.zeros(self.n_donor, dtype=np.int64)
        self.ms = (0.0, 0.0)

    def round(self, half_width=HALF_WIDTH):
        """all variants against the current classes: (max entropy, n_tied, n_kept)"""
        order = np.argsort(self.rank, kind="stable").astype(np.int32)
        n_class = int(self.rank.max()) + 1
        bnd = np.searchsorted(self.rank[order], np.arange(n_class + 1)).astype(np.int32)
        table = entr_table(self.n_donor, half_width)
        top = C.c_double(0.0)
        counts = np.zeros(3, dtype=np.int64)
        ms = np.zeros(2)
        i32 = C.POINTER(C.c_int32)
        _lib.check(_lib.lib().vrx_barcode_round(
            self._h, order.ctypes.data_as(i32), bnd.ctypes.data_as(i32), n_class, dptr(table), half_width,
            float(np.log(2)), C.byref(top), counts.ctypes.data_as(C.POINTER(C.c_int64)), dptr(ms)))
        self.ms = (float(ms[0]), float(ms[1]))
        return np.float64(top.value), int(counts[0]), int(counts[1])

    def pick(self, r):
        """the r-th survivor of the last round in ascending variant index, and its entropy"""
        idx, ent = C.c_int64(-1), C.c_double(0.0)
        _lib.check(_lib.lib().vrx_barcode_pick(self._h, int(r), C.byref(idx), C.byref(ent)))
        return np.int64(idx.value), np.float64(ent.value)

    def choose(self, values):
        """the samples' classes once a variant with these genotypes joins the barcode: the dense rank of
        (class, value), which is the string order of the longer barcodes"""
        key = self.rank * 16 + np.asarray(values, dtype=np.int64)
        self.rank = np.unique(key, return_inverse=True)[1].astype(np.int64).reshape(-1)

    def entropies(self):
        out = np.empty(self.n_var)
        _lib.check(_lib.lib().vrx_barcode_entropies(self._h, dptr(out)))
        return out


def variant_select(GT, var_count=None, rand_seed=0):
    """Greedy choice of discriminatory variants by information gain.

    GT: (n_var, n_donor) categorical values 0..9, at most 128 samples; var_count: (n_var,) counts --
    of the variants tied at the best entropy only those at or above the median count stay in the draw.
    Returns (entropy, barcodes, chosen variant indices); (0, ['#', ...], []) when no variant splits
    anything.  Seeds and draws from NumPy's global generator like the reference."""
    rounds = BarcodeRounds(GT, var_count)
    G = np.asarray(GT)
    try:
        np.random.seed(rand_seed)
        entropy_now = 0
        variant_set = []
        barcode_set = ["#"] * rounds.n_donor
        while True:
            top, _n_tied, n_kept = rounds.round()
            if top == entropy_now:
                break
            print("Randomly select 1 more variants out %d" % n_kept)
            idx_use, entropy_now = rounds.pick(np.random.randint(n_kept))
            variant_set.append(idx_use)
            barcode_set = [b + str(g) for b, g in zip(barcode_set, G[idx_use, :])]
            rounds.choose(G[idx_use, :])
    finally:
        rounds.close()
    if entropy_now < np.log2(rounds.n_donor):
        print("Warning: variant_select can't distinguish all samples.")
    return entropy_now, barcode_set, variant_set
