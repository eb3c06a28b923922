"""Small helpers of vireoSNP/utils/base_utils.py."""
import numpy as np


def get_confusion(ids1, ids2):
    """Confusion matrix of two annotations of the same samples (base_utils.py:3-31)
    -> (confuse_mat, ids1_uniq, ids2_uniq): confuse_mat[i, j] = how many samples have ids1 == ids1_uniq[i] and
    ids2 == ids2_uniq[j], the unique ids sorted as ``np.unique`` sorts them.  The reference counts every (i, j)
    pair with a pass of its own; here each sample is numbered once (``return_inverse``) and the pairs are
    counted by one ``bincount``.  Annotations of unequal length are a ValueError."""
    ids1, ids2 = np.asarray(ids1).reshape(-1), np.asarray(ids2).reshape(-1)
    if ids1.size != ids2.size:
        raise ValueError("get_confusion: ids1 has %d entries, ids2 %d" % (ids1.size, ids2.size))
    ids1_uniq, inv1 = np.unique(ids1, return_inverse=True)
    ids2_uniq, inv2 = np.unique(ids2, return_inverse=True)
    n1, n2 = len(ids1_uniq), len(ids2_uniq)
    pair = inv1.reshape(-1).astype(np.int64) * n2 + inv2.reshape(-1)
    confuse_mat = np.bincount(pair, minlength=n1 * n2).reshape(n1, n2).astype(int)
    return confuse_mat, ids1_uniq, ids2_uniq
