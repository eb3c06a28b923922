"""Plain restatements for the synthetic-pool tests: the fixture cases (shared with
tests/golden/make_synthpool_golden.py), the pool plan and its truth labels in a few lines of Python, the 0/1
source x pooled matrix, and get_confusion's double loop."""
import functools
import json
import os

import numpy as np
from scipy.sparse import csc_matrix

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "synth_pool")

# (split, n_cell, minor_sample, seed, doublet_rate, sample_suffix)
CASES = [
    ("3", 200, 0.5, 3, 0.1, True),
    ("3", None, 1.0, 1, None, True),
    ("3", 250, 1.0, 7, 0.0, True),        # 750 sources -> 748 pooled: collisions without doublets
    ("3", 100, 0.25, 0, 1.0, True),
    ("3", 90, 0.25, 4, 0.2, True),        # round(22.5) = 22
    ("3", None, 1.0, 8, 0.25, False),
    ("11", 60, 1.0, 2, 0.15, True),       # two-digit suffixes
    ("11", None, 1.0, 6, None, True),
]


@functools.lru_cache(maxsize=None)
def packed():
    """files.npz: the reference's text files as bytes, keys barcodes_in, case<i>_barcodes_pool, case<i>_cell_info"""
    with np.load(os.path.join(GOLD, "files.npz")) as z:
        return {k: z[k].tobytes() for k in z.files if not k.startswith("conf_")}


def confusion():
    """the get_confusion fixture: ids1, ids2 and the reference's mat, uniq1, uniq2"""
    with np.load(os.path.join(GOLD, "files.npz")) as z:
        return {k[5:]: z[k] for k in z.files if k.startswith("conf_")}


def barcodes_all():
    return [x.rstrip() for x in packed()["barcodes_in"].decode().splitlines()]


def split(bc, how):
    """the samples of a case: "3" = contiguous 300 / 300 / rest, "11" = bc[i::11]"""
    if how == "3":
        return [list(bc[:300]), list(bc[300:600]), list(bc[600:])]
    return [list(bc[i::11]) for i in range(11)]


def split_columns(n, how):
    """the column numbers of the same split"""
    return [np.array(s, dtype=np.int64) for s in split(list(range(n)), how)]


def cases_json():
    with open(os.path.join(GOLD, "cases.json")) as f:
        return json.load(f)


def parse_cell_info(text):
    """cell_info.tsv -> (CB_pool, CB_origin, Sample_id) string lists, rows in file order"""
    lines = text.split("\n")
    assert lines[0] == "CB_pool\tCB_origin\tSample_id" and lines[-1] == ""
    rows = [ln.split("\t") for ln in lines[1:-1]]
    return [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]


def read_cell_info(path):
    with open(path) as f:
        return parse_cell_info(f.read())


def cell_info(i):
    """the committed cell_info.tsv of case i"""
    return parse_cell_info(packed()["case%d_cell_info" % i].decode())


def plan_of(pool_names, sample_ids):
    """pool_names / sample_ids per source cell in cell_info.tsv row order -> (pooled names sorted, the list of
    source cells of every pooled cell, truth labels)"""
    groups = {}
    for s, name in enumerate(pool_names):
        groups.setdefault(name, []).append(s)
    names = sorted(groups)
    assert names == np.unique(pool_names).tolist()
    sources = [groups[n] for n in names]
    truth = []
    for src in sources:
        ids = {sample_ids[s] for s in src}
        truth.append(str(sample_ids[src[0]]) if len(ids) == 1 else "doublet")
    return names, sources, truth


def pool_matrix(sources, n_src):
    """0/1 int64 CSC (source cells x pooled cells)"""
    rows = np.array([s for src in sources for s in src], dtype=np.int64)
    cols = np.array([j for j, src in enumerate(sources) for _ in src], dtype=np.int64)
    return csc_matrix((np.ones(rows.size, dtype=np.int64), (rows, cols)), shape=(n_src, len(sources)))


def confusion_loops(ids1, ids2):
    """get_confusion as the reference writes it: one pass per pair of ids"""
    ids1, ids2 = np.array(ids1), np.array(ids2)
    u1, u2 = np.unique(ids1), np.unique(ids2)
    mat = np.zeros((len(u1), len(u2)), dtype=int)
    for i, a in enumerate(u1):
        for j, b in enumerate(u2):
            mat[i, j] = np.sum((ids1 == a) * (ids2 == b))
    return mat, u1, u2
