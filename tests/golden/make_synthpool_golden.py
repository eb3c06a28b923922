"""Synthetic-pool fixtures from the REAL reference (build container only, /root/reference):

    python tests/golden/make_synthpool_golden.py

  synth_pool/files.npz           the text files as bytes: barcodes_in (the 952 barcodes of the reference's
                                 data/cellSNP_mat) and per case of tests/synthpool_np.CASES case<i>_barcodes_pool and
                                 case<i>_cell_info, barcodes_pool.tsv and cell_info.tsv as simulate/synth_pool.py
                                 wrote them
                                 and conf_ids1, conf_ids2: two label vectors (the sample tag of every c1 barcode;
                                 the donor_id column of the committed reference run tests/golden/cli/mode1_noGT) with
                                 conf_mat, conf_uniq1, conf_uniq2: what the reference's get_confusion returns for them
  synth_pool/cases.json          per case: its settings and the np.random.rand() drawn right after the reference's
                                 calls (pins the state of the generator)

The seventeen text files (11 000 lines, 400 KB) are committed as bytes in one compressed file because of their
size alone; ``tests/synthpool_np.packed()`` hands them out, and
``python -c "from tests import synthpool_np as S; print(S.packed()['case0_cell_info'].decode())"`` prints one.

simulate/synth_pool.py imports pysam and cellSNP at module level; neither is needed by sample_barcodes and
pool_barcodes, so empty stand-in modules take their place in sys.modules and the file is loaded by path.
The calls are those of its main() (:275-279).  Asserts that no pooled barcode has more than two source cells.
Pure data: names and numbers only."""
import importlib.util
import json
import os
import shutil
import sys
import tempfile
import types

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import synthpool_np as SN                              # noqa: E402


def load_reference():
    for name in ("pysam", "cellSNP", "cellSNP.utils", "cellSNP.utils.vcf_utils", "cellSNP.utils.pileup_utils"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["cellSNP.utils.vcf_utils"].load_VCF = None
    sys.modules["cellSNP.utils.pileup_utils"].check_pysam_chrom = None
    spec = importlib.util.spec_from_file_location("ref_synth_pool", os.path.join(REF, "simulate", "synth_pool.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ref = load_reference()
    os.makedirs(SN.GOLD, exist_ok=True)
    with open(os.path.join(REF, "data", "cellSNP_mat", "cellSNP.samples.tsv")) as f:
        bc = [x.rstrip() for x in f.readlines()]
    assert len(bc) == 952
    files = dict(barcodes_in="".join(x + "\n" for x in bc).encode())
    out = []
    tmp = tempfile.mkdtemp(prefix="synthpool_")
    for i, (how, n_cell, minor, seed, rate, suffix) in enumerate(SN.CASES):
        d = os.path.join(tmp, "case%d" % i)
        os.makedirs(d)
        barcodes_in = SN.split(bc, how)
        if n_cell is not None:
            barcodes_in = ref.sample_barcodes(barcodes_in, n_cell, minor, seed)
        if suffix:
            ref.pool_barcodes(barcodes_in, d, rate, seed=seed)
        else:
            ref.pool_barcodes(barcodes_in, d, rate, sample_suffix=False, seed=seed)
        nxt = float(np.random.rand())
        pool, origin, sid = SN.read_cell_info(os.path.join(d, "cell_info.tsv"))
        names, sources, truth = SN.plan_of(pool, sid)
        assert max(len(s) for s in sources) <= 2, (i, "a pooled barcode with three sources: take another seed")
        with open(os.path.join(d, "barcodes_pool.tsv")) as f:
            assert [x.rstrip() for x in f.readlines()] == names
        for name in ("barcodes_pool", "cell_info"):
            with open(os.path.join(d, name + ".tsv"), "rb") as f:
                files["case%d_%s" % (i, name)] = f.read()
        out.append(dict(split=how, n_cell=n_cell, minor_sample=minor, seed=seed, doublet_rate=rate,
                        sample_suffix=suffix, next_rand=nxt, n_src=len(pool), n_pool=len(names),
                        n_doublet=truth.count("doublet")))
        print("case %d: %d sources -> %d pooled, %d two-source cells, %d doublets" % (
            i, len(pool), len(names), sum(len(s) == 2 for s in sources), truth.count("doublet")))
    shutil.rmtree(tmp)
    with open(os.path.join(SN.GOLD, "cases.json"), "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(c) for c in out) + "\n]\n")

    sys.path.insert(0, REF)
    from vireoSNP.utils.base_utils import get_confusion
    with open(os.path.join(HERE, "cli", "mode1_noGT", "donor_ids.tsv")) as f:
        rows = [ln.split("\t") for ln in f.read().split("\n")[1:] if ln]
    assert [r[0] for r in rows] == bc
    ids1 = [x.split("-")[1] for x in bc]
    ids2 = [r[1] for r in rows]
    mat, u1, u2 = get_confusion(ids1, ids2)
    assert mat.sum() == len(bc)
    arrays = {k: np.frombuffer(v, dtype=np.uint8) for k, v in files.items()}
    arrays.update(conf_ids1=np.array(ids1), conf_ids2=np.array(ids2), conf_mat=mat, conf_uniq1=u1, conf_uniq2=u2)
    np.savez_compressed(os.path.join(SN.GOLD, "files.npz"), **arrays)
    print("confusion %s" % (mat.shape,))


if __name__ == "__main__":
    main()
