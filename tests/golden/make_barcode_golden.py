"""Barcode-selection fixtures from the REAL reference (build container only, /root/reference):

    python tests/golden/make_barcode_golden.py

  c1_barcode.npz            vireoSNP.utils.variant_select.variant_select on the seeded cases of
                            tests/variant_select_np.py: per case `<name>_` + every round's per-variant
                            entropies (the values barcode_entropy returned, in call order), the tie counts
                            before and after the median filter, the chosen indices, the final entropy, the
                            barcodes, the printed lines and the generator state after the call; plus the
                            numpy and scipy versions
  barcode/<run>/            the reference's GTbarcode command on tests/golden/data/donors.cellSNP.vcf.gz
                            with --noPlot: GTbarcode.tsv and the captured stdout

At least three cases must be ones on which an order-blind entropy (class sizes summed in sorted order)
changes a tie count or a choice: a fixture set that cannot tell the two apart is rejected.  Pure data:
numbers, names and printed lines only.  Follows make_match_golden.py (which it does not change)."""
import contextlib
import io
import os
import sys

import numpy as np
import scipy

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import vireoSNP                                                  # noqa: E402
from vireoSNP.utils import variant_select as RVS                 # noqa: E402
from tests import variant_select_np as V                         # noqa: E402

SEED = 0


def record_case(name):
    GT, vc = V.case_input(name)
    n_var = GT.shape[0]
    seen = []
    real = RVS.barcode_entropy

    def listening(X, y=None):
        rv = real(X, y)
        seen.append(rv[0])
        return rv

    out = io.StringIO()
    RVS.barcode_entropy = listening
    try:
        with contextlib.redirect_stdout(out):
            final, barcodes, chosen = RVS.variant_select(GT, vc, rand_seed=SEED)
    finally:
        RVS.barcode_entropy = real
    state = np.random.get_state()
    ent = np.array(seen, dtype=np.float64).reshape(-1, n_var)
    assert ent.shape[0] == len(chosen) + 1
    lines = out.getvalue().splitlines()
    tied = [int(np.sum(np.max(e) == e)) for e in ent[:-1]]
    kept = [int(line.rsplit(" ", 1)[1]) for line in lines[:len(chosen)]]
    return dict(ent=ent, tied=np.array(tied, dtype=np.int64), kept=np.array(kept, dtype=np.int64),
                chosen=np.array(chosen, dtype=np.int64), final=np.asarray(final),
                barcodes=np.asarray(barcodes, dtype=str), lines=np.asarray(lines, dtype=str),
                rng_key=state[1], rng_pos=np.int64(state[2]))


def run_command(run, args):
    from vireoSNP import GTbarcode
    d = V.barcode_run_dir(run)
    os.makedirs(d, exist_ok=True)
    tsv = os.path.join(d, "GTbarcode.tsv")
    out = io.StringIO()
    argv = sys.argv
    sys.argv = ["GTbarcode", "-i", V.BARCODE_VCF, "-o", tsv, "--noPlot"] + args
    try:
        with contextlib.redirect_stdout(out):
            GTbarcode.main()
    finally:
        sys.argv = argv
    with open(os.path.join(d, "stdout.txt"), "w") as f:
        f.write(out.getvalue())
    return out.getvalue(), open(tsv).read()


def main():
    assert vireoSNP.__version__ == "0.5.9", vireoSNP.__version__
    rec = dict(numpy_version=np.array(np.__version__), scipy_version=np.array(scipy.__version__))
    telling = []
    for name in V.CASES:
        c = record_case(name)
        GT, vc = V.case_input(name)
        blind = V.select(GT, vc, rand_seed=SEED, order_blind=True)
        differs = (list(c["tied"]) != blind["tied"] or list(c["kept"]) != blind["kept"]
                   or list(c["chosen"]) != blind["chosen"])
        if differs:
            telling.append(name)
        for key in V.FIXTURE_KEYS:
            rec["%s_%s" % (name, key)] = c[key]
        print("%-20s rounds %2d  tied %s  kept %s  chosen %s%s" % (
            name, len(c["chosen"]), list(c["tied"]), list(c["kept"]), list(c["chosen"]),
            "  [order-blind differs]" if differs else ""))
    assert len(telling) >= 3, telling
    assert set(V.ORDER_SENSITIVE) & set(telling), telling
    path = os.path.join(HERE, "c1_barcode.npz")
    np.savez_compressed(path, **rec)
    print("c1_barcode.npz %.1f KB; order-sensitive cases: %s" % (os.path.getsize(path) / 1024, telling))
    for run, args in V.BARCODE_RUNS.items():
        stdout, tsv = run_command(run, args)
        print("barcode/%s: %d variants; %s" % (run, len(tsv.splitlines()) - 1, stdout.splitlines()[:2]))


if __name__ == "__main__":
    main()
