"""Stop-rule fixture from the REAL reference's own loops (build container only, /root/reference):

    python tests/golden/make_stop_golden.py

  stop_rule.npz   the planted traces of tests/stop_np.planted_cases and, per trace and per loop, what
                  Vireo._fit_VB and BinomMixtureVB._fit_BV (verbose=True) do with it: the length of the ELBO[:it]
                  they return and the text they print.  The models are tiny, their update methods are stubbed out,
                  and get_ELBO reads the next planted value -- the loop, its zero-initialised ELBO array, its
                  comparisons and its prints are the reference's.

Numeric arrays only (the printed text as bytes).  Follows make_varmix_golden.py."""
import contextlib
import io
import os
import sys

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import vireoSNP                                                   # noqa: E402
from vireoSNP import BinomMixtureVB, Vireo                        # noqa: E402
from tests import stop_np as S                                    # noqa: E402


class Planted:
    def __init__(self, trace):
        self.trace, self.at = trace, 0

    def __call__(self, *a, **k):
        v = self.trace[self.at]
        self.at += 1
        return v


def nothing(*a, **k):
    return None


def run_vireo(trace, mn, mx, eps):
    m = Vireo(n_cell=2, n_var=2, n_donor=2)
    m.update_theta_size = m.update_GT_prob = m.update_ID_prob = nothing
    m.get_ELBO = Planted(trace)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), np.errstate(all="ignore"):
        kept = m._fit_VB(None, None, max_iter=mx, min_iter=mn, epsilon_conv=eps, verbose=True)
    return kept, m.get_ELBO.at, buf.getvalue()


def run_bmm(trace, mn, mx, eps):
    m = BinomMixtureVB(n_cell=2, n_var=2, n_donor=2)
    m.update_theta_size = m.get_E_logLik = m.update_ID_prob = nothing
    m.get_ELBO = Planted(trace)
    m.ELBO_iters = np.array([])
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), np.errstate(all="ignore"):
        m._fit_BV(None, None, max_iter=mx, min_iter=mn, epsilon_conv=eps, verbose=True)
    return m.ELBO_iters, m.get_ELBO.at, buf.getvalue()


def main():
    assert vireoSNP.__version__ == "0.5.9", vireoSNP.__version__
    cases = S.planted_cases()
    n = len(cases)
    trace = np.full((n, S.CASE_LEN), np.nan)
    rule_i = np.zeros((n, 2), dtype=np.int32)
    eps = np.zeros(n)
    out = dict()
    for c, (tr, mn, mx, e) in enumerate(cases):
        trace[c, :mx] = tr
        rule_i[c] = (mn, mx)
        eps[c] = e
    for name, run in (("vireo", run_vireo), ("bmm", run_bmm)):
        kept_n = np.zeros(n, dtype=np.int32)
        computed = np.zeros(n, dtype=np.int32)
        text, off = bytearray(), [0]
        for c, (tr, mn, mx, e) in enumerate(cases):
            kept, calls, printed = run(tr, mn, mx, e)
            assert S.same_bits(kept, tr[:len(kept)])
            kept_n[c], computed[c] = len(kept), calls
            text += printed.encode()
            off.append(len(text))
        out.update({"kept_" + name: kept_n, "computed_" + name: computed,
                    "text_" + name: np.frombuffer(bytes(text), dtype=np.uint8), "text_off_" + name: np.array(off)})
        print("%s: %d cases, %d warning bytes, kept 0..%d" % (name, n, len(text), kept_n.max()))
    differ = int(np.sum((out["kept_vireo"] != out["kept_bmm"]) | (out["computed_vireo"] != out["computed_bmm"])))
    print("cases on which the two loops differ in length: %d" % differ)
    path = os.path.join(HERE, "stop_rule.npz")
    np.savez_compressed(path, trace=trace, rule_i=rule_i, eps=eps, **out)
    print("stop_rule %.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
