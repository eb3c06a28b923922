"""The stop rule of the reference's fit loops, restated in NumPy float64, and the planted table every copy of it is
held to (the host and the device compile of csrc/vrx_stop.h, the fixture tests/golden/stop_rule.npz).

    X = np.zeros(max_iter)
    for it in range(max_iter):
        ...; X[it] = bound
        if it > min_iter:
            if   <decreased>:                 warn            (verdict 1, warn bit 1)
            elif it == max_iter - 1:          warn            (verdict 2, warn bit 2)
            elif X[it] - X[it - 1] < eps:     break           (verdict 3)

The loops differ in <decreased> alone: vireo_model.py:266-274 (VIREO), bmm_model.py:190-199 (BMM),
vireo_bulk.py:97-105 and vireo_doublet.py:173-181 (EM)."""
import numpy as np

VIREO, BMM, EM = 0, 1, 2
FORMS = (VIREO, BMM, EM)
FORM_NAMES = {VIREO: "vireo", BMM: "bmm", EM: "em"}
CONTINUE, WARN_DECREASED, WARN_NOT_CONVERGED, STOP = 0, 1, 2, 3
VERDICT_NAMES = ("continue", "warn-decreased", "warn-not-converged", "stop")
LINE_NOT_CONVERGED = "Warning: VB did not converge!\n"
LINE_VIREO_DECREASED = "Warning: Lower bound decreases!\n"
LINE_BMM_DECREASED = "Warning: ELBO decreases %.8f to %.8f!\n"
LINE_EM_DECREASED = "Warning: logLikelihood decreases!\n"


def _decreased(form, prev, cur):
    if form == VIREO:
        return bool(cur < prev - np.float64(1e-6))                    # vireo_model.py:267 (numerical_minimal, :256)
    if form == BMM:
        return bool(cur - prev < np.float64(-1e-6))                   # bmm_model.py:191
    return bool(cur < prev)                                           # vireo_bulk.py:98, vireo_doublet.py:174


def _verdict(form, it, min_iter, max_iter, eps, prev, cur):
    if not it > min_iter:
        return CONTINUE
    if _decreased(form, prev, cur):
        return WARN_DECREASED
    if it == max_iter - 1:
        return WARN_NOT_CONVERGED
    return STOP if bool(cur - prev < eps) else CONTINUE


def decreased(form, prev, cur):
    with np.errstate(invalid="ignore", over="ignore"):                # (inf - inf, and beyond the largest double)
        return _decreased(form, np.float64(prev), np.float64(cur))


def verdict(form, it, min_iter, max_iter, eps, prev, cur):
    """the block under ``if it > min_iter`` with X[it - 1] = prev, X[it] = cur"""
    with np.errstate(invalid="ignore", over="ignore"):
        return _verdict(form, it, min_iter, max_iter, np.float64(eps), np.float64(prev), np.float64(cur))


def prev_of(it, max_iter, trace_prev, cur):
    """X[it - 1] of X = np.zeros(max_iter) while X[it] = cur is its newest entry: Python's X[-1] at it = 0"""
    X = np.zeros(max_iter)
    if it >= 1:
        X[it - 1] = trace_prev
    X[it] = cur
    return X[it - 1]


def events(form, trace, min_iter, max_iter, eps, judge=verdict):
    """The reference's loop run over ``trace`` (the bounds an unruled run computes, at least as many as the loop
    reaches) -> (it, [(iteration, verdict, X[it - 1], X[it]) of every warning]).  X is the zero-initialised array of
    the reference, indexed as Python indexes it."""
    X = np.zeros(max_iter)
    out = []
    it = None
    eps = np.float64(eps)
    judge = _verdict if judge is verdict else judge
    with np.errstate(invalid="ignore", over="ignore"):
        for it in range(max_iter):
            X[it] = trace[it]
            v = judge(form, it, min_iter, max_iter, eps, X[it - 1], X[it])
            if v == STOP:
                break
            if v != CONTINUE:
                out.append((it, v, X[it - 1], X[it]))
    return it, out


def replay(form, trace, min_iter, max_iter, eps, judge=verdict):
    """-> (it, warn_bits, n_kept): the loop variable the reference leaves, bit 1 / bit 2 for a printed "decreased" /
    "did not converge", and the length of the X[:it] it returns"""
    it, ev = events(form, trace, min_iter, max_iter, eps, judge)
    bits = 0
    for _, v, _, _ in ev:
        bits |= 1 if v == WARN_DECREASED else 2
    return it, bits, len(np.zeros(max_iter)[:it])


def lines(form, trace, min_iter, max_iter, eps):
    """what the reference prints with verbose=True, as one string"""
    _, ev = events(form, trace, min_iter, max_iter, eps)
    out = []
    for _, v, prev, cur in ev:
        if v == WARN_NOT_CONVERGED:
            out.append(LINE_NOT_CONVERGED)
        elif form == VIREO:
            out.append(LINE_VIREO_DECREASED)
        elif form == BMM:
            out.append(LINE_BMM_DECREASED % (prev, cur))
        else:
            out.append(LINE_EM_DECREASED)
    return "".join(line + "\n" for line in out)                       # (print adds its own newline)


# ---- the planted table ---------------------------------------------------------------------------------------------
PREVS_FINITE = (-1e-3, -1.0, -3e8, -1e10, -1e15, 5.0, 0.0)
PREVS_OTHER = (np.inf, -np.inf, np.nan)
EPSILONS = (1e-2, 1e-3, 0.0, -1.0, 5e-324, np.inf, np.nan)
THRESHOLDS = (-1e-6, 0.0, 1e-2, 1e-3, -1.0, 5e-324)      # the decreased tests (VIREO / BMM, EM), then each finite eps
REACH = 4              # ulps on either side of fl(prev + threshold): the flip of either form lies within 1 of it
# (it, min_iter, max_iter): it = min_iter and min_iter + 1, the last iteration, and it = 0 under min_iter = -1
POSITIONS = ((5, 5, 200), (6, 5, 200), (7, 5, 8), (0, -1, 1), (0, -1, 2), (0, -1, 200), (1, -1, 2))


def step(x, k):
    """x moved by k representable doubles"""
    x = np.float64(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, np.float64(np.inf if k > 0 else -np.inf))
    return x


def curs_near(prev, reach=REACH, thresholds=THRESHOLDS):
    """prev + k ulp for the k around every threshold (bit patterns, unique, in order of appearance)"""
    out, seen = [], set()
    for t in thresholds:
        with np.errstate(over="ignore"):
            base = np.float64(prev) + np.float64(t)
        for k in range(-reach, reach + 1):
            c = step(base, k)
            key = c.tobytes()
            if key not in seen:
                seen.add(key)
                out.append(c)
    return out


def table():
    """-> (rows_i int32 [n][4] = form, it, min_iter, max_iter; rows_d float64 [n][3] = eps, trace_prev, cur)"""
    pairs = []
    for prev in PREVS_FINITE:
        pairs += [(prev, c) for c in curs_near(prev)]
        pairs += [(prev, c) for c in (np.nan, np.inf, -np.inf)]
    for prev in PREVS_OTHER:
        pairs += [(prev, c) for c in (prev, -prev, np.nan, 0.0, -1.0, 1.7e308, -1.7e308)]
    ri, rd = [], []
    for form in FORMS:
        for it, mn, mx in POSITIONS:
            for eps in EPSILONS:
                for prev, cur in pairs:
                    ri.append((form, it, mn, mx))
                    rd.append((eps, prev, cur))
    return np.array(ri, dtype=np.int32), np.array(rd, dtype=np.float64)


def table_verdicts(rows_i, rows_d, judge=verdict, prev=prev_of):
    """-> (verdict [n] int32, X[it - 1] [n]) of the restatement on every row"""
    v = np.zeros(len(rows_i), dtype=np.int32)
    p = np.zeros(len(rows_i))
    for i, ((form, it, mn, mx), (eps, tp, cur)) in enumerate(zip(rows_i.tolist(), rows_d)):
        p[i] = prev(it, mx, tp, cur)
        v[i] = judge(form, it, mn, mx, eps, p[i], cur)
    return v, p


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint64), b.view(np.uint64)))


# ---- the traces planted into the reference's own loops (tests/golden/make_stop_golden.py) ---------------------------
CASE_LEN = 8


def planted_cases():
    """-> list of (trace [max_iter], min_iter, max_iter, eps).  A pair (prev, cur) of the table sits at a judged
    position of a short trace; the entries around it move by 100 a step, so the planted comparison decides."""
    cases = []

    def plant(prev, cur, eps, it, mn, mx):
        tr = np.zeros(mx)
        for i in range(mx):
            tr[i] = prev - 100.0 * (it - 1 - i) if i < it else cur + 100.0 * (i - it)
        if it >= 1:
            tr[it - 1] = prev
        tr[it] = cur
        cases.append((tr, mn, mx, eps))

    near = (-1e-6, 0.0, 1e-2)
    for prev in PREVS_FINITE:
        for c in curs_near(prev, 2, near):
            plant(prev, c, 1e-2, 3, 2, CASE_LEN)                   # it = min_iter + 1
            plant(prev, c, 1e-2, CASE_LEN - 1, 2, CASE_LEN)        # it = max_iter - 1
        for c in curs_near(prev, 1, near):
            plant(prev, c, 1e-2, 2, 2, CASE_LEN)                   # it = min_iter: not judged
            plant(prev, c, 1e-2, 1, -1, 2)
        for eps in EPSILONS[1:]:
            ts = (eps,) if np.isfinite(eps) else (0.0,)
            for c in curs_near(prev, 1, ts):
                plant(prev, c, eps, 3, 2, CASE_LEN)
    for prev in PREVS_OTHER:
        for c in (prev, -prev, np.nan, 0.0):
            for eps in (1e-2, np.inf, np.nan):
                plant(prev, c, eps, 3, 2, CASE_LEN)
    # it = 0 under min_iter = -1: X[-1] is the array's last entry
    for cur in (-3e8, -1.0, -2e-6, -1e-6, step(-1e-6, 1), step(-1e-6, -1), 0.0, 5e-3, 1e-2, step(1e-2, -1), 5.0,
                np.nan, np.inf, -np.inf):
        for eps in (1e-2, 0.0, np.inf):
            for mx in (1, 2, CASE_LEN):
                plant(0.0, cur, eps, 0, -1, mx)
            plant(0.0, cur, eps, 0, -3, 2)
    return cases


# ---- the ambient rule of tests/test_gpu_stop_rule.py ---------------------------------------------------------------
AMBIENT_RULE = dict(min_iter=0, max_iter=9, eps=0.3)       # cells leave at it = 1 .. 8: at most 8 forced calls


def ambient_inputs():
    """(AD, DP, theta, selected, psi0) of the c1 ambient fixture, with starts of this module's own"""
    from tests import ambient_np, gold
    g = gold.load("c1_ambient_step")
    AD, DP = gold.c1()
    theta = ambient_np.theta_of(g["GT_prob"], g["beta_mu"])
    psi0 = np.random.RandomState(5).dirichlet([1] * theta.shape[1], size=AD.shape[1])
    return AD, DP, theta, g["selected"], psi0
