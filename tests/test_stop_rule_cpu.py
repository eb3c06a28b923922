"""The stop rule before it runs on a GPU.  tests/stop_np.py restates the reference's loop; here it is held to the
reference's own loops (tests/golden/stop_rule.npz: Vireo._fit_VB and BinomMixtureVB._fit_BV run over planted bounds),
to every pinned NumPy fit of this suite, and the host build of csrc/vrx_stop.h -- the source text the five device
loops call -- is held to it on the whole planted table, as a stand-alone program under AddressSanitizer and UBSan.
Planted defects in a copy of the restatement each change some row, so the table can see them.  No GPU."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import __graft_entry__ as entry
from oracle import vireo_oracle as O
from tests import ambient_np as A
from tests import bulk_np as B
from tests import gold
from tests import stop_np as S
from tests import varmix_np as VN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def planted():
    ri, rd = S.table()
    v, p = S.table_verdicts(ri, rd)
    return ri, rd, v, p


@pytest.fixture(scope="module")
def golden():
    return gold.load("stop_rule")


def fixture_cases(g):
    for c in range(len(g["eps"])):
        mn, mx = (int(x) for x in g["rule_i"][c])
        yield c, g["trace"][c, :mx], mn, mx, float(g["eps"][c])


def fixture_text(g, name, c):
    off = g["text_off_" + name]
    return bytes(g["text_" + name][off[c]:off[c + 1]]).decode()


# ---- the table itself ------------------------------------------------------------------------------------------------
def test_table_holds_what_it_is_meant_to_hold(planted):
    ri, rd, v, p = planted
    assert 20000 < len(ri) < 100000
    for form in S.FORMS:
        assert set(v[ri[:, 0] == form].tolist()) == {0, 1, 2, 3}
    assert set(rd[:, 0][np.isfinite(rd[:, 0])].tolist()) == {1e-2, 1e-3, 0.0, -1.0, 5e-324}
    assert np.isnan(rd[:, 0]).any() and np.isinf(rd[:, 0]).any()
    for col in (1, 2):
        assert np.isnan(rd[:, col]).any() and (rd[:, col] == np.inf).any() and (rd[:, col] == -np.inf).any()
    # the rows of one form are the rows of the others: where do Vireo and BMM disagree?
    a, b = ri[:, 0] == S.VIREO, ri[:, 0] == S.BMM
    assert np.array_equal(ri[a][:, 1:], ri[b][:, 1:]) and S.same_bits(rd[a], rd[b])
    differ = v[a] != v[b]
    assert differ.sum() >= 10
    # (the row named in the issue: prev = -3e8, cur = prev - 17 ulp; Vireo does not call it a decrease, BMM does)
    prev, cur = np.float64(-3e8), S.step(-3e8, -17)
    assert not S.decreased(S.VIREO, prev, cur) and S.decreased(S.BMM, prev, cur)
    hit = differ & (rd[a][:, 1] == prev) & (rd[a][:, 2] == cur) & (ri[a][:, 1] >= 1)
    assert hit.any()
    # it = 0: X[-1] is 0, or X[0] when max_iter is 1
    zero = ri[:, 1] == 0
    one = zero & (ri[:, 3] == 1)
    assert one.any() and S.same_bits(p[one], rd[one, 2])
    assert (zero & ~one).any() and np.all(p[zero & ~one] == 0.0)
    assert S.same_bits(p[~zero], rd[~zero, 1])


# ---- the host build of vrx_stop.h under sanitizers -----------------------------------------------------------------
def _compilers():
    out = []
    if shutil.which("g++"):
        out.append(shutil.which("g++"))
    for clang in ("/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++"):
        if os.path.exists(clang):
            out.append(clang)
            break
    return out


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """the sanitizer builds of tests/san/stop_host.cpp, one per host compiler found (as tests/test_bgzf_cpu.py)"""
    compilers = _compilers()
    assert compilers, "no host compiler"
    d = tmp_path_factory.mktemp("stop_san")
    out = []
    for k, cxx in enumerate(compilers):
        exe = str(d / ("stop_host_%d" % k))
        static = ["-static-libasan", "-static-libubsan"] if cxx.endswith("g++") and "clang" not in cxx else []
        subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
                       + static + [os.path.join(ROOT, "tests", "san", "stop_host.cpp"), "-o", exe], check=True)
        out.append(exe)
    return out


def run_host(exe, ri, rd, workdir):
    cases, results = os.path.join(workdir, "cases.bin"), os.path.join(workdir, "results.bin")
    with open(cases, "wb") as fh:
        fh.write(struct.pack("<q", len(ri)))
        fh.write(np.ascontiguousarray(ri, dtype="<i4").tobytes())
        fh.write(np.ascontiguousarray(rd, dtype="<f8").tobytes())
    r = subprocess.run([exe, cases, results], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", "sanitizer log:\n" + r.stderr[-4000:]
    data = open(results, "rb").read()
    n = len(ri)
    assert len(data) == 12 * n
    return np.frombuffer(data, "<i4", n), np.frombuffer(data, "<f8", n, 4 * n)


def test_host_judge_equals_the_restatement_on_every_row(programs, planted, tmp_path):
    ri, rd, v, p = planted
    for exe in programs:
        got_v, got_p = run_host(exe, ri, rd, str(tmp_path))
        bad = np.flatnonzero(got_v != v)
        assert bad.size == 0, (exe, ri[bad[:5]], rd[bad[:5]], got_v[bad[:5]], v[bad[:5]])
        assert S.same_bits(got_p, p), exe


# ---- the reference's own loops ---------------------------------------------------------------------------------------
def test_replay_reproduces_the_reference_loops(golden):
    g = golden
    assert 300 <= len(g["eps"]) <= 1000
    seen = {name: set() for name in ("vireo", "bmm")}
    disagree = []
    for c, tr, mn, mx, eps in fixture_cases(g):
        for form, name in ((S.VIREO, "vireo"), (S.BMM, "bmm")):
            it, bits, kept = S.replay(form, tr, mn, mx, eps)
            assert kept == g["kept_" + name][c] and it + 1 == g["computed_" + name][c], (name, c)
            assert S.lines(form, tr, mn, mx, eps) == fixture_text(g, name, c), (name, c)
            seen[name].add((it, bits))
        if (g["kept_vireo"][c] != g["kept_bmm"][c]
                or fixture_text(g, "vireo", c).count("\n\n") != fixture_text(g, "bmm", c).count("\n\n")):
            disagree.append(c)
    for name in seen:                                   # early stops, full runs, each warning, none
        assert {b for _, b in seen[name]} >= {0, 1, 2, 3}, name
        assert len({i for i, _ in seen[name]}) >= 4, name
    assert len(disagree) >= 4
    # the 17-ulp row is one of them: _fit_BV warns and goes on, _fit_VB stops
    prev, cur = np.float64(-3e8), S.step(-3e8, -17)
    named = [c for c, tr, mn, mx, eps in fixture_cases(g)
             if c in disagree and mx == S.CASE_LEN and tr[2] == prev and tr[3] == cur and mn == 2]
    assert named
    c = named[0]
    assert g["kept_vireo"][c] == 3 and g["kept_bmm"][c] > 3 and "ELBO decreases" in fixture_text(g, "bmm", c)
    # negative min_iter reached it = 0 in the reference, for max_iter 1 and 2
    neg = [(mx, g["computed_vireo"][c]) for c, tr, mn, mx, eps in fixture_cases(g) if mn < 0]
    assert {mx for mx, _ in neg} >= {1, 2, S.CASE_LEN} and any(n == 1 and mx > 1 for mx, n in neg)


def test_fixture_is_the_planted_cases(golden):
    cases = S.planted_cases()
    assert len(cases) == len(golden["eps"])
    for (c, tr, mn, mx, eps), (tr2, mn2, mx2, eps2) in zip(fixture_cases(golden), cases):
        assert (mn, mx) == (mn2, mx2) and S.same_bits(tr, tr2) and S.same_bits([eps], [eps2])


# ---- the pinned fits of this suite -----------------------------------------------------------------------------------
def rules_for(U, min_iters):
    """rules whose stops fall on U's own differences: on them, beside them, and the plain ones"""
    d = np.diff(U)
    out = []
    for mn in min_iters:
        for j in range(max(mn + 1, 1), min(mn + 6, len(U) - 1)):
            out += [(mn, len(U), d[j - 1]), (mn, len(U), np.nextafter(d[j - 1], np.inf))]
        out += [(mn, len(U), e) for e in (1e-2, 1e-3, 0.0, -1.0, np.inf, np.nan)]
        out += [(mn, mx, 1e-2) for mx in (1, 2, mn + 1, mn + 2) if 1 <= mx <= len(U)]
    return out


def test_replay_predicts_the_oracle_fits():
    T = 24
    AD, DP = O.synth_donor(300, 200, 3, 0.06, seed=3)
    for form, new, fit in ((S.VIREO, lambda: O.vireo_new(200, 300, 3), O.vireo_fit_vb),
                           (S.BMM, lambda: O.bmm_new(200, 300, 3), O.bmm_fit_vb)):
        def run(mn, mx, eps):
            np.random.seed(11)
            st = new()
            r = fit(st, AD, DP, max_iter=mx, min_iter=mn, epsilon_conv=eps)
            return r[1] if isinstance(r, tuple) else r
        np.random.seed(11)
        st = new()
        r = fit(st, AD, DP, max_iter=T + 1, min_iter=T + 1)
        U = (r[0] if isinstance(r, tuple) else st.ELBO_iters)[:T]
        assert len(U) == T
        its = set()
        for mn, mx, eps in rules_for(U, (-1, 0, 2, 5)):
            it = S.replay(form, U, mn, mx, eps)[0]
            assert run(mn, mx, eps) == it, (form, mn, mx, eps)
            its.add(it)
        assert len(its) >= 6


def test_replay_predicts_the_bulk_fit():
    AD, DP, GT = B.c1_bulk()
    psi, theta = np.random.RandomState(3).dirichlet(np.ones(GT.shape[1])), np.array([0.01, 0.5, 0.99])
    T = 30
    full = B.fit(AD, DP, GT, psi, theta, max_iter=T, min_iter=T)
    U = np.append(full["logLik_all"], full["logLik"])
    assert len(U) == T
    its = set()
    for mn, mx, eps in rules_for(U, (-1, 0, 3, 8)):
        got = B.fit(AD, DP, GT, psi, theta, max_iter=mx, min_iter=mn, epsilon_conv=eps)
        it, bits, kept = S.replay(S.EM, U, mn, mx, eps)
        assert got["it"] == it and len(got["logLik_all"]) == kept, (mn, mx, eps)
        assert S.same_bits(np.append(got["logLik_all"], got["logLik"]), U[:it + 1])
        assert "".join(w + "\n" for w in got["warnings"]) == S.lines(S.EM, U, mn, mx, eps)
        its.add(it)
    assert len(its) >= 6


def test_replay_predicts_the_ambient_cells():
    g = gold.load("c1_ambient_step")
    AD, DP = gold.c1()
    AD, DP = AD.tocsc(), DP.tocsc()
    theta = A.theta_of(g["GT_prob"], g["beta_mu"])
    K = theta.shape[1]
    psi0 = np.random.RandomState(5).dirichlet([1] * K, size=AD.shape[1])
    T = 40
    its = set()
    for c in range(0, 60, 3):
        rows, a, b = A.cell_entries(AD, DP, g["selected"], c)
        if a.sum() + b.sum() == 0:
            continue
        U = []
        A.fit_cell(a, b, theta[rows], psi0[c], min_iter=T, max_iter=T, trace=U)
        assert len(U) == T
        for mn, mx, eps in rules_for(np.array(U), (0, 3)):
            it = S.replay(S.EM, U, mn, mx, eps)[0]
            assert A.fit_cell(a, b, theta[rows], psi0[c], min_iter=mn, max_iter=mx, eps=eps)[3] == it, (c, mn, mx, eps)
            its.add(it)
    assert len(its) >= 6


def test_ambient_rule_of_the_gpu_test_gives_few_counts():
    """tests/test_gpu_stop_rule.py makes one forced call per distinct count: the restatement alone says how many"""
    AD, DP, theta, sel, psi0 = S.ambient_inputs()
    it = A.predict(theta, sel, AD, DP, psi0, **S.AMBIENT_RULE)[3]
    assert 3 <= len(set(it.tolist())) <= 8
    assert min(it) > S.AMBIENT_RULE["min_iter"] and np.sum(it < S.AMBIENT_RULE["max_iter"] - 1) > 100


def test_replay_predicts_the_variant_mixture_rows():
    AD, DP = VN.gen_rows([120, 64, 33, 9, 2], seed=8, n_cell=120)
    T = 30
    its = set()
    for v in range(len(AD)):
        for K in (2, 3):
            U = VN.fit_row(AD[v], DP[v], K, max_iter=T, min_iter=T)["trace"]
            assert len(U) == T
            for mn, mx, eps in rules_for(U, (0, 2)):
                got = VN.fit_row(AD[v], DP[v], K, max_iter=mx, min_iter=mn, epsilon_conv=eps)
                it, bits, kept = S.replay(S.BMM, U, mn, mx, eps)
                assert (got["n_iter"], got["warn"]) == (it, bits), (v, K, mn, mx, eps)
                assert S.same_bits(got["trace"], U[:it + 1])
                its.add(it)
    assert len(its) >= 6


# ---- planted defects -------------------------------------------------------------------------------------------------
def _mutant(decr=S.decreased, gate=lambda it, mn: it > mn, eps_first=False, eps_le=False):
    def judge(form, it, mn, mx, eps, prev, cur):
        if not gate(it, mn):
            return S.CONTINUE
        if decr(form, prev, cur):
            return S.WARN_DECREASED
        with np.errstate(invalid="ignore", over="ignore"):
            d = np.float64(cur) - np.float64(prev)
            small = bool(d <= np.float64(eps)) if eps_le else bool(d < np.float64(eps))
        if eps_first:
            return S.STOP if small else (S.WARN_NOT_CONVERGED if it == mx - 1 else S.CONTINUE)
        if it == mx - 1:
            return S.WARN_NOT_CONVERGED
        return S.STOP if small else S.CONTINUE
    return judge


def _decr_le(form, prev, cur):
    prev, cur = np.float64(prev), np.float64(cur)
    with np.errstate(invalid="ignore", over="ignore"):
        if form == S.VIREO:
            return bool(cur <= prev - np.float64(1e-6))
        if form == S.BMM:
            return bool(cur - prev <= np.float64(-1e-6))
        return bool(cur <= prev)


MUTANTS = {
    "decreased: <= for <": dict(judge=_mutant(decr=_decr_le)),
    "eps: <= for <": dict(judge=_mutant(eps_le=True)),
    "vireo judged with the bmm test": dict(judge=_mutant(
        decr=lambda f, p, c: S.decreased(S.BMM if f == S.VIREO else f, p, c)), forms=(S.VIREO,)),
    "bmm judged with the vireo test": dict(judge=_mutant(
        decr=lambda f, p, c: S.decreased(S.VIREO if f == S.BMM else f, p, c)), forms=(S.BMM,)),
    "em judged with the vireo test": dict(judge=_mutant(
        decr=lambda f, p, c: S.decreased(S.VIREO if f == S.EM else f, p, c)), forms=(S.EM,)),
    "eps before max_iter - 1": dict(judge=_mutant(eps_first=True)),
    "it >= min_iter": dict(judge=_mutant(gate=lambda it, mn: it >= mn)),
    "prev at it = 0 from the end of the computed trace": dict(prev=lambda it, mx, tp, cur: tp if it >= 1 else cur),
    "prev at it = 0 always zero": dict(prev=lambda it, mx, tp, cur: tp if it >= 1 else 0.0),
}


def test_the_unmutated_copy_changes_nothing(planted):
    ri, rd, v, p = planted
    v2, p2 = S.table_verdicts(ri, rd, judge=_mutant())
    assert np.array_equal(v, v2) and S.same_bits(p, p2)


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_every_planted_defect_changes_a_row(planted, name):
    ri, rd, v, p = planted
    m = MUTANTS[name]
    v2, p2 = S.table_verdicts(ri, rd, judge=m.get("judge", S.verdict), prev=m.get("prev", S.prev_of))
    changed = v2 != v
    assert changed.any(), name
    for form in m.get("forms", S.FORMS):
        assert changed[ri[:, 0] == form].any(), (name, form)
    other = ~np.isin(ri[:, 0], m.get("forms", S.FORMS))
    assert not changed[other].any()


# ---- what the package prints ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def va():
    entry.build()
    import vireo_amd
    return vireo_amd


class _FakeModel:
    """stands where the device model stands: hands back the planted bounds up to the reference's ``it``"""

    def __init__(self, trace, it):
        self.trace, self.it = trace, it

    def fit(self, max_iter, min_iter, eps, delay_fit_theta=0):
        return self.trace[:self.it + 1].copy(), self.it, 0

    def close(self):
        pass


def test_vireo_fit_vb_prints_what_the_reference_prints(va, golden, monkeypatch, capsys):
    m = va.Vireo(n_cell=2, n_var=2, n_donor=2)
    monkeypatch.setattr(m, "_pull", lambda dm, want_GT=True: None)
    for c, tr, mn, mx, eps in fixture_cases(golden):
        it = int(golden["computed_vireo"][c]) - 1
        monkeypatch.setattr(m, "_device_model", lambda AD, DP: (_FakeModel(tr, it), None))
        capsys.readouterr()
        kept = m._fit_VB(None, None, max_iter=mx, min_iter=mn, epsilon_conv=eps, verbose=True)
        assert capsys.readouterr().out == fixture_text(golden, "vireo", c), c
        assert S.same_bits(kept, tr[:golden["kept_vireo"][c]])


def test_bmm_warn_prints_what_the_reference_prints(va, golden, capsys):
    for c, tr, mn, mx, eps in fixture_cases(golden):
        it = int(golden["computed_bmm"][c]) - 1
        capsys.readouterr()
        va.BinomMixtureVB._warn(tr[:it + 1], it, mn, mx)
        assert capsys.readouterr().out == fixture_text(golden, "bmm", c), c
