"""Sequences of model calls: the machinery of tests/test_model_sequences_cpu.py (host only) and
tests/test_gpu_model_sequences.py (the device).

A ``DeviceModel`` lives across a whole restart search (vireo_amd/restarts.py, bmm_model.py), and
between its calls the engine carries state no caller sees (csrc/vrx_engine.hip: w_valid, s_pending,
l_pending, theta_pending, elbo_deferred, n_cell_part, th_cur, the control words).  The rule that
makes those safe: a deferral is invisible at the ABI.  The *visible state* sigma of a model is its
state arrays (per restart), the priors as last set, logLik_ID, the snapshot slot and the two staging
buffers; the two properties held here are

1. history independence, bit for bit: a call's results (trace, it, flags, ELBO, ELBO parts, sigma
   afterwards) on a model with any history are those of a fresh model that was given sigma through
   set_prior / set_state / set_loglik / snapshot / stage_raw -- ``twin`` is that fresh-model executor;
2. observation is true: what get_state / get_loglik / elbo_parts return after a sequence is what the
   float64 oracle driven through the same sequence holds (``RefModel``), within the tolerance
   tests/test_gpu_fuzz.py uses for chains of a few iterations.

``RefModel`` is oracle/vireo_oracle.py as a state machine with the DeviceModel / DeviceBatch method
names.  ``LazyRef`` is RefModel with deferrals of the engine's kind restated as flags -- somewhat
lazier than the engine, so that every flag lives across calls -- and ``wrong=`` plants one way such
a flag can be mishandled: the CPU test holds that the sequence families below catch every one.

The sequences: (1) every ordered pair of the alphabet from one start state, (2) the production
sequences of restarts.py / bmm_model.py with their iteration counts shortened (a chaotic iteration
amplifies a rounding; the tolerance stays, the walk is shortened), (3) seeded walks of twelve calls.
Every sequence opens with the same prelude, which is history as well: it leaves a snapshot of
another state, valid S / W / KL caches and a computed ELBO behind.  logLik_ID of a restart batch
can be neither read nor set through the Python classes, so the batch alphabet holds only calls that
define what they read.
"""
import copy
from types import SimpleNamespace

import numpy as np

from oracle import vireo_oracle as O
from tests import exact_cases as EC
from tests import stop_np as S

STEP_THETA, STEP_GT, STEP_ID, STEP_LOGLIK, STEP_ELBO, STEP_SOFTMAX = 1, 2, 3, 4, 5, 6   # vireo_amd/_lib.py
STEP_UNKNOWN = 99


REFUSED = "refused"            # what a refused call leaves in a trail in place of a result


class Refused(Exception):
    """the oracle's side of an argument check of the C ABI"""


# ------------------------------------------------------------------------------------
# configurations
# ------------------------------------------------------------------------------------
CONFIGS = {}


def _config(name, data, K, kind="vireo", T=3, ase=False, fix=False, learn_gt=True, learn_theta=True, R=1,
            env=None, want=None, families=(1, 2, 3)):
    CONFIGS[name] = SimpleNamespace(name=name, data=data, K=K, kind=kind, T=T if kind == "vireo" else 1, ase=ase,
                                    fix=fix, learn_gt=learn_gt, learn_theta=learn_theta, R=R, env=dict(env or {}),
                                    want=dict(want or {}), families=families)


_RIDE1, _RIDE0 = {"VIREO_ELBO_RIDE": "1"}, {"VIREO_ELBO_RIDE": "0"}
_config("gather_fused", "small", 4, env=dict(EC.LDS0, **EC.FUSE1, **_RIDE1), want=EC.OFF)
_config("gather_plain", "small", 4, env=dict(EC.LDS0, **EC.FUSE0, **_RIDE0), want=EC.OFF)
_config("lds_one_range", "mid", 6, env=EC.LDS1, want=dict(EC.ON, cell_form=1, var_form=3))
_config("lds_many_ranges", "many", 6, env=EC.LDS1, want=dict(EC.ON, ranges_variant=EC.many, ranges_cell=EC.many))
_config("lds_split_rows", "split", 6, env=EC.LDS1,
        want=dict(EC.ON, extra_pieces_cell=EC.some, extra_pieces_variant=EC.some), families=(2, 3))
_config("ase_fix_beta_sum", "small", 4, ase=True, fix=True, env=EC.LDS0, want=EC.OFF)
_config("fixed_gt_no_theta", "small", 4, learn_gt=False, learn_theta=False, env=EC.LDS0, want=EC.OFF)
_config("clone_gather", "clone", 5, kind="bmm", env=EC.LDS0, want=EC.OFF)
_config("clone_lds", "clone", 5, kind="bmm", env=EC.LDS1, want=EC.ON)
_config("batch3_gather", "small", 4, R=3, env=EC.LDS0, want=dict(EC.OFF, n_batch=3))
_config("batch3_lds", "mid", 4, R=3, env=EC.LDS1, want=dict(EC.ON, n_batch=3))
# the CPU file's own: the smallest data, one single model and one batch
_config("cpu_single", "small", 3)
_config("cpu_batch", "small", 3, R=3)
_config("cpu_clone", "tiny", 3, kind="bmm")
GPU_CONFIGS = [n for n in CONFIGS if not n.startswith("cpu_")]


def theta_shape(cfg, N):
    return ((N if cfg.ase else 1), cfg.T) if cfg.kind == "vireo" else (N, cfg.K)


def default_prior(cfg):
    """set_prior() without arguments: vireo_model.py:107-137, bmm_model.py:87-105"""
    if cfg.kind == "vireo":
        g = np.linspace(0.01, 0.99, cfg.T)[None, :]
        return (None, None, g * 50.0, (1 - g) * 50.0)
    return (None, None, np.ones((1, cfg.K)), np.ones((1, cfg.K)))


# ------------------------------------------------------------------------------------
# the oracle as a state machine
# ------------------------------------------------------------------------------------
class RefModel:
    """oracle/vireo_oracle.py behind the method names of DeviceModel (R = 1) and DeviceBatch"""

    def __init__(self, cfg, AD, DP, R=1):
        self.c, self.AD, self.DP, self.R = cfg, AD, DP, int(R)
        self.N, self.M = AD.shape
        self.K, self.T = cfg.K, cfg.T
        self.vireo = cfg.kind == "vireo"
        self.form = S.VIREO if self.vireo else S.BMM
        th = theta_shape(cfg, self.N)        # (the device's arrays are undefined until they are set; zeros here)
        self.s = [SimpleNamespace(ID=np.zeros((self.M, self.K)), mu=np.zeros(th), sm=np.zeros(th),
                                  GT=np.zeros((self.N, self.K, self.T)) if self.vireo else None) for _ in range(self.R)]
        self.L = [np.zeros((self.M, self.K)) for _ in range(self.R)]     # (vrx_model_create zeroes LID)
        self.parts = [None] * self.R
        self.pri = None
        self.snap, self.reserved, self.stage = None, False, {}

    def clone(self):
        m = copy.copy(self)
        m.s = [copy.copy(s) for s in self.s]
        m.L, m.parts, m.stage = list(self.L), list(self.parts), dict(self.stage)
        return m

    def close(self):
        pass

    # ---- hooks of LazyRef --------------------------------------------------------------
    def _sync(self, who):
        pass

    def _wrote(self, r, id_=False, gt=False, theta=False):
        pass

    def _id_for_sums(self, r):
        return self.s[r].ID

    def _w_inputs(self, r):
        s = self.s[r]
        return s.GT, s.mu, s.sm

    def _tables(self):
        return self.pri[0], self.pri[1]

    def _store_theta(self, r, mu, sm, pend):
        self.s[r].mu, self.s[r].sm = mu, sm

    def _store_loglik(self, r, L, loop):
        self.L[r] = L

    def _store_parts(self, r, parts, loop_last):
        self.parts[r] = parts

    def _frozen(self, r):
        return False

    def _begin(self):
        pass

    def _stopped(self, its, stops):
        pass

    # ---- plumbing ------------------------------------------------------------------------
    def _refuse(self, why):
        raise Refused(why)

    def _single(self, who):
        self._sync(who)
        if self.R != 1:
            raise TypeError("not available on a restart batch")

    def _ost(self, r, ID=None, GT=None, mu=None, sm=None):
        """the oracle's state object of restart r (tests/exact_cases.py, oracle_state)"""
        c, s = self.c, self.s[r]
        idp, gtp = self._tables()
        st = SimpleNamespace(n_cell=self.M, n_var=self.N, n_donor=self.K, n_GT=self.T, learn_GT=c.learn_gt,
                             learn_theta=c.learn_theta, ASE_mode=c.ase, fix_beta_sum=c.fix,
                             beta_mu=s.mu if mu is None else mu, beta_sum=s.sm if sm is None else sm,
                             ID_prob=s.ID if ID is None else ID, theta_s1_prior=self.pri[2],
                             theta_s2_prior=self.pri[3])
        st.ID_prior = idp if idp is not None else O.unit_sum(np.ones((self.M, self.K)))
        if self.vireo:
            st.GT_prob = s.GT if GT is None else GT
            st.GT_prior = (np.broadcast_to(gtp, st.GT_prob.shape) if gtp is not None
                           else O.unit_sum(np.ones((self.N, self.K, self.T))))
        return st

    @staticmethod
    def _arr(a):
        return None if a is None else np.array(a, dtype=np.float64)

    def _put(self, r, ID, GT, mu, sm, raw):
        s = self.s[r]
        if ID is not None:
            s.ID = O.unit_sum(self._arr(ID)) if raw else self._arr(ID)
        if GT is not None and self.vireo:
            s.GT = O.unit_sum(self._arr(GT)) if raw else self._arr(GT)
        if mu is not None:
            s.mu = self._arr(mu)
        if sm is not None:
            s.sm = self._arr(sm)
        self._wrote(r, id_=ID is not None, gt=GT is not None and self.vireo, theta=mu is not None or sm is not None)

    # ---- state / priors ------------------------------------------------------------------
    def set_prior(self, ID_prior, GT_prior, theta_s1_prior, theta_s2_prior):
        self._sync("set_prior")

        def table(P):                      # (a constant table is the uniform one: engine.py, _prior_rows)
            P = self._arr(P)
            return None if P is None or (P.size and P.min() == P.max()) else P
        self.pri = (table(ID_prior), table(GT_prior) if self.vireo else None,
                    self._arr(theta_s1_prior), self._arr(theta_s2_prior))
        self._prior_set()

    def _prior_set(self):
        pass

    def set_state(self, ID_prob=None, GT_prob=None, beta_mu=None, beta_sum=None):
        self._single("set_state")
        self._put(0, ID_prob, GT_prob, beta_mu, beta_sum, False)

    def set_state_raw(self, ID_raw=None, GT_raw=None, beta_mu=None, beta_sum=None):
        self._single("set_state_raw")
        self._put(0, ID_raw, GT_raw, beta_mu, beta_sum, True)

    def stage_reserve(self):
        self._single("stage_reserve")
        if not self.vireo:
            self._refuse("single Vireo models only")
        self.reserved = True

    def stage_raw(self, buf, ID_raw, GT_raw):
        self._single("stage_raw")
        if not self.reserved or buf not in (0, 1):
            self._refuse("call stage_reserve first")
        self.stage[buf] = (self._arr(ID_raw), self._arr(GT_raw))

    def set_state_staged(self, buf, beta_mu=None, beta_sum=None):
        self._single("set_state_staged")
        if not self.reserved or buf not in (0, 1):
            self._refuse("nothing was staged")
        self._put(0, self.stage[buf][0], self.stage[buf][1], beta_mu, beta_sum, True)

    def snapshot(self):
        self._single("snapshot")
        self.snap = copy.copy(self.s[0])

    def restore(self):
        self._single("restore")
        if self.snap is None:
            self._refuse("nothing saved")
        self.s[0] = copy.copy(self.snap)
        self._wrote(0, id_=True, gt=self.vireo, theta=True)

    def get_state(self, want_GT=True):
        self._single("get_state")
        s = self.s[0]
        return s.ID.copy(), (s.GT.copy() if want_GT and self.vireo else None), s.mu.copy(), s.sm.copy()

    def get_loglik(self):
        self._single("get_loglik")
        return self.L[0].copy()

    def set_loglik(self, L):
        self._single("set_loglik")
        self.L[0] = self._arr(L)

    def elbo_parts(self):
        self._sync("elbo_parts")
        p = np.array([np.asarray(q, dtype=np.float64) for q in self.parts])
        return p[0] if self.R == 1 else p

    def set_restart(self, r, ID=None, GT=None, beta_mu=None, beta_sum=None, raw=False):
        self._sync("set_restart")
        if not 0 <= r < self.R:
            self._refuse("slot outside the batch")
        self._put(r, ID, GT, beta_mu, beta_sum, raw)

    def copy_to(self, single, r):
        self._sync("copy_to")
        single._sync("copied_into")
        single.s[0] = copy.copy(self.s[r])
        single._wrote(0, id_=True, gt=self.vireo, theta=True)

    # ---- the updates -----------------------------------------------------------------------
    def _theta(self, r, pend=False):
        if self._frozen(r):
            return
        st = self._ost(r, ID=self._id_for_sums(r))
        (O.vireo_theta_step if self.vireo else O.bmm_theta_step)(st, self.AD, self.DP)
        self._store_theta(r, st.beta_mu, st.beta_sum, pend)
        self._wrote(r, theta=True)

    def _gt(self, r):
        if self._frozen(r):
            return
        st = self._ost(r, ID=self._id_for_sums(r))
        O.vireo_gt_step(st, self.AD, self.DP)
        self.s[r].GT = st.GT_prob
        self._wrote(r, gt=True)

    def _loglik(self, r):
        GT, mu, sm = self._w_inputs(r)
        st = self._ost(r, GT=GT, mu=mu, sm=sm)
        if self.vireo:
            return O._cell_loglik(st.GT_prob, *O._psi3(st), self.AD, self.DP)
        return O.bmm_cell_loglik(st, self.AD, self.DP)

    def _softmax(self, r, L):
        st = self._ost(r)
        self.s[r].ID = O.softmax_log(L + np.log(st.ID_prior))
        self._wrote(r, id_=True)

    def _parts(self, r, L, where):
        st = self._ost(r)
        return self._parts_of(r, st, L, where)

    def _parts_of(self, r, st, L, where):
        return np.array(O.vireo_elbo_parts(st, L) if self.vireo else EC._bmm_parts(st, L), dtype=np.float64)

    def _iteration(self, r, do_theta, last):
        """vireo_model.py:257-264 / bmm_model.py:183-188 -> this iteration's ELBO"""
        if self.vireo:
            if do_theta:
                self._theta(r)
            if self.c.learn_gt:
                self._gt(r)
        else:
            self._theta(r)
        L = self._loglik(r)
        self._softmax(r, L)
        self._store_loglik(r, L, True)
        parts = self._parts(r, L, "fit")
        self._store_parts(r, parts, last)
        return parts[0] - parts[1] - parts[2] - parts[3]

    def fit(self, max_iter, min_iter, epsilon_conv, delay_fit_theta=0):
        self._sync("fit")
        self._begin()
        traces, its, flags, stops = [], np.zeros(self.R, dtype=np.int32), np.zeros(self.R, dtype=np.int32), []
        for r in range(self.R):
            if self._frozen(r):                                   # (a planted defect: every kernel returns at once)
                traces.append(np.zeros(1))
                stops.append(False)
                continue
            X, it, stop = np.zeros(max_iter), 0, False
            for it in range(max_iter):
                do_theta = self.vireo and self.c.learn_theta and it >= delay_fit_theta
                X[it] = self._iteration(r, do_theta, False)
                v = S.verdict(self.form, it, min_iter, max_iter, epsilon_conv, X[it - 1], X[it])
                if v == S.STOP:
                    stop = True
                    break
                if v != S.CONTINUE:
                    flags[r] |= 1 if v == S.WARN_DECREASED else 2
            traces.append(X[:it + 1])
            its[r] = it
            stops.append(stop)
        self._stopped(its, stops)
        if self.R == 1:
            return traces[0], int(its[0]), int(flags[0])
        return traces, its, flags

    def run_iters(self, n_iter, theta_from_iter=0):
        self._sync("run_iters")
        self._begin()
        X = np.zeros((self.R, n_iter))
        for r in range(self.R):
            if self._frozen(r):
                continue
            for it in range(n_iter):
                X[r, it] = self._iteration(r, self.vireo and self.c.learn_theta and it >= theta_from_iter,
                                           it == n_iter - 1)
        return (X[0] if self.R == 1 else X), 0.0

    def step(self, which):
        self._sync("step")
        if which not in (STEP_THETA, STEP_GT, STEP_ID, STEP_LOGLIK, STEP_ELBO, STEP_SOFTMAX) or (
                which == STEP_GT and not self.vireo):
            self._refuse("unknown step %d" % which)
        self._begin()
        out = np.zeros(self.R)
        for r in range(self.R):
            if self._frozen(r):
                continue
            if which == STEP_THETA:
                self._theta(r, pend=True)
            elif which == STEP_GT:
                self._gt(r)
            elif which in (STEP_ID, STEP_LOGLIK):
                L = self._loglik(r)
                self._store_loglik(r, L, False)
                if which == STEP_ID:
                    self._softmax(r, L)
            elif which == STEP_SOFTMAX:
                self._softmax(r, self.L[r])
            else:
                parts = self._parts(r, self.L[r], "step")
                self._store_parts(r, parts, False)
                out[r] = parts[0] - parts[1] - parts[2] - parts[3]
        return float(out[0]) if self.R == 1 else out


# ------------------------------------------------------------------------------------
# the oracle with deferrals, and the ways to get one wrong
# ------------------------------------------------------------------------------------
DEFECTS = (
    "restore_keeps_w",                # restore leaves W valid: the next cell pass runs on the old (GT, theta)
    "set_id_keeps_s",                 # set_state(ID only) leaves S valid: the next theta / GT update sums the old ID
    "set_prior_keeps_log_tables",     # set_prior leaves the log tables of the ID / GT priors as they were
    "set_prior_keeps_kl",             # set_prior leaves the KL_theta partials valid
    "fit_leaves_old_loglik",          # a fit never writes logLik_ID
    "get_state_unfinalised_theta",    # get_state reads theta in front of its deferred finalisation
    "snapshot_unfinalised_theta",     # snapshot saves it so
    "set_loglik_ignored_if_pending",  # set_loglik while a deferred sum waits: the sum lands on top of it
    "elbo_stale_partial_count",       # the ELBO sums as many cell partials as the kernel before the last wrote
    "stop_flag_survives",             # the stop word of a fit is still set in the next call
    "batch_slot_stays_frozen",        # ... for the slots of a batch that stopped before its last one
    "refusal_drops_deferred_elbo",    # a refused call forgets the ELBO parts that still waited
)
BATCH_DEFECTS = ("batch_slot_stays_frozen",)


class LazyRef(RefModel):
    """RefModel that defers like the engine: S and W cached across calls, theta finalised and
    logLik_ID / the ELBO parts summed by their next consumer, the KL_theta partials reused while
    theta and its prior stand, a stop word per slot.  With ``wrong=None`` every deferral is
    invisible: the results are RefModel's, bit for bit."""

    def __init__(self, cfg, AD, DP, R=1, wrong=None):
        super().__init__(cfg, AD, DP, R)
        assert wrong is None or wrong in DEFECTS
        self.wrong = wrong
        self.s_id = [None] * self.R          # the ID that S was summed from (s_valid)
        self.w_in = [None] * self.R          # the (GT, mu, sm) that W was formed from (w_valid)
        self.kl = [None] * self.R            # the KL_theta partials, summed
        self.th_pend = [None] * self.R
        self.l_pend = [None] * self.R
        self.p_pend = [None] * self.R
        self.tables = (None, None)
        self.cell_count = "step"             # which kernel wrote the cell partials last
        self.frozen = [False] * self.R

    def clone(self):
        m = super().clone()
        for k in ("s_id", "w_in", "kl", "th_pend", "l_pend", "p_pend", "frozen"):
            setattr(m, k, list(getattr(self, k)))
        return m

    NO_THETA = ("set_loglik", "get_loglik", "set_prior", "stage_reserve", "stage_raw", "elbo_parts")
    COMPUTE = ("step", "fit", "run_iters")

    def _sync(self, who):
        """what waits is finalised for the call that needs it, and stays where a call does not"""
        for r in range(self.R):
            if self.th_pend[r] is not None and who not in self.NO_THETA and not (
                    (who == "get_state" and self.wrong == "get_state_unfinalised_theta")
                    or (who == "snapshot" and self.wrong == "snapshot_unfinalised_theta")):
                self.s[r].mu, self.s[r].sm = self.th_pend[r]
                self.th_pend[r] = None
            if self.l_pend[r] is not None:
                if who == "set_loglik":
                    if self.wrong != "set_loglik_ignored_if_pending":
                        self.l_pend[r] = None
                elif who == "get_loglik" or who in self.COMPUTE:
                    self.L[r], self.l_pend[r] = self.l_pend[r], None
            if self.p_pend[r] is not None and who in self.COMPUTE:
                self.parts[r], self.p_pend[r] = self.p_pend[r], None

    def elbo_parts(self):
        """(reads the waiting parts where they are: a read-back finalises nothing)"""
        self._sync("elbo_parts")
        p = np.array([np.asarray(w if w is not None else q, dtype=np.float64) for w, q in zip(self.p_pend, self.parts)])
        return p[0] if self.R == 1 else p

    def _pre_refusal(self):
        if self.wrong == "refusal_drops_deferred_elbo":
            self.p_pend = [None] * self.R

    def _wrote(self, r, id_=False, gt=False, theta=False):
        if id_:
            self.s_id[r] = None
        if gt or theta:
            self.w_in[r] = None
        if theta:
            self.kl[r] = None

    def set_state(self, ID_prob=None, GT_prob=None, beta_mu=None, beta_sum=None):
        keep = self.s_id[0]
        super().set_state(ID_prob, GT_prob, beta_mu, beta_sum)
        if self.wrong == "set_id_keeps_s" and GT_prob is None and beta_mu is None and beta_sum is None:
            self.s_id[0] = keep

    def restore(self):
        keep = self.w_in[0]
        super().restore()
        if self.wrong == "restore_keeps_w":
            self.w_in[0] = keep

    def _prior_set(self):
        if self.wrong != "set_prior_keeps_log_tables" or not self._had_prior:   # (the first one makes them)
            self.tables = (self.pri[0], self.pri[1])
        self._had_prior = True
        if self.wrong != "set_prior_keeps_kl":
            self.kl = [None] * self.R

    _had_prior = False

    def _tables(self):
        return self.tables

    def _id_for_sums(self, r):
        if self.s_id[r] is None:
            self.s_id[r] = self.s[r].ID
        return self.s_id[r]

    def _w_inputs(self, r):
        if self.w_in[r] is None:
            s = self.s[r]
            self.w_in[r] = (s.GT, s.mu, s.sm)
        return self.w_in[r]

    def _store_theta(self, r, mu, sm, pend):
        if pend:                              # (the step API leaves the finalisation to the next consumer)
            self.th_pend[r] = (mu, sm)
        else:
            self.s[r].mu, self.s[r].sm = mu, sm

    def _store_loglik(self, r, L, loop):
        if not loop:
            self.L[r] = L
        elif self.wrong != "fit_leaves_old_loglik":
            self.l_pend[r] = L

    def _store_parts(self, r, parts, loop_last):
        if loop_last:
            self.p_pend[r] = parts
        else:
            self.parts[r], self.p_pend[r] = parts, None

    def _parts_of(self, r, st, L, where):
        parts = super()._parts_of(r, st, L, where)
        if self.kl[r] is None:
            self.kl[r] = parts[3]
        parts[3] = self.kl[r]
        if where == "step" and self.cell_count == "fit" and self.wrong == "elbo_stale_partial_count":
            h = self.M // 2                  # (the fused cell pass wrote fewer partials: the tail is not summed)
            st.ID_prob, st.ID_prior = st.ID_prob[:h], st.ID_prior[:h]
            parts[:2] = super()._parts_of(r, st, L[:h], where)[:2]
        self.cell_count = where
        return parts

    def _frozen(self, r):
        return self.frozen[r]

    def _begin(self):
        if self.wrong not in ("stop_flag_survives", "batch_slot_stays_frozen"):
            self.frozen = [False] * self.R

    def _stopped(self, its, stops):
        if self.wrong == "stop_flag_survives":
            self.frozen = [f or s for f, s in zip(self.frozen, stops)]
        elif self.wrong == "batch_slot_stays_frozen":
            last = max(int(i) for i in its)
            self.frozen = [f or (s and int(i) < last) for f, s, i in zip(self.frozen, stops, its)]

    def step(self, which):
        if which not in (STEP_THETA, STEP_GT, STEP_ID, STEP_LOGLIK, STEP_ELBO, STEP_SOFTMAX):
            self._pre_refusal()
        return super().step(which)

    def set_state_staged(self, buf, beta_mu=None, beta_sum=None):
        if not self.reserved:
            self._pre_refusal()
        return super().set_state_staged(buf, beta_mu, beta_sum)


# ------------------------------------------------------------------------------------
# a system: one single model, and a restart batch where the configuration has one
# ------------------------------------------------------------------------------------
class RefFactory:
    """makes the models of a configuration: the oracle's (cls = RefModel / LazyRef) here, the device's in
    tests/test_gpu_model_sequences.py"""

    def __init__(self, cfg, cls=RefModel, **kw):
        self.cfg, self.cls, self.kw = cfg, cls, kw
        self.AD, self.DP = EC.data(cfg.data)
        self.refusals = (Refused,)

    def single(self):
        return self.cls(self.cfg, self.AD, self.DP, 1, **self.kw)

    def batch(self):
        return self.cls(self.cfg, self.AD, self.DP, self.cfg.R, **self.kw)


class System:
    def __init__(self, factory):
        self.f, self.cfg = factory, factory.cfg
        self.single = factory.single()
        self.batch = factory.batch() if self.cfg.R > 1 else None
        self._probe = None
        self.calls = 0

    def probe(self):
        """a single model that only ever receives a slot to be read"""
        if self._probe is None:
            self._probe = self.f.single()
        return self._probe

    def clone(self):
        s = copy.copy(self)
        s.single = self.single.clone()
        s.batch = self.batch.clone() if self.batch is not None else None
        s._probe = None
        return s

    def close(self):
        for m in (self.single, self.batch, self._probe):
            if m is not None:
                m.close()


# ------------------------------------------------------------------------------------
# fixed arguments
# ------------------------------------------------------------------------------------
def arguments(cfg):
    """every array a call of the alphabet passes, seeded by the configuration"""
    if getattr(cfg, "_x", None) is not None:
        return cfg._x
    AD, DP = EC.data(cfg.data)
    N, M = AD.shape
    K, T = cfg.K, cfg.T
    rng = np.random.default_rng(4242 + sum(map(ord, cfg.name)))
    rows, cols = theta_shape(cfg, N)
    vireo = cfg.kind == "vireo"

    def theta0():
        if vireo:                            # the constructor's (vireo_model.py:84-93)
            return np.ones((rows, cols)) * np.linspace(0.01, 0.99, T), np.full((rows, cols), 50.0)
        return rng.uniform(0.1, 0.9, (rows, cols)), rng.uniform(10.0, 60.0, (rows, cols))

    def state(theta=None):
        mu, sm = theta or (rng.uniform(0.05, 0.95, (rows, cols)), rng.uniform(5.0, 150.0, (rows, cols)))
        return (O.unit_sum(rng.random((M, K)) + 0.02),
                O.unit_sum(rng.random((N, K, T)) + 0.02) if vireo else None, mu, sm)

    x = SimpleNamespace(cfg=cfg, N=N, M=M)
    x.theta0 = theta0()
    x.start = [state(x.theta0 if vireo else None) for _ in range(cfg.R)]
    x.alt = state()
    x.other = state()
    x.raw = [(rng.random((M, K)), rng.random((N, K, T)) if vireo else None) for _ in range(3)]
    x.staged = (rng.random((M, K)), rng.random((N, K, T)))
    x.L = rng.normal(-40.0, 12.0, (M, K))
    x.default_prior = default_prior(cfg)
    p = SimpleNamespace(M=M, N=N, K=K, T=T, kind=cfg.kind)
    th = (dict(th1=rng.uniform(0.3, 40.0, (rows, cols)), th2=rng.uniform(0.3, 40.0, (rows, cols))) if cfg.ase
          else EC.pr_bmm_clones(p, rng) if not vireo else EC.pr_theta(p, rng))
    x.full_prior = (EC.pr_id_cells(p, rng)["ID_prior"], EC.pr_gt_full(p, rng)["GT_prior"] if vireo else None,
                    th["th1"], th["th2"])
    cfg._x = x
    x.eps_stop = _eps_for_stops(cfg, x) if cfg.R > 1 else None
    return x


def stop_iterations(form, traces, min_iter, max_iter, eps):
    return [S.replay(form, tr, min_iter, max_iter, eps)[0] for tr in traces]


def pick_eps(form, traces, min_iter, max_iter):
    """an epsilon_conv at which the restarts stop at as many different iterations as they can (by the
    rule rather than at max_iter where there is a choice), half-way between two neighbouring judged
    gains that lie at least 2e-6 |ELBO| apart: a gain is a difference of two bounds, each a float64
    sum of about 1e5 terms (a relative 1e-11 on either side), so neither the oracle's rounding nor
    the device's comes within five orders of magnitude of moving a stop"""
    gains = sorted({float(g) for tr in traces for g in np.diff(tr)[max(min_iter, 0):] if g > 0})
    margin = 1e-6 * max(float(np.abs(tr).max()) for tr in traces)
    best = None
    for lo, hi in zip(gains, gains[1:]):
        if (hi - lo) / 2 < margin:
            continue
        eps = (lo + hi) / 2
        its = stop_iterations(form, traces, min_iter, max_iter, eps)
        score = (len(set(its)), max(its) < max_iter - 1, -max(its))
        if best is None or score > best[0]:
            best = (score, eps, its)
    assert best is not None and best[0][0] >= 2, "the restarts do not stop at different iterations"
    return best[1]


STOP_RULE = (1, 12)       # (min_iter, max_iter) of the batch fit whose slots stop at different iterations


def _eps_for_stops(cfg, x):
    """from the oracle's unruled traces of the start state (behind the prelude)"""
    sysm = System(RefFactory(cfg))
    for c in prelude(cfg):
        _execute(sysm, c, x, _Shadow(cfg), sysm.f.refusals)
    X, _ = sysm.batch.run_iters(STOP_RULE[1], 0)
    return pick_eps(S.VIREO if cfg.kind == "vireo" else S.BMM, list(X), STOP_RULE[0], STOP_RULE[1])


# ------------------------------------------------------------------------------------
# calls
# ------------------------------------------------------------------------------------
class Call:
    """name: the key of the alphabet; fn(system, arguments) -> list of arrays or None; on: the model whose
    ELBO parts the call defines (elbo=True); refused(shadow): the argument check sends it back"""

    def __init__(self, name, fn, on="single", elbo=False, refused=None, note=None):
        self.name, self.fn, self.on, self.elbo, self.note = name, fn, on, elbo, note
        self.refused = refused or (lambda sh: False)

    def __repr__(self):
        return self.name


def _fit_out(out):
    tr, it, fl = out
    if isinstance(tr, list):
        tr = np.concatenate(tr)
    return [np.asarray(tr, dtype=np.float64), np.asarray(it), np.asarray(fl)]


def _fit(on, *a):
    return lambda s, x: _fit_out(getattr(s, on).fit(*a))


def _run(on, *a):
    return lambda s, x: [np.asarray(getattr(s, on).run_iters(*a)[0])]


def _step(on, which):
    return lambda s, x: [np.asarray(getattr(s, on).step(which))]


FIT_MAX = (3, 5, 1e-2)           # never judged (it <= min_iter): runs to max_iter, the shape of a restart's first fit
FIT_STOP = (8, 0, 1e30)          # the rule fires at it = 1, inside the first poll batch of iterations 0 .. 3
FIT_DELAY = (4, 5, 1e-2, 2)      # delay_fit_theta = 2


def _note_prior(which):
    def note(sh, x):
        sh.pri = getattr(x, which)
    return note


def _note_snapshot(sh, x):
    sh.has_snap = True
    sh.snap_now = True


def _note_stage(sh, x):
    sh.reserved = True
    sh.stage[0] = x.staged


def _stage(s, x):
    s.single.stage_reserve()
    s.single.stage_raw(0, *x.staged)
    s.single.set_state_staged(0, *x.theta0)


def single_alphabet(cfg):
    vireo = cfg.kind == "vireo"
    A = [Call("step_theta", _step("single", STEP_THETA))]
    if vireo:
        A.append(Call("step_gt", _step("single", STEP_GT)))
    A += [Call("step_id", _step("single", STEP_ID)),
          Call("step_loglik", _step("single", STEP_LOGLIK)),
          Call("step_softmax", _step("single", STEP_SOFTMAX)),
          Call("step_elbo", _step("single", STEP_ELBO), elbo=True),
          Call("fit_max", _fit("single", *FIT_MAX), elbo=True),
          Call("fit_stop", _fit("single", *FIT_STOP), elbo=True),
          Call("fit_delay", _fit("single", *FIT_DELAY), elbo=True),
          Call("run_2_0", _run("single", 2, 0), elbo=True),
          Call("run_3_1", _run("single", 3, 1), elbo=True),
          Call("set_id", lambda s, x: s.single.set_state(x.other[0], None, None, None))]
    if vireo:
        A.append(Call("set_gt", lambda s, x: s.single.set_state(None, x.other[1], None, None)))
    A += [Call("set_theta", lambda s, x: s.single.set_state(None, None, x.other[2], x.other[3])),
          Call("set_all", lambda s, x: s.single.set_state(*x.other)),
          Call("set_raw", lambda s, x: s.single.set_state_raw(x.raw[0][0], x.raw[0][1], *x.theta0))]
    if vireo:
        A.append(Call("stage", _stage, note=_note_stage))
    A += [Call("prior_full", lambda s, x: s.single.set_prior(*x.full_prior), note=_note_prior("full_prior")),
          Call("prior_default", lambda s, x: s.single.set_prior(*x.default_prior), note=_note_prior("default_prior")),
          Call("snapshot", lambda s, x: s.single.snapshot(), note=_note_snapshot),
          Call("restore", lambda s, x: s.single.restore(), refused=lambda sh: not sh.has_snap),
          Call("set_loglik", lambda s, x: s.single.set_loglik(x.L)),
          # (refused until something has been staged; afterwards a valid call on buffer 0)
          Call("staged_0", lambda s, x: s.single.set_state_staged(0, None, None), refused=lambda sh: not sh.reserved),
          Call("step_unknown", _step("single", STEP_UNKNOWN), refused=lambda sh: True)]
    return A


def batch_alphabet(cfg):
    vireo = cfg.kind == "vireo"
    A = [Call("set_restart_1", lambda s, x: s.batch.set_restart(1, *x.other, raw=False)),
         Call("set_restart_raw_2", lambda s, x: s.batch.set_restart(2, x.raw[0][0], x.raw[0][1], *x.theta0, raw=True)),
         Call("fit_max", _fit("batch", *FIT_MAX), on="batch", elbo=True),
         Call("fit_stop", lambda s, x: _fit_out(s.batch.fit(STOP_RULE[1], STOP_RULE[0], x.eps_stop)), on="batch",
              elbo=True),
         Call("fit_delay", _fit("batch", *FIT_DELAY), on="batch", elbo=True),
         Call("run_2_0", _run("batch", 2, 0), on="batch", elbo=True),
         Call("run_3_1", _run("batch", 3, 1), on="batch", elbo=True),
         Call("step_theta", _step("batch", STEP_THETA), on="batch")]
    if vireo:
        A.append(Call("step_gt", _step("batch", STEP_GT), on="batch"))
    A += [Call("step_id", _step("batch", STEP_ID), on="batch"),
          Call("copy_0", lambda s, x: s.batch.copy_to(s.single, 0)),
          Call("copy_2", lambda s, x: s.batch.copy_to(s.single, 2)),
          Call("step_unknown", _step("batch", STEP_UNKNOWN), on="batch", refused=lambda sh: True)]
    return A


def alphabet(cfg):
    return batch_alphabet(cfg) if cfg.R > 1 else single_alphabet(cfg)


def prelude(cfg):
    """Every sequence starts here.  A refused restore on the model that has nothing saved; a snapshot
    of another state; the start state; then theta, GT, logLik_ID and the ELBO through the step API, which
    leave valid S, W and KL_theta behind (the deferrals of LazyRef are all armed)."""
    P = [Call("prior_default", lambda s, x: s.single.set_prior(*x.default_prior), note=_note_prior("default_prior")),
         Call("restore", lambda s, x: s.single.restore(), refused=lambda sh: not sh.has_snap),
         Call("set_alt", lambda s, x: s.single.set_state(*x.alt)),
         Call("snapshot", lambda s, x: s.single.snapshot(), note=_note_snapshot),
         Call("set_start", lambda s, x: s.single.set_state(*x.start[0])),
         Call("step_theta", _step("single", STEP_THETA))]
    if cfg.kind == "vireo":           # (theta is a function of ID and GT: behind this a second theta step moves it again)
        P.append(Call("step_gt", _step("single", STEP_GT)))
    P += [Call("step_loglik", _step("single", STEP_LOGLIK)),
         Call("step_elbo", _step("single", STEP_ELBO), elbo=True)]
    if cfg.R > 1:
        P.append(Call("batch_prior", lambda s, x: s.batch.set_prior(*x.default_prior)))
        for r in range(cfg.R):
            P.append(Call("set_restart_%d" % r, lambda s, x, r=r: s.batch.set_restart(r, *x.start[r], raw=False)))
        P.append(Call("step_theta", _step("batch", STEP_THETA), on="batch"))
    return P


# ------------------------------------------------------------------------------------
# the executors
# ------------------------------------------------------------------------------------
class _Shadow:
    """the parts of sigma the host follows by itself: priors, what was saved, what was staged"""

    def __init__(self, cfg):
        self.pri = None
        self.has_snap, self.snap_now, self.snap = False, False, None
        self.reserved, self.stage = False, {}
        self.parts_on = None           # the model whose ELBO parts are defined right now


def _execute(sysm, call, x, sh, refusals):
    """one call -> (result, ELBO parts where the call defines them, or a refusal left them defined)"""
    sysm.calls += 1
    if call.refused(sh):
        try:
            call.fn(sysm, x)
        except refusals:
            parts = None
            if sh.parts_on is not None:           # a refused call changes nothing: they are still defined
                parts = np.asarray(getattr(sysm, sh.parts_on).elbo_parts())
            return REFUSED, parts
        raise AssertionError("%s was not refused" % call.name)
    out = call.fn(sysm, x)
    if call.note:
        call.note(sh, x)
    parts = None
    if call.elbo:
        parts = np.asarray(getattr(sysm, call.on).elbo_parts())
        sh.parts_on = call.on
    else:
        sh.parts_on = None
    return out, parts


def read_sigma(sysm):
    """state, logLik_ID, and every slot of the batch (through a model of its own)"""
    sig = SimpleNamespace(state=sysm.single.get_state(), L=sysm.single.get_loglik(), slots=[])
    if sysm.batch is not None:
        for r in range(sysm.cfg.R):
            sysm.batch.copy_to(sysm.probe(), r)
            sig.slots.append(sysm.probe().get_state())
    return sig


def upload_sigma(sysm, sh, sig, x):
    if sh.pri is not None:
        sysm.single.set_prior(*sh.pri)
    if sysm.batch is not None:
        sysm.batch.set_prior(*x.default_prior)
    if sh.has_snap:
        sysm.single.set_state(*sh.snap)
        sysm.single.snapshot()
    if sh.reserved:
        sysm.single.stage_reserve()
        for b, (i, g) in sh.stage.items():
            sysm.single.stage_raw(b, i, g)
    sysm.single.set_state(*sig.state)
    sysm.single.set_loglik(sig.L)
    for r, st in enumerate(sig.slots):
        sysm.batch.set_restart(r, *st, raw=False)


def observe(sysm, sh):
    """everything a caller can see, the saved and the staged content last (reading them overwrites
    the state) -> name -> array"""
    sig = read_sigma(sysm)
    out = dict(zip(("ID", "GT", "mu", "sm"), sig.state), L=sig.L)
    for r, st in enumerate(sig.slots):
        out.update(zip(("ID[%d]" % r, "GT[%d]" % r, "mu[%d]" % r, "sm[%d]" % r), st))
    if sh.has_snap:
        sysm.single.restore()
        out.update(zip(("snap_ID", "snap_GT", "snap_mu", "snap_sm"), sysm.single.get_state()))
    for b in sorted(sh.stage):
        sysm.single.set_state_staged(b, None, None)
        out.update(zip(("stage%d_ID" % b, "stage%d_GT" % b), sysm.single.get_state()[:2]))
    return {k: v for k, v in out.items() if v is not None}


class Trail:
    """what a run returned, call by call, and what it left visible"""

    def __init__(self):
        self.results, self.parts, self.after_refusal, self.seen = [], [], [], None


def _record(trail, call, out, parts, sh):
    trail.results.append(out)
    refused = out is REFUSED
    trail.parts.append(None if refused else parts)
    trail.after_refusal.append(parts if refused else None)


def run(factory, seq, x, sysm=None, sh=None, watch=True):
    """the sequence on ONE system, as a caller makes it -> Trail"""
    own = sysm is None
    sysm = sysm or System(factory)
    sh = sh or _Shadow(factory.cfg)
    t = Trail()
    try:
        for call in seq:
            out, parts = _execute(sysm, call, x, sh, factory.refusals)
            _record(t, call, out, parts, sh)
        if watch:
            t.seen = observe(sysm, sh)
    finally:
        t.calls = sysm.calls
        if own:
            sysm.close()
    t.system, t.shadow = (None, None) if own else (sysm, sh)
    return t


def twin(factory, seq, x, start=None):
    """the same sequence, every call on a FRESH system that was given sigma: after each call sigma is
    read back, the system closed, a new one made and sigma uploaded.  What was saved and staged is
    kept on the host and replayed.  start = (sigma, shadow): begin from an uploaded sigma."""
    t = Trail()
    calls = 0
    sysm = System(factory)
    if start is None:
        sh = _Shadow(factory.cfg)
    else:
        sig, sh = start[0], copy.copy(start[1])
        sh.stage, sh.parts_on = dict(sh.stage), None
        upload_sigma(sysm, sh, sig, x)
    try:
        for k, call in enumerate(seq):
            sh.snap_now = False
            out, parts = _execute(sysm, call, x, sh, factory.refusals)
            _record(t, call, out, parts, sh)
            if k + 1 == len(seq):
                break
            sig = read_sigma(sysm)
            if sh.snap_now:
                sh.snap = sig.state
            calls += sysm.calls
            sysm.close()
            sysm = System(factory)
            sh.parts_on = None             # (the parts are no part of sigma: a fresh system has none)
            upload_sigma(sysm, sh, sig, x)
        if sh.snap_now:
            sh.snap = read_sigma(sysm).state
        t.sigma, t.shadow = read_sigma(sysm), sh
        t.seen = observe(sysm, sh)
    finally:
        t.calls = calls + sysm.calls
        sysm.close()
    return t


# ------------------------------------------------------------------------------------
# the judges
# ------------------------------------------------------------------------------------
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.shape, a.dtype.str, a.tobytes()


def same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, str) or isinstance(b, str):
        return a == b
    return _bits(np.asarray(a)) == _bits(np.asarray(b))


def differences(one, two, last_only=False):
    """property 1: the names of what differs in any bit between two trails of one sequence (last_only: of
    two sequences that end in the same call, that call alone).  The parts
    read behind a refusal belong to the history, not to sigma: a twin has none, they are not compared."""
    bad = []
    assert last_only or len(one.results) == len(two.results)
    for k in ((-1,) if last_only else range(len(one.results))):
        a, b = one.results[k], two.results[k]
        if (a is None) != (b is None) or (a is REFUSED) != (b is REFUSED) or (a is not None and a is not REFUSED and (
                len(a) != len(b) or not all(same_bits(p, q) for p, q in zip(a, b)))):
            bad.append("result[%d]" % k)
        if not same_bits(one.parts[k], two.parts[k]):
            bad.append("parts[%d]" % k)
    if one.seen is not None and two.seen is not None:
        assert sorted(one.seen) == sorted(two.seen), (sorted(one.seen), sorted(two.seen))
        bad += [k for k in one.seen if not same_bits(one.seen[k], two.seen[k])]
    return bad


def _rel(a, b, atol):
    """the largest |a - b| / |b| beyond atol (np.testing.assert_allclose's measure); inf where the
    shapes, the non-finite entries or the integers differ"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return np.inf
    if a.dtype.kind in "iu" or b.dtype.kind in "iu":
        return 0.0 if np.array_equal(a, b) else np.inf
    fin = np.isfinite(a) & np.isfinite(b)
    if not np.array_equal(a[~fin], b[~fin], equal_nan=True):
        return np.inf
    d = np.abs(a[fin] - b[fin])
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(d <= atol, 0.0, d / np.abs(b[fin]))
    return float(q.max()) if q.size else 0.0


def part_floors(cfg, N, M):
    """What float64 can hold of KL_ID and KL_GT, as absolute floors of (LB_p, KL_ID, KL_GT, KL_theta).
    Each is a sum of p * (log p - log q) over rows that sum to one; a term carries an absolute error
    of about eps * p * (|log p| + |log q|), a row of width w about eps * 2 * log w, and the first
    order of the terms cancels: while a posterior still sits at its prior (the first iterations of a
    random start under the uniform ID prior) the sum is a second-order residue of 1e-11 that neither
    the oracle nor the device can hold to a relative 1e-5.  Two such sums are compared: twice that."""
    eps = np.finfo(np.float64).eps
    return np.array([0.0, 2 * eps * M * 2 * np.log(max(cfg.K, 2)),
                     2 * eps * N * cfg.K * 2 * np.log(max(cfg.T, 2)), 0.0])


def _rel_parts(a, b, atol, floors):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if floors is None or a.shape != b.shape:
        return _rel(a, b, atol)
    return max(_rel(a[..., k], b[..., k], max(atol, floors[k])) for k in range(4))


def distance(got, ref, atol, floors=None):
    """property 2: the largest relative distance between what a run returned and showed and what the
    oracle's run of the same sequence holds -> (distance, the name it sits at).  floors: part_floors."""
    worst, where = 0.0, None

    def take(d, name):
        nonlocal worst, where
        if d > worst:
            worst, where = d, name
    assert len(got.results) == len(ref.results)
    for k, (a, b) in enumerate(zip(got.results, ref.results)):
        if (a is None) != (b is None) or (a is REFUSED) != (b is REFUSED):
            take(np.inf, "result[%d]" % k)
        elif a is not None and a is not REFUSED:
            if len(a) != len(b):
                take(np.inf, "result[%d]" % k)
            for p, q in zip(a, b):
                take(_rel(p, q, atol), "result[%d]" % k)
        for pa, pb, tag in ((got.parts[k], ref.parts[k], "parts"),
                            (got.after_refusal[k], ref.after_refusal[k], "parts behind the refusal")):
            if (pa is None) != (pb is None):
                take(np.inf, "%s[%d]" % (tag, k))
            elif pa is not None:
                take(_rel_parts(pa, pb, atol, floors), "%s[%d]" % (tag, k))
    if got.seen is not None:
        assert sorted(got.seen) == sorted(ref.seen), (sorted(got.seen), sorted(ref.seen))
        for k in got.seen:
            take(_rel(got.seen[k], ref.seen[k], atol), k)
    return worst, where


# ------------------------------------------------------------------------------------
# the families
# ------------------------------------------------------------------------------------
def pairs_from(cfg, first):
    """family 1, the share of one first call: (a, b) for every b of the alphabet"""
    A = alphabet(cfg)
    a = next(c for c in A if c.name == first)
    return [(a, b) for b in A]


WALKS, WALK_LEN = 8, 12


WALK_SEED = 27


def is_compute(call):
    return call.name.split("_")[0] in ("step", "fit", "run") and call.name != "step_unknown"


def walks(cfg, seed=None):
    """family 3: seeded walks over the alphabet, a call that computes and one that does not in turn
    (uploads, priors, snapshot and restore, copies, refusals: what touches a flag sits between the
    kernels that set and read it).  A refusal that is no longer one is a valid call.  WALK_SEED is the
    first base seed at which the walks of the CPU configurations catch every planted defect of
    LazyRef (tests/test_model_sequences_cpu.py holds that they do)."""
    A = alphabet(cfg)
    halves = [c for c in A if is_compute(c)], [c for c in A if not is_compute(c)]
    rng = np.random.default_rng((WALK_SEED if seed is None else seed) + sum(map(ord, cfg.name)))
    return [[halves[k % 2][rng.integers(0, len(halves[k % 2]))] for k in range(WALK_LEN)] for _ in range(WALKS)]


# production, shortened: a restart's first fit runs 8 iterations at most (max_iter_init = 20 in vireo_wrap.py:23),
# the winner's refinement 12 (200 in restarts.py, winner); clone mode 8 and 12 at min_iter = 3
# (100 / 200 at min_iter = 20 in bmm_model.py:204)
PROD_FIT, PROD_REFINE = (8, 5, 1e-2, 3), (12, 5, 1e-2, 0)
CLONE_FIT, CLONE_REFINE = (8, 3, 1e-2), (12, 3, 1e-2)


def _best_so_far(elbos):
    """which restarts ``_argmax_takes`` / ``_is_record`` snapshot: every strict new maximum"""
    out, best = [], None
    for e in elbos:
        out.append(best is None or e > best)
        best = e if out[-1] else best
    return out


def _get_state(s, x):
    return [a for a in s.single.get_state() if a is not None]


def _push_pulled(s, x):
    """BinomMixtureVB.fit behind its restore: _pull, set_initial (which normalises ID_prob again), _push"""
    ID, _, mu, sm = s.single.get_state()
    s.single.set_state(O.unit_sum(ID), None, mu, sm)


def production(cfg):
    """family 2 -> {name: sequence}.  Which restarts are a new best, and so get a snapshot, is decided
    by the oracle's ELBOs once (the sequences are fixed lists)."""
    x = arguments(cfg)
    ref = RefFactory(cfg)
    vireo = cfg.kind == "vireo"
    out = {}
    snap = Call("snapshot", lambda s, x: s.single.snapshot(), note=_note_snapshot)
    restore = Call("restore", lambda s, x: s.single.restore(), refused=lambda sh: not sh.has_snap)
    get = Call("get_state", _get_state)
    if vireo and cfg.R == 1:
        # DeviceRestarts.run x 3, winner(refine=True): fixed arrays first, then the raw draws; the second
        # restart arrives through a staging buffer (not with a fixed GT: staging carries both arrays)
        fixed_gt = not cfg.learn_gt

        def upload(i):
            ID, GT = x.raw[i]
            if fixed_gt:
                return [Call("set_fixed", lambda s, x: s.single.set_state(None, x.alt[1], None, None)),
                        Call("set_raw", lambda s, x, ID=ID: s.single.set_state_raw(ID, None, *x.theta0))]
            if i == 1:
                def note(sh, x, ID=ID, GT=GT):
                    sh.reserved, sh.stage[1] = True, (ID, GT)
                return [Call("stage_reserve", lambda s, x: s.single.stage_reserve(),
                             note=lambda sh, x: setattr(sh, "reserved", True)),
                        Call("stage_raw", lambda s, x, ID=ID, GT=GT: s.single.stage_raw(1, ID, GT), note=note),
                        Call("set_staged", lambda s, x: s.single.set_state_staged(1, *x.theta0))]
            return [Call("set_raw", lambda s, x, ID=ID, GT=GT: s.single.set_state_raw(ID, GT, *x.theta0))]
        fit = Call("fit", _fit("single", *PROD_FIT), elbo=True)
        sysm, sh, elbos = System(ref), _Shadow(cfg), []
        sysm.single.set_prior(*x.default_prior)
        for i in range(3):
            for c in upload(i) + [fit]:
                res, _ = _execute(sysm, c, x, sh, ref.refusals)
            elbos.append(res[0][int(res[1]) - 1])             # ELBO_[-1] = trace[:it][-1]
        seq = [prelude(cfg)[0]]
        for i, new in enumerate(_best_so_far(elbos)):
            seq += upload(i) + [fit] + ([snap] if new else [])
        out["run_x3_winner"] = seq + [restore, Call("refine", _fit("single", *PROD_REFINE), elbo=True), get]
    elif vireo:
        # DeviceRestarts.submit x 3, _fit_pending, winner(refine=True): the slots stop at different iterations
        ups = [Call("set_restart_raw_%d" % r,
                    lambda s, x, r=r: s.batch.set_restart(r, x.raw[r][0], x.raw[r][1], *x.theta0, raw=True))
               for r in range(3)]
        head = [prelude(cfg)[0], Call("batch_prior", lambda s, x: s.batch.set_prior(*x.default_prior))]
        sysm = System(ref)
        sh = _Shadow(cfg)
        for c in head + ups:
            _execute(sysm, c, x, sh, ref.refusals)
        n = 14
        X, _ = sysm.clone().batch.run_iters(n, 3)
        eps = pick_eps(S.VIREO, list(X), 5, n)
        its = stop_iterations(S.VIREO, list(X), 5, n, eps)
        assert len(set(its)) >= 2
        elbos = [X[r][its[r] - 1] for r in range(3)]
        seq = head + ups + [Call("fit", lambda s, x, eps=eps: _fit_out(s.batch.fit(n, 5, eps, 3)), on="batch", elbo=True)]
        for r, new in enumerate(_best_so_far(elbos)):
            if new:
                seq += [Call("copy_%d" % r, lambda s, x, r=r: s.batch.copy_to(s.single, r)), snap]
        out["submit_x3_winner"] = seq + [restore, Call("refine", _fit("single", *PROD_REFINE), elbo=True), get]
    else:
        # BinomMixtureVB.fit, one model: set_initial + _fit_BV (push, fit, pull) x 3, the best is kept in
        # the snapshot; then restore, pull, set_initial, push, the final fit, pull
        ups = [Call("push_%d" % i, lambda s, x, i=i: s.single.set_state(O.unit_sum(x.raw[i][0]), None, *x.theta0))
               for i in range(3)]
        fit = Call("fit", _fit("single", *CLONE_FIT), elbo=True)
        sysm, sh, elbos = System(ref), _Shadow(cfg), []
        sysm.single.set_prior(*x.default_prior)
        for i in range(3):
            for c in [ups[i], fit]:
                res, _ = _execute(sysm, c, x, sh, ref.refusals)
            elbos.append(res[0][int(res[1]) - 1])
        seq = [prelude(cfg)[0]]
        for i, new in enumerate(_best_so_far(elbos)):
            seq += [ups[i], fit, get] + ([snap] if new else [])
        out["clone_inits_x3"] = seq + [restore, Call("push_pulled", _push_pulled),
                                       Call("final", _fit("single", *CLONE_REFINE), elbo=True), get]
    return out
