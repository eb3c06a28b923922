// Per-variant clone mixtures (vrx_varmix_*): BinomMixtureVB._fit_BV (vireoSNP/utils/bmm_model.py:178-201)
// on every variant's own 1 x n_cell row, all rows in one launch, plus the closed form of the same bound
// with one component.  Included by vrx_varmix.hip only.
//
// The model on one row (default priors Beta(1, 1), uniform ID prior, fix_beta_sum = False), per iteration:
//   update_theta_size (:133-144)   s1_k = 1 + sum_i a_i ID_ik, s2_k = 1 + sum_i b_i ID_ik; beta_mu = s1 / (s1 + s2),
//                                  beta_sum = s1 + s2; the shapes used below are beta_mu * beta_sum and
//                                  (1 - beta_mu) * beta_sum, as the reference's properties form them (:107-115)
//   get_E_logLik (:118-130)        L_ik = a_i psi(s1_k) + b_i psi(s2_k) - d_i psi(s1_k + s2_k)
//   update_ID_prob (:147-154)      ID_ik = exp(L_ik - max_k L_ik) / sum_k (the uniform prior cancels)
//   get_ELBO (:157-175)            sum L ID - sum_i KL(ID_i || 1/K) - sum_k KL(Beta(s1_k, s2_k) || Beta(1, 1))
// and the stop rule of :190-199.  A cell without reads has L = 0, ID = 1/K and adds exactly nothing to any
// sum, so a row is the list of its covered cells' (ad, dp) pairs and nothing else: no cell index.
//
// One pass over the row per iteration; ID_prob is never stored.  A pass with the shapes of iteration `it`
// forms every entry's L and softmax in registers and accumulates, per component, sum a ID, sum b ID (the next
// shapes) and sum ID (the size), and sum L ID and the assignment KL of this iteration.  log ID_ik is taken as
// (L_ik - max) - log(sum_k exp): one log per entry.  Pass 0 forms the first sums from the start values
//   w_k = max(0, 1 - |a / d - k / (K - 1)| (K - 1)) + 1/64,  ID = w / sum w  (normalised once more, as
// set_initial does, :80-81), evaluated from (a, d) on the fly.  The 3 K digammas of an iteration are
// computed by lanes 0 .. 3 K - 1, the K Beta KL terms by lanes 0 .. K - 1, and read back lane by lane into
// wave-uniform values.  K is a template parameter: every per-component array is registers.
//
// Work unit by row length alone: a row of at most VRX_VM_WAVE_ROWS entries is fitted by one wave (four rows
// per workgroup), a longer one by a workgroup of 256 threads.  Thread t of the unit takes the entry pairs
// t, t + T, t + 2 T, ... (T = 64 or 256; a pair is one 16-byte load), so a wave of a workgroup owns fixed
// 128-entry chunks.  Every sum is lane-sequential, then the wave butterfly, then (workgroup) the four waves'
// values from LDS in wave order: no atomics, and a row's results are a function of its entries and the
// call's parameters only -- not of the other rows of the call, their order, or the run.  The stop rule is
// evaluated on values every lane of the unit holds equal, so a finished row's wave or workgroup simply
// returns.  The launch takes the rows longest first (perm).
#pragma once

#include "vrx_common.h"
#include "vrx_special.h"
#include "vrx_stop.h"

constexpr int VRX_VM_BLOCK = 256;  // threads of a workgroup: four rows by wave, or one long row
constexpr int VRX_VM_WAVES = VRX_VM_BLOCK / 64;
constexpr int VRX_VM_WAVE_ROWS = 512;  // longest row fitted by one wave
constexpr int VRX_VM_MIN_K = 2, VRX_VM_MAX_K = 8;

#pragma clang fp contract(off)

__device__ __forceinline__ double vrx_vm_lane(double v, int lane) {  // lane: a compile-time constant
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double vrx_vm_wave_sum(double v) {  // all 64 lanes, converged
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);  // (a + b == b + a: every lane ends equal)
    return v;
}

// Sum the first NV values over the unit; every lane of the unit ends with the same bits.  xch: 2 x 4 x NVMAX
// doubles of LDS, the halves used in turn (a wave may still read one half while another wave, one
// reduction ahead, writes the other; two ahead is behind the barrier in between).
template <int NV, int NVMAX, int N>
__device__ __forceinline__ void vrx_vm_reduce(double (&v)[N], bool block, double* xch, int& phase) {
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = vrx_vm_wave_sum(v[i]);
    if (block) {  // (uniform over the workgroup)
        double* buf = xch + (phase & 1) * (VRX_VM_WAVES * NVMAX);
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < NV; ++i) buf[wave * NVMAX + i] = v[i];
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            double r = buf[i];
#pragma unroll
            for (int w = 1; w < VRX_VM_WAVES; ++w) r += buf[w * NVMAX + i];
            v[i] = r;
        }
        ++phase;
    }
}

// the start values of one entry: acc = A[K] | B[K] | sum a | sum b
template <int K, int N>
__device__ __forceinline__ void vrx_vm_init_entry(int a, int d, double (&acc)[N]) {
    const double da = (double)a, db = (double)(d - a);
    const double f = da / (double)d;
    double w[K];
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double c = (double)k / (double)(K - 1);
        w[k] = fmax(0.0, 1.0 - fabs(f - c) * (double)(K - 1)) + 0.015625;
        s += w[k];
    }
    double s2 = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        w[k] = w[k] / s;
        s2 += w[k];
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double id = w[k] / s2;
        acc[k] += da * id;
        acc[K + k] += db * id;
    }
    acc[2 * K] += da;
    acc[2 * K + 1] += db;
}

// one entry of an iteration's pass: acc = A[K] | B[K] | size[K] | sum L ID | sum KL(ID || 1/K)
template <int K, int N>
__device__ __forceinline__ void vrx_vm_entry(int a, int d, const double (&p1)[K], const double (&p2)[K],
                                             const double (&ps)[K], double log_k, double (&acc)[N]) {
    const double da = (double)a, db = (double)(d - a), dd = (double)d;
    double L[K];
    double mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        L[k] = da * p1[k] + db * p2[k] - dd * ps[k];
        mx = fmax(mx, L[k]);
    }
    double e[K];
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        e[k] = exp(L[k] - mx);
        s += e[k];
    }
    const double log_s = log(s);
    double lb = 0.0, kl = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double id = e[k] / s;
        lb += L[k] * id;
        kl += id * (((L[k] - mx) - log_s) + log_k);  // rel_entr(0, q) = 0: id = 0 gives 0 * finite
        acc[k] += da * id;
        acc[K + k] += db * id;
        acc[2 * K + k] += id;
    }
    acc[3 * K] += lb;
    acc[3 * K + 1] += kl;
}

// One theta step from the sums a wave left in its LDS block: shapes, digammas and the Beta KL of the K
// components, and beside them the one-component model on the row totals ta, tb (n_donor = 1: ID = 1, so
// _fit_BV records sum_i L_i - KL(Beta(s1, s2) || Beta(1, 1)) at every iteration).  Lane 3 k + r takes the
// r-th digamma of component k, lane k its KL; component K is the one-component model.  A lane keeps its own
// component's shapes while the unrolled loop passes them: no array is indexed by a lane number.
// Not inlined: the constants of lgamma and digamma would otherwise live in scalar registers across the
// whole fit, where exp and log need theirs.  In a workgroup each of the four waves runs the step itself on the
// same sums (same bits): once per wave, which saves a barrier and a broadcast through LDS.
//   w (doubles, one block per wave):  in  A[K] | B[K] | ta | tb
//                                     out psi(s1)[K] | psi(s2)[K] | psi(s1 + s2)[K] | beta_mu[K] | beta_sum[K] |
//                                         sum_k KL | one-component bound
// Orders the LDS accesses of the lanes of one wave (a lane reads what another lane of its wave wrote): a
// release / acquire pair at wavefront scope and a scheduling barrier; no instruction beyond the waits.
__device__ __forceinline__ void vrx_vm_wave_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int K>
struct VrxVmLds {
    enum { A = 0, B = K, TA = 2 * K, TB = 2 * K + 1, P1 = 2 * K + 2, P2 = 3 * K + 2, PS = 4 * K + 2, MU = 5 * K + 2,
           SM = 6 * K + 2, KL = 7 * K + 2, ONE = 7 * K + 3, WORDS = 7 * K + 4 };
};

template <int K>
__device__ __noinline__ void vrx_vm_theta(double* w, int lane) {
    typedef VrxVmLds<K> O;
    const int j = lane < 3 * (K + 1) ? lane : 0;
    const int kd = j / 3, r = j - 3 * kd;
    const int kc = lane <= K ? lane : 0;
    const double ta = w[O::TA], tb = w[O::TB];
    double x = 1.0, y = 1.0, cx = 1.0, cy = 1.0;
#pragma unroll
    for (int k = 0; k <= K; ++k) {
        const double s1 = (k < K ? w[O::A + k] : ta) + 1.0, s2 = (k < K ? w[O::B + k] : tb) + 1.0;
        const double s = s1 + s2, m = s1 / s;
        const double t1 = m * s, t2 = (1.0 - m) * s;
        if (k < K && lane == 0) {
            w[O::MU + k] = m;
            w[O::SM + k] = s;
        }
        x = kd == k ? t1 : x;
        y = kd == k ? t2 : y;
        cx = kc == k ? t1 : cx;
        cy = kc == k ? t2 : cy;
    }
    const double dg = vrx_digamma(r == 0 ? x : r == 1 ? y : x + y);
    if (lane < 3 * K) w[O::P1 + r * K + kd] = dg;  // (P1, P2, PS are K apart; read after the caller's fence)
    const double kl = vrx_beta_kl(cx, cy, 1.0, 1.0, __shfl(dg, 3 * kc), __shfl(dg, 3 * kc + 1), __shfl(dg, 3 * kc + 2));
    double kl_theta = 0.0;
#pragma unroll
    for (int q = 0; q < K; ++q) kl_theta += vrx_vm_lane(kl, q);
    const double d1 = vrx_vm_lane(dg, 3 * K), d2 = vrx_vm_lane(dg, 3 * K + 1), ds = vrx_vm_lane(dg, 3 * K + 2);
    if (lane == 0) {
        w[O::KL] = kl_theta;
        w[O::ONE] = (ta * d1 + tb * d2 - (ta + tb) * ds) - vrx_vm_lane(kl, K);
    }
}

// Read from device memory where it is needed: as kernel arguments the seventeen words would sit in scalar
// registers from entry to exit, beside the constants of exp and log.
struct VrxVmArgs {
    int64_t n_var, n_long;
    const int32_t* perm;   // rows, longest first; the first n_long are longer than VRX_VM_WAVE_ROWS
    const int64_t* start;  // first entry of a row in `pairs` (even)
    const int32_t* len;
    const int4* pairs;     // (ad, dp) (ad, dp): two entries per element, rows padded to whole elements
    int max_iter, min_iter;
    double eps;
    double *elbo_k, *elbo_one, *mu, *sum, *size;  // outputs by row
    int32_t *n_iter, *warn;
    double* trace;  // n_var x max_iter or null
};

// A workgroup of the first n_long fits one long row; every other workgroup fits four rows, one per wave.  One
// code path: `block` (uniform over the workgroup) only sets the stride of the entry loop and sends the sums
// through LDS.
template <int K>
__global__ __launch_bounds__(VRX_VM_BLOCK) void vrx_varmix_fit_k(const VrxVmArgs* __restrict__ g) {
    constexpr int NV = 3 * K + 2;
    typedef VrxVmLds<K> O;
    __shared__ double xch[2 * VRX_VM_WAVES * NV];
    __shared__ double theta[VRX_VM_WAVES * O::WORDS];
    double* w = theta + (threadIdx.x >> 6) * O::WORDS;  // this wave's block: waves never share one
    const int lane = threadIdx.x & 63;
    const bool block = (int64_t)blockIdx.x < g->n_long;
    const int64_t at = block ? (int64_t)blockIdx.x
                             : g->n_long + ((int64_t)blockIdx.x - g->n_long) * VRX_VM_WAVES + (threadIdx.x >> 6);
    if (at >= g->n_var) return;  // (whole waves of a workgroup that fits by wave: no barrier follows for them)
    const int64_t v = g->perm[at];
    const int nt = block ? VRX_VM_BLOCK : 64;
    const int t = block ? (int)threadIdx.x : lane;
    const int n = g->len[v];
    const int n_pair = (n + 1) >> 1;
    const int4* row = g->pairs + (g->start[v] >> 1);
    int phase = 0;
    double acc[NV];

    // pass 0: the first sums from the start values, and the row totals of the one-component bound
#pragma unroll
    for (int i = 0; i < NV; ++i) acc[i] = 0.0;
    for (int p = t; p < n_pair; p += nt) {
        const int4 q = row[p];
        vrx_vm_init_entry<K>(q.x, q.y, acc);
        if (2 * p + 1 < n) vrx_vm_init_entry<K>(q.z, q.w, acc);
    }
    vrx_vm_reduce<2 * K + 2, NV>(acc, block, xch, phase);
    if (lane == 0) {
        w[O::TA] = acc[2 * K];
        w[O::TB] = acc[2 * K + 1];
    }
    vrx_vm_wave_fence();

    const double log_k = log((double)K);
    double prev = 0.0;
    int warn = 0, it = 0;
    for (;; ++it) {
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < 2 * K; ++i) w[O::A + i] = acc[i];
        }
        vrx_vm_wave_fence();  // the lanes read what lane 0 wrote, and below what the theta step's lanes wrote
        vrx_vm_theta<K>(w, lane);
        vrx_vm_wave_fence();
        double p1[K], p2[K], ps[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            p1[k] = w[O::P1 + k];
            p2[k] = w[O::P2 + k];
            ps[k] = w[O::PS + k];
        }
        const double kl_theta = w[O::KL];
#pragma unroll
        for (int i = 0; i < NV; ++i) acc[i] = 0.0;
        for (int p = t; p < n_pair; p += nt) {
            const int4 q = row[p];
            vrx_vm_entry<K>(q.x, q.y, p1, p2, ps, log_k, acc);
            if (2 * p + 1 < n) vrx_vm_entry<K>(q.z, q.w, p1, p2, ps, log_k, acc);
        }
        vrx_vm_reduce<NV, NV>(acc, block, xch, phase);
        const double elbo = acc[3 * K] - acc[3 * K + 1] - kl_theta;
        if (g->trace && t == 0) g->trace[v * g->max_iter + it] = elbo;
        bool stop = it == g->max_iter - 1;
        // bmm_model.py:190-199, in its order of comparisons
        const int verdict = vrx_stop_judge(VRX_STOP_BMM, it, g->min_iter, g->max_iter, g->eps,
                                           vrx_stop_prev(it, g->max_iter, prev, elbo), elbo);
        if (verdict == VRX_STOP_WARN_DECREASED)
            warn |= 1;
        else if (verdict == VRX_STOP_WARN_NOT_CONVERGED)
            warn |= 2;
        else if (verdict == VRX_STOP_STOP)
            stop = true;
        if (stop) break;  // (uniform over the unit)
        prev = elbo;
    }
    // ELBO_iters[-1] is ELBO[it - 1]: the last value computed is dropped by ELBO[:it] (:201)
    if (t == 0) {
        g->elbo_k[v] = prev;
        g->elbo_one[v] = w[O::ONE];
        g->n_iter[v] = it;
        g->warn[v] = warn;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            g->mu[v * K + k] = w[O::MU + k];
            g->sum[v * K + k] = w[O::SM + k];
            g->size[v * K + k] = acc[2 * K + k];
        }
    }
}
