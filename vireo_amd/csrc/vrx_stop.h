// The stop rule of every fit loop, once, for host and device.
//
// Each loop of the reference has the shape
//     X = np.zeros(max_iter)
//     for it in range(max_iter):
//         ...; X[it] = bound
//         if it > min_iter:
//             if   <X decreased>:              warn
//             elif it == max_iter - 1:         warn "did not converge"
//             elif X[it] - X[it - 1] < eps:    break
// and the loops differ in the "decreased" test alone.  vrx_stop_judge restates that block in the reference's
// order of comparisons, vrx_stop_prev restates what X[it - 1] holds.  Plain comparisons of doubles: a NaN makes
// each of them false (the loop goes on), nothing here reads memory, nothing is rearranged -- the two
// subtracting forms below differ by a rounding, which is why they are kept apart.
#pragma once

#if defined(__HIPCC__)
#define VRX_STOP_FN __host__ __device__ inline
#else
#define VRX_STOP_FN inline
#endif

// ---- the three "decreased" tests -----------------------------------------------------------------------------------
#define VRX_STOP_VIREO 0  // vireo_model.py:266-274   ELBO[it] < ELBO[it - 1] - numerical_minimal
#define VRX_STOP_BMM 1    // bmm_model.py:190-199     ELBO[it] - ELBO[it - 1] < -1e-6
#define VRX_STOP_EM 2     // vireo_bulk.py:97-105, vireo_doublet.py:173-181   logLik[it] < logLik[it - 1]

// ---- the verdicts --------------------------------------------------------------------------------------------------
#define VRX_STOP_CONTINUE 0
#define VRX_STOP_WARN_DECREASED 1      // the first branch: warn, go on (warn bit 1)
#define VRX_STOP_WARN_NOT_CONVERGED 2  // the second: warn, the loop ends by itself (warn bit 2)
#define VRX_STOP_STOP 3                // the third: break

#define VRX_STOP_NUMERICAL_MINIMAL 1e-6  // vireo_model.py:256, written out in bmm_model.py:191

// model kind (VRX_KIND_VIREO 0, VRX_KIND_BMM 1 of vireo_hip.h) -> form
VRX_STOP_FN int vrx_stop_form_of_kind(int kind) { return kind == 1 ? VRX_STOP_BMM : VRX_STOP_VIREO; }

// The value of the reference's X[it - 1] when X[it] = cur has just been written.  it >= 1: the entry before,
// which the caller hands in (trace_prev; at it == 0 the caller passes anything and reads nothing).  it == 0:
// Python's X[-1], the last entry of np.zeros(max_iter) -- still 0, or X[0] itself when max_iter == 1.
VRX_STOP_FN double vrx_stop_prev(int it, int max_iter, double trace_prev, double cur) {
    if (it >= 1) return trace_prev;
    return max_iter == 1 ? cur : 0.0;
}

VRX_STOP_FN int vrx_stop_judge(int form, int it, int min_iter, int max_iter, double eps, double prev, double cur) {
    if (!(it > min_iter)) return VRX_STOP_CONTINUE;
    bool decreased;
    if (form == VRX_STOP_VIREO)
        decreased = cur < prev - VRX_STOP_NUMERICAL_MINIMAL;
    else if (form == VRX_STOP_BMM)
        decreased = cur - prev < -VRX_STOP_NUMERICAL_MINIMAL;
    else
        decreased = cur < prev;
    if (decreased) return VRX_STOP_WARN_DECREASED;
    if (it == max_iter - 1) return VRX_STOP_WARN_NOT_CONVERGED;
    if (cur - prev < eps) return VRX_STOP_STOP;
    return VRX_STOP_CONTINUE;
}
