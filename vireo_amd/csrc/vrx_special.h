// Special functions of the Beta posteriors, shared by the kernels of vrx_kernels.h and vrx_varmix.h.
#pragma once

#include <hip/hip_runtime.h>

// ------------------------------------------------------------------------------------
// special functions
// ------------------------------------------------------------------------------------
// digamma for x > 0: upward recurrence to x >= 10, then the asymptotic series
// ln x - 1/(2x) - sum B_2k / (2k x^2k)  (the classic Cephes scheme scipy.special.digamma
// uses away from its root; absolute accuracy ~1e-15 on the Beta shapes met here).
__device__ __forceinline__ double vrx_digamma(double x) {
    if (!(x > 0.0)) return __builtin_nan("");
    double w = 0.0;
    while (x < 10.0) {
        w += 1.0 / x;
        x += 1.0;
    }
    const double z = 1.0 / (x * x);
    double y = 8.33333333333333333333e-2;
    y = y * z - 2.10927960927960927961e-2;
    y = y * z + 7.57575757575757575758e-3;
    y = y * z - 4.16666666666666666667e-3;
    y = y * z + 3.96825396825396825397e-3;
    y = y * z - 8.33333333333333333333e-3;
    y = y * z + 8.33333333333333333333e-2;
    return log(x) - 0.5 / x - y * z - w;
}

__device__ __forceinline__ double vrx_betaln(double a, double b) {
    return lgamma(a) + lgamma(b) - lgamma(a + b);
}

// KL( Beta(p1,p2) || Beta(q1,q2) ), term order of vireoSNP/utils/vireo_base.py:96-125
// (cross(p,q) - cross(p,p)); d1,d2,ds are digamma(p1), digamma(p2), digamma(p1+p2).
__device__ __forceinline__ double vrx_beta_kl(double p1, double p2, double q1, double q2,
                                              double d1, double d2, double ds) {
    const double cq = vrx_betaln(q1, q2) - (q1 - 1.0) * d1 - (q2 - 1.0) * d2 +
                      ((q1 + q2) - 2.0) * ds;
    const double cp = vrx_betaln(p1, p2) - (p1 - 1.0) * d1 - (p2 - 1.0) * d2 +
                      ((p1 + p2) - 2.0) * ds;
    return cq - cp;
}
