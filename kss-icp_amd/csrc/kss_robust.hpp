// kss_robust.hpp -- robust ICP: the M-estimator weight and the per-pass scale, ONE body each for the device
// kernels (kss_pair.hip, kss_pairb.hip through kss_pair_device.hpp) and the C-ABI's host helpers (kss_robust_weight, kss_robust_scale2).
// f64 +, -, *, / and one sqrt (Huber); nothing here can be contracted into an fma.
#pragma once
#include <hip/hip_runtime.h>

#include "kss_internal.hpp"

namespace kss {

// Weight of the squared residual x under `loss` with squared scale c2 (the definition at kss_icp_robust in include/kssicp.h).
// kept: whether a candidate with this x counts into cnt and the sums -- "w is finite and greater than 0" decided by compares
// alone (no division: the count cannot depend on how a quotient rounds).  The two agree wherever c2 / x does not underflow
// to 0 and x / c2 does not overflow, i.e. for every x a float residual can give once c2 >= 2^-768.
__host__ __device__ inline double robust_weight_of(int loss, double x, double c2, bool& kept) {
    const double inf = __builtin_huge_val();
    if (loss == KSS_LOSS_L2) { kept = true; return 1.0; }
    if (c2 == 0.0) { kept = x == 0.0; return kept ? 1.0 : 0.0; }
    const bool c2_ok = c2 == c2;   // (a NaN scale keeps nothing)
    if (loss == KSS_LOSS_HUBER) {
        kept = c2_ok && (x <= c2 || x < inf);
        return x <= c2 ? 1.0 : sqrt(c2 / x);
    }
    const double u2 = x / c2;
    if (loss == KSS_LOSS_TUKEY) {
        kept = x < c2;
        const double a = 1.0 - u2;
        return x < c2 ? a * a : 0.0;
    }
    kept = c2_ok && x < inf;   // Cauchy
    return 1.0 / (1.0 + u2);
}

// c2 of the automatic form from the median key widened to f64 (point metric: a squared distance; plane: |r|), K =
// (tune * 1.4826)^2 and min2 = min_scale^2 formed on the host
__host__ __device__ inline double robust_scale2_of(bool plane, double K, double med, double min2) {
    const double medx = plane ? med * med : med;
    const double c2 = K * medx;
    return c2 < min2 ? min2 : c2;
}

}  // namespace kss
