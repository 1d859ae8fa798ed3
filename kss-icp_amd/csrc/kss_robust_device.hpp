// kss_robust_device.hpp -- what the single-pair robust kernels (kss_robust.hip) and the batched ones (kss_pairb.hip) share beyond
// the per-source bodies of kss_pair_device.hpp: the squared scale of a pass.
#pragma once
#include "kss_pair_device.hpp"

namespace kss {

// c2 of a pass, derived by every workgroup that needs it from the selection's last TrimState (sel: not read with a fixed
// scale): one f64 product or two, the same bits everywhere
__device__ __forceinline__ double robust_pass_c2(const RobustScale& rs, bool plane, const TrimState* __restrict__ sel) {
    if (!rs.autoscale) return rs.c2;
    const double med = sel->cut;   // the median key widened (-1: no candidate)
    return med >= 0.0 ? robust_scale2_of(plane, rs.K, med, rs.min2) : 0.0;
}

}  // namespace kss
