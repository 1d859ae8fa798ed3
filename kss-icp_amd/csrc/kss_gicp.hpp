// kss_gicp.hpp -- generalized ICP (plane-to-plane; against a voxel map, 2.30): the metric of one correspondence, ONE body for the device
// kernels (kss_pair.hip, kss_pairb.hip through kss_pair_device.hpp) and the C-ABI's host helper (kss_gicp_metric).
// f64 +, -, *, / in the order written down at kss_icp_gicp in include/kssicp.h; the including translation unit is compiled with
// fp contraction off, so nothing here becomes an fma.
#pragma once
#include <hip/hip_runtime.h>

namespace kss {

// M[6] = {M00, M01, M02, M11, M12, M22}, the upper triangle of (2I - e (Q + m m^T))^-1 with e = 1 - epsilon formed by the caller
// and Q[6] = {Q00, Q01, Q02, Q11, Q12, Q22} the target's share of g: nq nq^T for a target point (gicp_metric_of below), the
// voxel's average n n^T for a voxel map (kss_icp_vgicp).  False (M untouched): dropped, det is not finite or not > 0.
__host__ __device__ inline bool gicp_metric_of_g(const double Q[6], const double m[3], double e, double M[6]) {
#pragma clang fp contract(off)
    const double c00 = 2.0 - e * (Q[0] + m[0] * m[0]);
    const double c01 = -(e * (Q[1] + m[0] * m[1]));
    const double c02 = -(e * (Q[2] + m[0] * m[2]));
    const double c11 = 2.0 - e * (Q[3] + m[1] * m[1]);
    const double c12 = -(e * (Q[4] + m[1] * m[2]));
    const double c22 = 2.0 - e * (Q[5] + m[2] * m[2]);
    const double a00 = c11 * c22 - c12 * c12;
    const double a01 = c02 * c12 - c01 * c22;
    const double a02 = c01 * c12 - c02 * c11;
    const double a11 = c00 * c22 - c02 * c02;
    const double a12 = c01 * c02 - c00 * c12;
    const double a22 = c00 * c11 - c01 * c01;
    const double det = (c00 * a00 + c01 * a01) + c02 * a02;
    if (!(det > 0.0) || !(det < __builtin_huge_val())) return false;
    M[0] = a00 / det; M[1] = a01 / det; M[2] = a02 / det;
    M[3] = a11 / det; M[4] = a12 / det; M[5] = a22 / det;
    return true;
}
// ... with the target's normal nq: Q = nq nq^T, every product rounded once before g's addition, as the definition writes it
__host__ __device__ inline bool gicp_metric_of(const double nq[3], const double m[3], double e, double M[6]) {
#pragma clang fp contract(off)
    const double Q[6] = {nq[0] * nq[0], nq[0] * nq[1], nq[0] * nq[2], nq[1] * nq[1], nq[1] * nq[2], nq[2] * nq[2]};
    return gicp_metric_of_g(Q, m, e, M);
}

// the rotation applied to the source normals, by value into the kernel (row-major, float as in the accumulated Matrix4f)
struct GicpRot {
    float r[9];
};
// ... from the row-major 3 x 3 an entry point was given (null: identity)
inline GicpRot gicp_rot_of(const float Rn[9]) {
    GicpRot R;
    for (int k = 0; k < 9; ++k) R.r[k] = Rn ? Rn[k] : (k % 4 == 0 ? 1.0f : 0.0f);
    return R;
}

}  // namespace kss
