// kss_symm_robust.hip -- robust symmetric ICP (M-estimator weights on the symmetric metric; the definition at kss_icp_symm_robust in
// include/kssicp.h): the weighted correspondence sums of one pass and the keys its median is selected over.
//
// A pass with the AUTOMATIC scale: symm_robust_keys_kernel writes (float)|r| per source, NaN where it is no candidate ->
// launch_trim_select at overlap 0.5 with an infinite bound (kss_trim.hip, unchanged) -> symm_robust_rows_kernel ->
// robust_plane_final_kernel (kss_robust.hip, unchanged, through launch_robust_plane_final).  Every workgroup of the rows kernel and
// the final kernel derive c2 from the selection's last TrimState themselves (robust_pass_c2).  With a FIXED scale: two launches.
// No counter, no flag, no atomic across workgroups: the hand-over is the launch boundary.
//
// The rows kernel has symm_rows_kernel's grid and lane assignment -- p2l_rows_blocks(n) workgroups of 256 lanes, lane t of workgroup
// b takes the sources b * 256 + t + k * 256 * grid in ORIGINAL index order -- so the bits are a function of the source count alone;
// the per-source body is symm_source in its PAIR_ROBUST and PAIR_KEY modes (kss_pair_device.hpp).
#pragma clang fp contract(off)

#include "kss_robust_device.hpp"

namespace kss {

template <int SRC>
__global__ __launch_bounds__(P2L_THREADS) void symm_robust_keys_kernel(const float* __restrict__ src3, const float4* __restrict__ src4,
                                                                       const int32_t* __restrict__ perm, const int32_t* __restrict__ idx,
                                                                       const float* __restrict__ d2_in, const float* __restrict__ sn,
                                                                       const float* __restrict__ tgt, const float* __restrict__ nrm, int64_t n,
                                                                       int64_t nt, double max_d2, const GicpRot Rn, int align,
                                                                       float* __restrict__ keys) {
    for (int64_t i = (int64_t)blockIdx.x * P2L_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * P2L_THREADS) {
        float key = __uint_as_float(0x7fc00000u);
        RobustArg ra;
        ra.key = &key;
        double acc[P2L_NSUMS];   // (never read in this mode)
        symm_source<SRC, PAIR_KEY>(acc, src3, src4, perm, idx, d2_in, sn, tgt, nrm, i, nt, max_d2, Rn, align, ra);
        keys[i] = key;
    }
}

template <int SRC>
__global__ __launch_bounds__(P2L_THREADS) void symm_robust_rows_kernel(const float* __restrict__ src3, const float4* __restrict__ src4,
                                                                       const int32_t* __restrict__ perm, const int32_t* __restrict__ idx,
                                                                       const float* __restrict__ d2_in, const float* __restrict__ sn,
                                                                       const float* __restrict__ tgt, const float* __restrict__ nrm, int64_t n,
                                                                       int64_t nt, double max_d2, const GicpRot Rn, int align,
                                                                       const RobustScale rs, const TrimState* __restrict__ sel,
                                                                       double* __restrict__ rows) {
    __shared__ double sh[P2L_THREADS / 64][P2L_NSUMS];
    double acc[P2L_NSUMS];
#pragma unroll
    for (int c = 0; c < P2L_NSUMS; ++c) acc[c] = 0.0;
    RobustArg ra;
    ra.loss = rs.loss;
    ra.c2 = robust_pass_c2(rs, true, sel);
    for (int64_t i = (int64_t)blockIdx.x * P2L_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * P2L_THREADS)
        symm_source<SRC, PAIR_ROBUST>(acc, src3, src4, perm, idx, d2_in, sn, tgt, nrm, i, nt, max_d2, Rn, align, ra);
    const double r = block_sum<P2L_NSUMS>(acc, sh);
    if (threadIdx.x < P2L_NSUMS) rows[(int64_t)blockIdx.x * P2L_NSUMS + threadIdx.x] = r;
}

static GicpRot symm_rot_of(const float Rn[9]) {
    GicpRot R;
    for (int k = 0; k < 9; ++k) R.r[k] = Rn ? Rn[k] : (k % 4 == 0 ? 1.0f : 0.0f);
    return R;
}

void launch_symm_robust_keys(hipStream_t st, const float* d_src3, const float4* d_src4, const int32_t* d_perm, const int32_t* d_idx,
                             const float* d_d2, const float* d_sn3, const float* d_tgt3, const float* d_nrm3, int64_t n, int64_t nt,
                             double max_d2, const float Rn[9], int align, float* d_keys) {
    const dim3 g(stream_blocks(n)), b(P2L_THREADS);
    const GicpRot R = symm_rot_of(Rn);
#define KSS_SYMM_ROBUST_KEYS(SRC) \
    hipLaunchKernelGGL((symm_robust_keys_kernel<SRC>), g, b, 0, st, d_src3, d_src4, d_perm, d_idx, d_d2, d_sn3, d_tgt3, d_nrm3, n, nt, max_d2, R, align, d_keys)
    if (d_src3) KSS_SYMM_ROBUST_KEYS(SRC_F3);
    else if (d_perm) KSS_SYMM_ROBUST_KEYS(SRC_F4_PERM);
    else KSS_SYMM_ROBUST_KEYS(SRC_F4);
#undef KSS_SYMM_ROBUST_KEYS
}

void launch_symm_robust_sums(hipStream_t st, const float* d_src3, const float4* d_src4, const int32_t* d_perm, const int32_t* d_idx,
                             const float* d_d2, const float* d_sn3, const float* d_tgt3, const float* d_nrm3, int64_t n, int64_t nt,
                             double max_d2, const float Rn[9], int align, const RobustScale& rs, const TrimState* d_sel, double* d_rows,
                             double* d_out, double* d_info) {
    const int nb = p2l_rows_blocks(n);
    const dim3 g(nb), b(P2L_THREADS);
    const GicpRot R = symm_rot_of(Rn);
#define KSS_SYMM_ROBUST_ROWS(SRC) \
    hipLaunchKernelGGL((symm_robust_rows_kernel<SRC>), g, b, 0, st, d_src3, d_src4, d_perm, d_idx, d_d2, d_sn3, d_tgt3, d_nrm3, n, nt, max_d2, R, align, rs, d_sel, d_rows)
    if (d_src3) KSS_SYMM_ROBUST_ROWS(SRC_F3);
    else if (d_perm) KSS_SYMM_ROBUST_ROWS(SRC_F4_PERM);
    else KSS_SYMM_ROBUST_ROWS(SRC_F4);
#undef KSS_SYMM_ROBUST_ROWS
    launch_robust_plane_final(st, d_rows, nb, rs, d_sel, d_out, d_info);
}

}  // namespace kss
