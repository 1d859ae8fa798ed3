// kss_robust.hip -- robust ICP (M-estimator weights, iteratively re-weighted least squares): the weighted
// correspondence sums of one pass for both metrics, and the keys the plane metric's median is selected over.
//
// A pass with the AUTOMATIC scale: [plane: robust_keys_kernel writes |r| per source, NaN where it is no candidate] ->
// launch_trim_select at overlap 0.5 (kss_trim.hip, unchanged: over d2 with max_d2 for the point metric, over the keys with an
// infinite bound for the plane metric) -> robust_*_rows_kernel -> robust_*_final_kernel.  Every workgroup of the rows kernel and
// the final kernel derive c2 from the selection's last TrimState themselves (robust_pass_c2: one f64 product or two, the same
// bits everywhere), so no launch exists for it.  With a FIXED scale there is no selection: two launches.
// No counter, no flag, no atomic across workgroups: the hand-over is the launch boundary, nothing has to be zero at rest.
//
// The rows kernels have p2l_rows_kernel's / trim_point_rows_kernel's shape and the final kernels their column order, so the bits
// are a function of the source count alone; the per-source bodies are p2l_source / trim_point_source in their PAIR_ROBUST and
// PAIR_KEY modes (kss_pair_device.hpp).  m and cnt travel as columns of the rows: sums of ones, exact in f64.
#pragma clang fp contract(off)

#include "kss_robust_device.hpp"

namespace kss {

// ---- keys ---------------------------------------------------------------------------------------------------------------
template <bool PLANE, int SRC>
__global__ __launch_bounds__(P2L_THREADS) void robust_keys_kernel(const float* __restrict__ src3, const float4* __restrict__ src4,
                                                                  const int32_t* __restrict__ perm, const int32_t* __restrict__ idx,
                                                                  const float* __restrict__ d2_in, const float* __restrict__ tgt,
                                                                  const float* __restrict__ nrm, int64_t n, int64_t nt, double max_d2,
                                                                  float* __restrict__ keys) {
    for (int64_t i = (int64_t)blockIdx.x * P2L_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * P2L_THREADS) {
        float key = __uint_as_float(0x7fc00000u);
        RobustArg ra;
        ra.key = &key;
        if constexpr (PLANE) {
            double acc[P2L_NSUMS];   // (never read in this mode)
            p2l_source<SRC, true, PAIR_KEY>(acc, src3, src4, perm, idx, d2_in, tgt, nrm, i, nt, max_d2, ra);
        } else {
            double acc[NSUMS];
            trim_point_source<false, PAIR_KEY, true>(acc, nullptr, nullptr, idx, nullptr, tgt, i, nt, max_d2, src3, ra);
        }
        keys[i] = key;
    }
}

void launch_robust_keys(hipStream_t st, bool plane, const float* d_src3, const float4* d_src4, const int32_t* d_perm, const int32_t* d_idx,
                        const float* d_d2, const float* d_tgt3, const float* d_nrm3, int64_t n, int64_t nt, double max_d2, float* d_keys) {
    const dim3 g(stream_blocks(n)), b(P2L_THREADS);
#define KSS_ROBUST_KEYS(PLANE, SRC) \
    hipLaunchKernelGGL((robust_keys_kernel<PLANE, SRC>), g, b, 0, st, d_src3, d_src4, d_perm, d_idx, d_d2, d_tgt3, d_nrm3, n, nt, max_d2, d_keys)
    if (!plane) KSS_ROBUST_KEYS(false, SRC_F3);   // (the loop selects over the NN pass's d2 itself: only kss_robust_sums comes here)
    else if (d_src3) KSS_ROBUST_KEYS(true, SRC_F3);
    else if (d_perm) KSS_ROBUST_KEYS(true, SRC_F4_PERM);
    else KSS_ROBUST_KEYS(true, SRC_F4);
#undef KSS_ROBUST_KEYS
}

// ---- plane metric -------------------------------------------------------------------------------------------------------
template <int SRC>
__global__ __launch_bounds__(P2L_THREADS) void robust_plane_rows_kernel(const float* __restrict__ src3, const float4* __restrict__ src4,
                                                                        const int32_t* __restrict__ perm, const int32_t* __restrict__ idx,
                                                                        const float* __restrict__ d2_in, const float* __restrict__ tgt,
                                                                        const float* __restrict__ nrm, int64_t n, int64_t nt, double max_d2,
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
        p2l_source<SRC, true, PAIR_ROBUST>(acc, src3, src4, perm, idx, d2_in, tgt, nrm, i, nt, max_d2, ra);
    const double r = block_sum<P2L_NSUMS>(acc, sh);
    if (threadIdx.x < P2L_NSUMS) rows[(int64_t)blockIdx.x * P2L_NSUMS + threadIdx.x] = r;
}

// the record as the columns are ([29] = m, [31] = cnt) and the info record {m, c2, [0], cnt}
__global__ __launch_bounds__(P2L_THREADS) void robust_plane_final_kernel(const double* __restrict__ rows, int nrows, const RobustScale rs,
                                                                         const TrimState* __restrict__ sel, double* __restrict__ out,
                                                                         double* __restrict__ info) {
    __shared__ double shg[P2L_GROUPS][P2L_NSUMS];
    const double v = p2l_rows_column_sum(rows, nrows, shg);
    const int t = threadIdx.x;
    if (t < P2L_NSUMS) out[t] = v;
    if (t == 29) info[0] = v;
    if (t == 1) info[1] = robust_pass_c2(rs, true, sel);
    if (t == 0) info[2] = v;
    if (t == 31) info[3] = v;
}

// ---- point metric -------------------------------------------------------------------------------------------------------
template <bool PERM, bool F3>
__global__ __launch_bounds__(TRIM_THREADS) void robust_point_rows_kernel(const float* __restrict__ src3, const float4* __restrict__ src4,
                                                                         const int32_t* __restrict__ perm, const int32_t* __restrict__ idx,
                                                                         const float* __restrict__ d2_in, const float* __restrict__ tgt,
                                                                         int64_t n, int64_t nt, double max_d2, const RobustScale rs,
                                                                         const TrimState* __restrict__ sel, double* __restrict__ rows) {
    __shared__ double sh[TRIM_THREADS / 64][NSUMS];
    double acc[NSUMS];
#pragma unroll
    for (int c = 0; c < NSUMS; ++c) acc[c] = 0.0;
    RobustArg ra;
    ra.loss = rs.loss;
    ra.c2 = robust_pass_c2(rs, false, sel);
    for (int64_t i = (int64_t)blockIdx.x * TRIM_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * TRIM_THREADS)
        trim_point_source<PERM, PAIR_ROBUST, F3>(acc, src4, perm, idx, d2_in, tgt, i, nt, max_d2, src3, ra);
    const double r = block_sum<NSUMS>(acc, sh);
    if (threadIdx.x < NSUMS) rows[(int64_t)blockIdx.x * NSUMS + threadIdx.x] = r;
}

// [17] = m, [18] = 0, [19] = cnt
__global__ __launch_bounds__(TRIM_THREADS) void robust_point_final_kernel(const double* __restrict__ rows, int nrows, const RobustScale rs,
                                                                          const TrimState* __restrict__ sel, double* __restrict__ out,
                                                                          double* __restrict__ info) {
    __shared__ double shg[ROWSUM_GROUPS][NSUMS];
    const double v = rows_column_sum(rows, nrows, shg);
    const int t = threadIdx.x;
    if (t < NSUMS) out[t] = t == 18 ? 0.0 : v;
    if (t == 17) info[0] = v;
    if (t == 1) info[1] = robust_pass_c2(rs, false, sel);
    if (t == 0) info[2] = v;
    if (t == 19) info[3] = v;
}

void launch_robust_plane_final(hipStream_t st, const double* d_rows, int nrows, const RobustScale& rs, const TrimState* d_sel, double* d_out,
                               double* d_info) {
    hipLaunchKernelGGL(robust_plane_final_kernel, dim3(1), dim3(P2L_THREADS), 0, st, d_rows, nrows, rs, d_sel, d_out, d_info);
}

void launch_robust_sums(hipStream_t st, bool plane, const float* d_src3, const float4* d_src4, const int32_t* d_perm, const int32_t* d_idx,
                        const float* d_d2, const float* d_tgt3, const float* d_nrm3, int64_t n, int64_t nt, double max_d2,
                        const RobustScale& rs, const TrimState* d_sel, double* d_rows, double* d_out, double* d_info) {
    const int nb = stream_blocks(n);
    const dim3 g(nb);
    if (plane) {
        const dim3 b(P2L_THREADS);
#define KSS_ROBUST_ROWS(SRC) \
    hipLaunchKernelGGL((robust_plane_rows_kernel<SRC>), g, b, 0, st, d_src3, d_src4, d_perm, d_idx, d_d2, d_tgt3, d_nrm3, n, nt, max_d2, rs, d_sel, d_rows)
        if (d_src3) KSS_ROBUST_ROWS(SRC_F3);
        else if (d_perm) KSS_ROBUST_ROWS(SRC_F4_PERM);
        else KSS_ROBUST_ROWS(SRC_F4);
#undef KSS_ROBUST_ROWS
        launch_robust_plane_final(st, d_rows, nb, rs, d_sel, d_out, d_info);
    } else {
        const dim3 b(TRIM_THREADS);
#define KSS_ROBUST_ROWS(PERM, F3) \
    hipLaunchKernelGGL((robust_point_rows_kernel<PERM, F3>), g, b, 0, st, d_src3, d_src4, d_perm, d_idx, d_d2, d_tgt3, n, nt, max_d2, rs, d_sel, d_rows)
        if (d_src3) KSS_ROBUST_ROWS(false, true);
        else if (d_perm) KSS_ROBUST_ROWS(true, false);
        else KSS_ROBUST_ROWS(false, false);
#undef KSS_ROBUST_ROWS
        hipLaunchKernelGGL(robust_point_final_kernel, dim3(1), b, 0, st, (const double*)d_rows, nb, rs, d_sel, d_out, d_info);
    }
}

}  // namespace kss
