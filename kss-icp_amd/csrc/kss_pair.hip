// kss_pair.hip -- the correspondence sums of the pair metrics for ONE pair: point-to-plane (pcl::registration::
// TransformationEstimationPointToPlaneLLS, PCL 1.8.1), trimmed (2.10), robust (2.12), generalized (2.14), symmetric
// (2.16), robust symmetric (2.19), similarity ICP (2.22) and voxelized generalized ICP against a voxel map (2.30; the map itself is
// kss_vmap.hip's); the definitions are restated in include/kssicp.h.
//   pair_rows_kernel<M, SRC>  the one rows kernel: pair_walk (kss_pair_device.hpp) over the metric functor M with
//                             the sources from SRC.  Grid of stream_blocks(n) workgroups of 256, lane t of workgroup b takes the
//                             sources b * 256 + t + k * 256 * grid in ORIGINAL index order, then block_sum's wave tree and fixed
//                             wave order: one partial row of M::NC f64 columns per workgroup.  The bits depend on the source count
//                             only (not on the NN engine, its tuning or the CU count).  A keys metric (the automatic scale of the
//                             robust forms) writes one selection key per source instead, NaN where it is no candidate.
//   *_final_kernel            one workgroup: the fixed-order column sums of those rows, written to host-mapped memory; the robust
//                             ones add the info record {m, c2, sum of weights, cnt}, deriving c2 like every rows workgroup does
//                             (robust_pass_c2), so no launch exists for it.
// A pass is [keys launch + launch_trim_select at overlap 0.5 (kss_trim.hip)] + rows launch + final launch.  No counter, no flag,
// no atomic across workgroups: the hand-over is the launch boundary, and nothing here has to be zero at rest.
#pragma clang fp contract(off)

#include <cassert>

#include "kss_pair_device.hpp"

namespace kss {

template <class M, int SRC>
__global__ __launch_bounds__(P2L_THREADS) void pair_rows_kernel(const PairArgs a, M m) {
    m.begin();
    pair_walk<M, SRC>(m, a.s, a.tgt, a.nrm, 0, (int64_t)blockIdx.x * P2L_THREADS + threadIdx.x, a.n, (int64_t)gridDim.x * P2L_THREADS, a.nt, a.rows,
                      a.keys);
}

int p2l_rows_blocks(int64_t n) { return stream_blocks(n); }

// the source form once: packed float triples where given (a metric without that form reads the NN pass's float4 output, as
// its body does), else float4 through perm where given
template <class M>
void launch_pair_rows(hipStream_t st, const PairArgs& a, const M& m) {
    const dim3 g(stream_blocks(a.n)), b(P2L_THREADS);
    if constexpr (M::F3) {
        if (a.s.src3) {
            hipLaunchKernelGGL((pair_rows_kernel<M, SRC_F3>), g, b, 0, st, a, m);
            return;
        }
    }
    if (a.s.perm) hipLaunchKernelGGL((pair_rows_kernel<M, SRC_F4_PERM>), g, b, 0, st, a, m);
    else hipLaunchKernelGGL((pair_rows_kernel<M, SRC_F4>), g, b, 0, st, a, m);
}
#define KSS_PAIR_METRIC(M) template void launch_pair_rows<M>(hipStream_t, const PairArgs&, const M&)
KSS_PAIR_METRIC(PlaneMetric<false>);
KSS_PAIR_METRIC(PlaneMetric<true>);
KSS_PAIR_METRIC(PointTrimMetric);
KSS_PAIR_METRIC(SimMetric);
KSS_PAIR_METRIC(PlaneRobustMetric<PAIR_ROBUST>);
KSS_PAIR_METRIC(PlaneRobustMetric<PAIR_KEY>);
KSS_PAIR_METRIC(PointRobustMetric<PAIR_ROBUST>);
KSS_PAIR_METRIC(PointRobustMetric<PAIR_KEY>);
KSS_PAIR_METRIC(GicpMetric);
KSS_PAIR_METRIC(SymmMetric<PAIR_PLAIN>);
KSS_PAIR_METRIC(SymmMetric<PAIR_ROBUST>);
KSS_PAIR_METRIC(SymmMetric<PAIR_KEY>);
#undef KSS_PAIR_METRIC

// voxelized generalized ICP: the same kernel over VgicpMetric, which has the packed-triple form only
template <bool MOVE>
void launch_vgicp_rows(hipStream_t st, const PairArgs& a, const VgicpMetric<MOVE>& m) {
    hipLaunchKernelGGL((pair_rows_kernel<VgicpMetric<MOVE>, SRC_F3>), dim3(stream_blocks(a.n)), dim3(P2L_THREADS), 0, st, a, m);
}
// the map's 7- or 27-voxel neighbourhood: the same walk over VgicpMetric<MOVE, true>, which carries the setting
template <bool MOVE>
void launch_vgicp_nb_rows(hipStream_t st, const PairArgs& a, VgicpMetric<MOVE, true> m, int nb) {
    m.nb = nb;
    hipLaunchKernelGGL((pair_rows_kernel<VgicpMetric<MOVE, true>, SRC_F3>), dim3(stream_blocks(a.n)), dim3(P2L_THREADS), 0, st, a, m);
}
void launch_vgicp_rows(hipStream_t st, const PairArgs& a, const VmapDev& v, const VmapMove* T, const float* d_in, float* d_out, const GicpRot& Rn,
                       double e, int nb) {
    assert(nb == 1 || nb == 7 || nb == 27);   // (kss_vmap_set_neighbourhood admits nothing else)
    if (nb == 7 || nb == 27) {
        if (T) launch_vgicp_nb_rows<true>(st, a, VgicpMetric<true, true>(v, *T, d_in, d_out, Rn, e), nb);
        else launch_vgicp_nb_rows<false>(st, a, VgicpMetric<false, true>(v, VmapMove(), d_in, nullptr, Rn, e), nb);
        return;
    }
    if (T) launch_vgicp_rows<true>(st, a, VgicpMetric<true>(v, *T, d_in, d_out, Rn, e));
    else launch_vgicp_rows<false>(st, a, VgicpMetric<false>(v, VmapMove(), d_in, nullptr, Rn, e));
}

// ---- the final launches -----------------------------------------------------------------------------------------------------
// the rows' column sums in p2l_rows_column_sum's fixed order (kss_pair_device.hpp); slot 31 is written as 0
__global__ __launch_bounds__(P2L_THREADS) void p2l_final_kernel(const double* __restrict__ rows, int nrows, double* __restrict__ out) {
    __shared__ double shg[P2L_GROUPS][P2L_NSUMS];
    const double v = p2l_rows_column_sum(rows, nrows, shg);
    if (threadIdx.x < P2L_NSUMS) out[threadIdx.x] = threadIdx.x == P2L_NSUMS - 1 ? 0.0 : v;
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

void launch_p2l_final(hipStream_t st, const double* d_rows, int nrows, double* d_out) {
    hipLaunchKernelGGL(p2l_final_kernel, dim3(1), dim3(P2L_THREADS), 0, st, d_rows, nrows, d_out);
}

void launch_robust_plane_final(hipStream_t st, const double* d_rows, int nrows, const RobustScale& rs, const TrimState* d_sel, double* d_out,
                               double* d_info) {
    hipLaunchKernelGGL(robust_plane_final_kernel, dim3(1), dim3(P2L_THREADS), 0, st, d_rows, nrows, rs, d_sel, d_out, d_info);
}

void launch_robust_point_final(hipStream_t st, const double* d_rows, int nrows, const RobustScale& rs, const TrimState* d_sel, double* d_out,
                               double* d_info) {
    hipLaunchKernelGGL(robust_point_final_kernel, dim3(1), dim3(TRIM_THREADS), 0, st, d_rows, nrows, rs, d_sel, d_out, d_info);
}

// ---- helpers of the loops ---------------------------------------------------------------------------------------------------
// perm[orig] = k for the cell-ordered sources of a cell-list plan (.w of the packed source = original index)
__global__ __launch_bounds__(256) void p2l_perm_kernel(const float4* __restrict__ src, int64_t n, int32_t* __restrict__ perm) {
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
        const int oi = __float_as_int(src[k].w);
        if (oi >= 0 && oi < n) perm[oi] = (int32_t)k;
    }
}

__global__ __launch_bounds__(256) void f64_to_f32_kernel(const double* __restrict__ in, int64_t n, float* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) out[i] = (float)in[i];
}

void launch_p2l_perm(hipStream_t st, const float4* d_src, int64_t n, int32_t* d_perm) {
    hipLaunchKernelGGL(p2l_perm_kernel, dim3(stream_blocks(n)), dim3(256), 0, st, d_src, n, d_perm);
}

void launch_f64_to_f32(hipStream_t st, const double* d_in, int64_t n, float* d_out) {
    if (n <= 0) return;
    hipLaunchKernelGGL(f64_to_f32_kernel, dim3(stream_blocks(n)), dim3(256), 0, st, d_in, n, d_out);
}

}  // namespace kss
