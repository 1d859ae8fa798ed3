// kss_pairb.hip -- the pair metrics for MANY pairs per call: per lockstep pass a
// handful of launches for the whole batch behind the NN pass, whatever the pair count.
//   pairb_rows_kernel<M, PERM>   the one rows kernel: grid = the sum over the pairs of stream_blocks(ns_p) workgroups, mapped through
//                         a row -> pair table.  Workgroup b of pair p builds the metric functor M from the per-pair tables at p
//                         (the pair's TrimState, RobustScale, PairPass) and runs pair_walk (kss_pair_device.hpp) over the pair's
//                         sources b * 256 + t + k * 256 * stream_blocks(ns_p) in ORIGINAL index order -- pair_rows_kernel's
//                         assignment for a pair of that size (kss_pair.hip).  So a pair's record is added in the order its
//                         source count alone decides: the single-pair call's bits.  A keys metric writes |r| per source (NaN: no
//                         candidate) into a batch-wide key array by global original source index, for the automatic pairs alone.
//   pairb_select_kernel   trimmed only.  One workgroup of 256 per active pair runs the radix select of kss_trim.hip over the
//                         pair's d2 segment: three digits (11 + 10 + 10 bits) in a loop, a 2048-bin LDS histogram filled with
//                         integer LDS atomics, every digit resolved by trim_resolve_counts (kss_pair_device.hpp) -- the logic of
//                         the four-launch form on LDS instead of histogram rows.  The segment is re-read per digit (40 KB at
//                         10k points: L2).  Writes the pair's TrimState (cut, m, k, kept) to a device table and {m, k, tau,
//                         kept} to a host-mapped one.  No atomics across workgroups, no counters, nothing zero at rest.  Any
//                         segment length is correct; one workgroup is what a pair gets, so a segment of millions of points
//                         is one slow workgroup (3M keys: about a millisecond) -- the batch is for pairs of tens of thousands.
//   pairb_robust_select_kernel   automatic pairs: that select at overlap 0.5 over the pair's keys (point metric: the NN pass's
//                         d2), the pair's TrimState alone -- its {m, k, tau, kept} is no part of the robust info record.
//   pairb_final_kernel    one workgroup per pair: the fixed-order column sums of the pair's rows, written to host-mapped memory.
//   pairb_robust_final_kernel    the same with the weighted record's columns and {m, c2, sum of weights, cnt}.
//   vgicpb_rows_kernel<MOVE>, vgicpb_final_kernel    many scans against one voxel map: the same walk over
//                         VgicpMetric and the same column sums, on a per-scan pass table of their own (no NN pass, no PairState).
// Workgroups of pairs that are no longer active leave at once: they read the per-pair state table of the NN pass.  Fixed-scale
// pairs skip the keys and the select; a batch without an automatic pair does not launch them.
// The generalized and symmetric forms read the rotation applied to the source normals and e / align_normals once per workgroup
// from the pair's PairPass, a table the host rewrites before every pass; the source normals are packed like the sources and
// read by global original index.
#pragma clang fp contract(off)

#include <cassert>

#include "kss_pair_device.hpp"

namespace kss {

__device__ __forceinline__ bool pairb_active(const PairState* __restrict__ state, int p) { return !state || state[p].active != 0; }

// one digit of the select over the segment d2[0..n): counts into hist, resolves into *out (prev: the state before it)
template <int DIGIT>
__device__ __forceinline__ void pairb_digit(const float* __restrict__ d2, int64_t n, double max_d2, double overlap, unsigned* hist,
                                            const TrimState* prev, TrimState* out, unsigned* wave_tot) {
    for (int b = threadIdx.x; b < TRIM_BINS; b += TRIM_HIST_THREADS) hist[b] = 0u;
    unsigned prefix = 0u;
    bool any = true;
    if constexpr (DIGIT > 0) {
        prefix = prev->prefix;
        any = prev->rank > 0;   // no candidate at all: nothing to count
    }
    __syncthreads();
    if (any) {
        // eight loads in flight per lane; a slot past the end holds a NaN, which is no candidate
        constexpr int64_t stride = TRIM_HIST_THREADS;
        for (int64_t i0 = threadIdx.x; i0 < n; i0 += 8 * stride) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int64_t i = i0 + u * stride;
                v[u] = i < n ? d2[i] : __uint_as_float(0x7fc00000u);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                unsigned key;
                bool live = trim_key(v[u], max_d2, key);
                if constexpr (DIGIT > 0) live = live && (key >> trim_shift(DIGIT - 1)) == prefix;
                if (live) atomicAdd(&hist[(key >> trim_shift(DIGIT)) & ((1u << trim_bits(DIGIT)) - 1u)], 1u);
            }
        }
    }
    __syncthreads();
    unsigned c[TRIM_LANE_BINS];
#pragma unroll
    for (int q = 0; q < TRIM_LANE_BINS; ++q) c[q] = hist[TRIM_LANE_BINS * threadIdx.x + q];
    trim_resolve_counts<DIGIT>(c, overlap, prev, out, wave_tot);
}

__global__ __launch_bounds__(TRIM_HIST_THREADS) void pairb_select_kernel(const float* __restrict__ d2_all, const PairbDesc* __restrict__ desc,
                                                                         const PairState* __restrict__ state, double max_d2,
                                                                         TrimState* __restrict__ st_out, double* __restrict__ info_out) {
    __shared__ unsigned hist[TRIM_BINS];
    __shared__ TrimState cur[2];
    __shared__ unsigned wave_tot[TRIM_HIST_THREADS / 64];
    const int p = blockIdx.x;
    if (!pairb_active(state, p)) return;
    const PairbDesc d = desc[p];
    const float* d2 = d2_all + d.src_base;
    pairb_digit<0>(d2, d.ns, max_d2, d.overlap, hist, &cur[1], &cur[0], wave_tot);
    pairb_digit<1>(d2, d.ns, max_d2, d.overlap, hist, &cur[0], &cur[1], wave_tot);
    pairb_digit<2>(d2, d.ns, max_d2, d.overlap, hist, &cur[1], &cur[0], wave_tot);
    if (threadIdx.x == 0) {
        const TrimState s = cur[0];
        st_out[p] = s;
        double* info = info_out + (int64_t)p * KSS_TRIM_NINFO;
        info[0] = (double)s.m; info[1] = (double)s.k;
        info[2] = s.rank > 0 ? s.cut : 0.0;
        info[3] = (double)s.kept;
    }
}

__device__ __forceinline__ bool pairb_robust_selects(const PairState* __restrict__ state, const RobustScale* __restrict__ rs, int p) {
    return pairb_active(state, p) && rs[p].autoscale != 0;
}

template <class M, bool PERM>
__global__ __launch_bounds__(P2L_THREADS) void pairb_rows_kernel(const PairbArgs a) {
    const int p = a.row_pair[blockIdx.x];
    if (M::KEYS ? !pairb_robust_selects(a.state, a.rs, p) : !pairb_active(a.state, p)) return;
    const PairbDesc d = a.desc[p];
    M m(a, p);
    m.begin();
    pair_walk<M, PERM ? SRC_F4_PERM : SRC_F4>(m, a.s, a.tgt + 3 * d.tgt_off, a.nrm + 3 * d.tgt_off, d.src_base,
                                              (int64_t)((int)blockIdx.x - d.row_base) * P2L_THREADS + threadIdx.x, d.ns,
                                              (int64_t)d.nrows * P2L_THREADS, d.nt, a.rows, a.keys);
}

// out: KSS_P2L_NSUMS doubles per pair for either metric (the point record fills the first KSS_NSUMS; slots 17..19 are 0; SIM, the
// similarity step's record: 17 is kept, 18 and 19 are 0)
template <bool PLANE, bool SIM = false>
__global__ __launch_bounds__(P2L_THREADS) void pairb_final_kernel(const double* __restrict__ rows, const PairbDesc* __restrict__ desc,
                                                                  const PairState* __restrict__ state, double* __restrict__ out) {
    constexpr int NC = PLANE ? P2L_NSUMS : NSUMS;
    constexpr int NG = PLANE ? P2L_GROUPS : ROWSUM_GROUPS;
    __shared__ double shg[NG][NC];
    const int p = blockIdx.x;
    if (!pairb_active(state, p)) return;
    const PairbDesc d = desc[p];
    const double* r = rows + (int64_t)d.row_base * NC;
    double* o = out + (int64_t)p * P2L_NSUMS;
    if constexpr (PLANE) {
        const double v = p2l_rows_column_sum(r, d.nrows, shg);
        if (threadIdx.x < P2L_NSUMS) o[threadIdx.x] = threadIdx.x == P2L_NSUMS - 1 ? 0.0 : v;
    } else {
        const double v = rows_column_sum(r, d.nrows, shg);
        if (threadIdx.x < NSUMS) o[threadIdx.x] = threadIdx.x >= (SIM ? 18 : 17) ? 0.0 : v;
    }
}

// the median key of every automatic pair: pairb_select_kernel at overlap 0.5, the TrimState alone
__global__ __launch_bounds__(TRIM_HIST_THREADS) void pairb_robust_select_kernel(const float* __restrict__ keys_all, const PairbDesc* __restrict__ desc,
                                                                                const PairState* __restrict__ state,
                                                                                const RobustScale* __restrict__ rs, double bound,
                                                                                TrimState* __restrict__ st_out) {
    __shared__ unsigned hist[TRIM_BINS];
    __shared__ TrimState cur[2];
    __shared__ unsigned wave_tot[TRIM_HIST_THREADS / 64];
    const int p = blockIdx.x;
    if (!pairb_robust_selects(state, rs, p)) return;
    const PairbDesc d = desc[p];
    const float* keys = keys_all + d.src_base;
    pairb_digit<0>(keys, d.ns, bound, 0.5, hist, &cur[1], &cur[0], wave_tot);
    pairb_digit<1>(keys, d.ns, bound, 0.5, hist, &cur[0], &cur[1], wave_tot);
    pairb_digit<2>(keys, d.ns, bound, 0.5, hist, &cur[1], &cur[0], wave_tot);
    if (threadIdx.x == 0) st_out[p] = cur[0];
}

// out: KSS_P2L_NSUMS doubles per pair for either metric, the record as the columns are (plane [29] = m, [31] = cnt; point [17] = m,
// [18] = 0, [19] = cnt); info: {m, c2, [0], cnt} per pair
template <bool PLANE>
__global__ __launch_bounds__(P2L_THREADS) void pairb_robust_final_kernel(const double* __restrict__ rows, const PairbDesc* __restrict__ desc,
                                                                         const PairState* __restrict__ state, const RobustScale* __restrict__ rs,
                                                                         const TrimState* __restrict__ ts, double* __restrict__ out,
                                                                         double* __restrict__ info_out) {
    constexpr int NC = PLANE ? P2L_NSUMS : NSUMS;
    constexpr int NG = PLANE ? P2L_GROUPS : ROWSUM_GROUPS;
    __shared__ double shg[NG][NC];
    const int p = blockIdx.x;
    if (!pairb_active(state, p)) return;
    const PairbDesc d = desc[p];
    const double* r = rows + (int64_t)d.row_base * NC;
    double* o = out + (int64_t)p * P2L_NSUMS;
    double* info = info_out + (int64_t)p * KSS_ROBUST_NINFO;
    const int t = threadIdx.x;
    if constexpr (PLANE) {
        const double v = p2l_rows_column_sum(r, d.nrows, shg);
        if (t < P2L_NSUMS) o[t] = v;
        if (t == 29) info[0] = v;
        if (t == 0) info[2] = v;
        if (t == 31) info[3] = v;
    } else {
        const double v = rows_column_sum(r, d.nrows, shg);
        if (t < NSUMS) o[t] = t == 18 ? 0.0 : v;
        if (t == 17) info[0] = v;
        if (t == 0) info[2] = v;
        if (t == 19) info[3] = v;
    }
    if (t == 1) info[1] = robust_pass_c2(rs[p], PLANE, ts + p);
}

void launch_pairb_select(hipStream_t st, const float* d_d2, const PairbDesc* d_desc, int npairs, const PairState* d_state, double max_d2,
                         TrimState* d_ts, double* d_info) {
    hipLaunchKernelGGL(pairb_select_kernel, dim3(npairs), dim3(TRIM_HIST_THREADS), 0, st, d_d2, d_desc, d_state, max_d2, d_ts, d_info);
}

template <class M>
void launch_pairb_rows(hipStream_t st, int total_rows, const PairbArgs& a) {
    if (a.s.perm) hipLaunchKernelGGL((pairb_rows_kernel<M, true>), dim3(total_rows), dim3(P2L_THREADS), 0, st, a);
    else hipLaunchKernelGGL((pairb_rows_kernel<M, false>), dim3(total_rows), dim3(P2L_THREADS), 0, st, a);
}
#define KSS_PAIRB_METRIC(M) template void launch_pairb_rows<M>(hipStream_t, int, const PairbArgs&)
KSS_PAIRB_METRIC(PlaneMetric<false>);
KSS_PAIRB_METRIC(PlaneMetric<true>);
KSS_PAIRB_METRIC(PointTrimMetric);   // (the untrimmed point metric is kss_icp_batch's)
KSS_PAIRB_METRIC(SimMetric);
KSS_PAIRB_METRIC(PlaneRobustMetric<PAIR_ROBUST>);
KSS_PAIRB_METRIC(PlaneRobustMetric<PAIR_KEY>);
KSS_PAIRB_METRIC(PointRobustMetric<PAIR_ROBUST>);   // (its keys are the NN pass's d2)
KSS_PAIRB_METRIC(GicpMetric);
KSS_PAIRB_METRIC(SymmMetric<PAIR_PLAIN>);
KSS_PAIRB_METRIC(SymmMetric<PAIR_ROBUST>);
KSS_PAIRB_METRIC(SymmMetric<PAIR_KEY>);
#undef KSS_PAIRB_METRIC

void launch_pairb_robust_select(hipStream_t st, int npairs, const PairbArgs& a, const float* d_keys, double bound) {
    hipLaunchKernelGGL(pairb_robust_select_kernel, dim3(npairs), dim3(TRIM_HIST_THREADS), 0, st, d_keys, a.desc, a.state, a.rs, bound, a.ts);
}

void launch_pairb_final(hipStream_t st, bool plane, int npairs, const PairbArgs& a, double* d_out, bool sim) {
    const dim3 g(npairs), b(P2L_THREADS);
    if (sim) hipLaunchKernelGGL((pairb_final_kernel<false, true>), g, b, 0, st, (const double*)a.rows, a.desc, a.state, d_out);
    else if (plane) hipLaunchKernelGGL(pairb_final_kernel<true>, g, b, 0, st, (const double*)a.rows, a.desc, a.state, d_out);
    else hipLaunchKernelGGL(pairb_final_kernel<false>, g, b, 0, st, (const double*)a.rows, a.desc, a.state, d_out);
}

// ---- voxelized generalized ICP, many scans against one map (kss_icp_vgicp_batch) ----
// The batch form of pair_rows_kernel<VgicpMetric<MOVE>, SRC_F3>: workgroup b of scan p runs pair_walk over the scan's own ns
// sources b * 256 + t + k * 256 * stream_blocks(ns), offset by the scan's base into the packed arrays -- the single-scan kernel's
// assignment -- on vgicp_source<MOVE> and block_sum, so a scan's rows are the single call's.  The scan's pass entry (its step, the
// rotation for its normals, e, the active flag) is one uniform load per workgroup; workgroups of scans that have ended leave at once.
// NEIGH: the map's 7- or 27-voxel neighbourhood (a.nb) through vgicp_source<MOVE, true>.
template <bool MOVE, bool NEIGH = false>
__global__ __launch_bounds__(P2L_THREADS) void vgicpb_rows_kernel(const VgicpbArgs a) {
    const int p = a.row_pair[blockIdx.x];
    const VgicpbPass pp = a.pass[p];
    if (pp.active == 0) return;
    const PairbDesc d = a.desc[p];
    const VgicpMetric<MOVE, NEIGH> m(a, pp);
    const PairSrc s = {nullptr, nullptr, nullptr, nullptr, nullptr, a.sn, a.max_d2};
    pair_walk<VgicpMetric<MOVE, NEIGH>, SRC_F3>(m, s, nullptr, nullptr, d.src_base, (int64_t)((int)blockIdx.x - d.row_base) * P2L_THREADS + threadIdx.x,
                                                d.ns, (int64_t)d.nrows * P2L_THREADS, 0, a.rows, nullptr);
}

// pairb_final_kernel<true> on the pass table's active flag
__global__ __launch_bounds__(P2L_THREADS) void vgicpb_final_kernel(const double* __restrict__ rows, const PairbDesc* __restrict__ desc,
                                                                   const VgicpbPass* __restrict__ pass, double* __restrict__ out) {
    __shared__ double shg[P2L_GROUPS][P2L_NSUMS];
    const int p = blockIdx.x;
    if (pass[p].active == 0) return;
    const PairbDesc d = desc[p];
    const double v = p2l_rows_column_sum(rows + (int64_t)d.row_base * P2L_NSUMS, d.nrows, shg);
    if (threadIdx.x < P2L_NSUMS) out[(int64_t)p * P2L_NSUMS + threadIdx.x] = threadIdx.x == P2L_NSUMS - 1 ? 0.0 : v;
}

void launch_vgicpb_rows(hipStream_t st, int total_rows, bool move, const VgicpbArgs& a) {
    assert(a.nb == 1 || a.nb == 7 || a.nb == 27);   // (kss_vmap_set_neighbourhood admits nothing else)
    if (a.nb == 7 || a.nb == 27) {
        if (move) hipLaunchKernelGGL((vgicpb_rows_kernel<true, true>), dim3(total_rows), dim3(P2L_THREADS), 0, st, a);
        else hipLaunchKernelGGL((vgicpb_rows_kernel<false, true>), dim3(total_rows), dim3(P2L_THREADS), 0, st, a);
        return;
    }
    if (move) hipLaunchKernelGGL(vgicpb_rows_kernel<true>, dim3(total_rows), dim3(P2L_THREADS), 0, st, a);
    else hipLaunchKernelGGL(vgicpb_rows_kernel<false>, dim3(total_rows), dim3(P2L_THREADS), 0, st, a);
}

void launch_vgicpb_final(hipStream_t st, int nscans, const VgicpbArgs& a, double* d_out) {
    hipLaunchKernelGGL(vgicpb_final_kernel, dim3(nscans), dim3(P2L_THREADS), 0, st, (const double*)a.rows, a.desc, a.pass, d_out);
}

void launch_pairb_robust_final(hipStream_t st, bool plane, int npairs, const PairbArgs& a, double* d_out, double* d_info) {
    const dim3 g(npairs), b(P2L_THREADS);
    if (plane)
        hipLaunchKernelGGL(pairb_robust_final_kernel<true>, g, b, 0, st, (const double*)a.rows, a.desc, a.state, a.rs, (const TrimState*)a.ts, d_out, d_info);
    else
        hipLaunchKernelGGL(pairb_robust_final_kernel<false>, g, b, 0, st, (const double*)a.rows, a.desc, a.state, a.rs, (const TrimState*)a.ts, d_out, d_info);
}

}  // namespace kss
