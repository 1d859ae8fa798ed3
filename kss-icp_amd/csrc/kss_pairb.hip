// kss_pairb.hip -- point-to-plane and trimmed ICP for MANY pairs per call: per lockstep pass THREE launches for
// the whole batch behind the NN pass, whatever the pair count.
//   pairb_select_kernel   trimmed only.  One workgroup of 256 per active pair runs the radix select of kss_trim.hip over the
//                         pair's d2 segment: three digits (11 + 10 + 10 bits) in a loop, a 2048-bin LDS histogram filled with
//                         integer LDS atomics, every digit resolved by trim_resolve_counts (kss_pair_device.hpp) -- the logic of
//                         the four-launch form on LDS instead of histogram rows.  The segment is re-read per digit (40 KB at
//                         10k points: L2).  Writes the pair's TrimState (cut, m, k, kept) to a device table and {m, k, tau,
//                         kept} to a host-mapped one.  No atomics across workgroups, no counters, nothing zero at rest.  Any
//                         segment length is correct; one workgroup is what a pair gets, so a segment of millions of points
//                         is one slow workgroup (3M keys: about a millisecond) -- the batch is for pairs of tens of thousands.
//   pairb_rows_kernel     grid = the sum over the pairs of stream_blocks(ns_p) workgroups, mapped through a row -> pair table.
//                         Workgroup b of pair p takes the pair's sources b * 256 + t + k * 256 * stream_blocks(ns_p) in
//                         ORIGINAL index order -- p2l_rows_kernel's / trim_point_rows_kernel's assignment for a pair of that
//                         size --, runs the shared per-source body and block_sum.  The cut is the pair's TrimState.
//   pairb_final_kernel    one workgroup per pair: the fixed-order column sums of the pair's rows, written to host-mapped memory.
// So a pair's record is added in the order its source count alone decides: the single-pair call's bits.
// Workgroups of pairs that are no longer active leave at once: they read the per-pair state table of the NN pass.
//
// Robust ICP for many pairs has the same shape, with the pair's RobustScale from a per-pair table:
//   pairb_robust_keys_kernel     plane metric, automatic pairs: pairb_rows_kernel's grid writes |r| per source (NaN: no candidate)
//                                into a batch-wide key array by global original source index.
//   pairb_robust_select_kernel   automatic pairs: the select above at overlap 0.5 over the pair's keys (point: the NN pass's d2),
//                                the pair's TrimState alone -- its {m, k, tau, kept} is no part of the robust info record.
//   pairb_robust_rows_kernel     pairb_rows_kernel with the PAIR_ROBUST bodies; every workgroup derives the pass's c2 itself.
//   pairb_robust_final_kernel    the column sums, the record and {m, c2, sum of weights, cnt} to host-mapped memory.
// Fixed-scale pairs skip the first two; a batch without an automatic pair does not launch them.
//
// Generalized ICP for many pairs: two launches per pass behind the NN pass.
//   pairb_gicp_rows_kernel       pairb_rows_kernel's grid on gicp_source (kss_pair_device.hpp); the rotation applied to the source
//                                normals and e = 1 - epsilon are the PAIR's, read once per workgroup from a per-pair table of
//                                GicpPass that the host rewrites before every pass.  The source normals are packed like the
//                                sources and read by global original index.
//   pairb_final_kernel<true>     unchanged.
//
// Symmetric ICP for many pairs: the same two launches, the table's transport shared with the generalized form.
//   pairb_symm_rows_kernel       pairb_rows_kernel's grid on symm_source (kss_pair_device.hpp); the rotation applied to the source
//                                normals and align_normals are the PAIR's, read once per workgroup from a per-pair table of
//                                SymmPass whose rotations the host rewrites before every pass.  The source normals are packed
//                                like the sources and read by global original index.
//   pairb_final_kernel<true>     unchanged.
//
// Robust symmetric ICP for many pairs: the robust shape on the symmetric body, both per-pair tables at once.
//   pairb_symm_robust_keys_kernel  automatic pairs: pairb_robust_keys_kernel's grid and exit test on symm_source's PAIR_KEY mode,
//                                  |r| per source (NaN: no candidate) into the batch-wide key array by global original source index.
//   pairb_robust_select_kernel     unchanged, over those keys with an infinite bound.
//   pairb_symm_robust_rows_kernel  pairb_symm_rows_kernel's grid on symm_source's PAIR_ROBUST mode; the rotation and align from the
//                                  pair's SymmPass, the loss and the pass's c2 from its RobustScale and TrimState.
//   pairb_robust_final_kernel<true>  unchanged.
#pragma clang fp contract(off)

#include "kss_robust_device.hpp"

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

template <bool PLANE, bool TRIM, bool PERM>
__global__ __launch_bounds__(P2L_THREADS) void pairb_rows_kernel(const float4* __restrict__ src4, const int32_t* __restrict__ perm,
                                                                 const int32_t* __restrict__ idx, const float* __restrict__ d2_in,
                                                                 const float* __restrict__ tgt_all, const float* __restrict__ nrm_all,
                                                                 const PairbDesc* __restrict__ desc, const int32_t* __restrict__ row_pair,
                                                                 const PairState* __restrict__ state, const TrimState* __restrict__ ts,
                                                                 double max_d2, double* __restrict__ rows) {
    constexpr int NC = PLANE ? P2L_NSUMS : NSUMS;
    __shared__ double sh[P2L_THREADS / 64][NC];
    const int p = row_pair[blockIdx.x];
    if (!pairb_active(state, p)) return;
    const PairbDesc d = desc[p];
    double acc[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = 0.0;
    const double lim = TRIM ? ts[p].cut : max_d2;   // tau of this pass (-1: no candidate), written by the selection
    const float* tgt = tgt_all + 3 * d.tgt_off;
    const int64_t step = (int64_t)d.nrows * P2L_THREADS;
    for (int64_t i = (int64_t)((int)blockIdx.x - d.row_base) * P2L_THREADS + threadIdx.x; i < d.ns; i += step) {
        if constexpr (PLANE)
            p2l_source<PERM ? SRC_F4_PERM : SRC_F4, TRIM>(acc, nullptr, src4, perm, idx, d2_in, tgt, nrm_all + 3 * d.tgt_off, d.src_base + i, d.nt, lim);
        else
            trim_point_source<PERM>(acc, src4, perm, idx, d2_in, tgt, d.src_base + i, d.nt, lim);
    }
    const double r = block_sum<NC>(acc, sh);
    if (threadIdx.x < NC) rows[(int64_t)blockIdx.x * NC + threadIdx.x] = r;
}

// out: KSS_P2L_NSUMS doubles per pair for either metric (the point record fills the first KSS_NSUMS; slots 17..19 are 0)
template <bool PLANE>
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
        if (threadIdx.x < NSUMS) o[threadIdx.x] = threadIdx.x >= 17 ? 0.0 : v;
    }
}

// ---- generalized ICP (kss_gicp.hip's kernel, per pair) ----------------------------------------------------------------------
// pass[p] is the same for every lane of the workgroup (p comes from blockIdx.x alone): one uniform load, nothing per source
template <bool PERM>
__global__ __launch_bounds__(P2L_THREADS) void pairb_gicp_rows_kernel(const float4* __restrict__ src4, const int32_t* __restrict__ perm,
                                                                      const int32_t* __restrict__ idx, const float* __restrict__ d2_in,
                                                                      const float* __restrict__ sn_all, const float* __restrict__ tgt_all,
                                                                      const float* __restrict__ nrm_all, const PairbDesc* __restrict__ desc,
                                                                      const int32_t* __restrict__ row_pair, const PairState* __restrict__ state,
                                                                      const GicpPass* __restrict__ pass, double max_d2,
                                                                      double* __restrict__ rows) {
    __shared__ double sh[P2L_THREADS / 64][P2L_NSUMS];
    const int p = row_pair[blockIdx.x];
    if (!pairb_active(state, p)) return;
    const PairbDesc d = desc[p];
    const GicpPass gp = pass[p];
    GicpRot Rn;
#pragma unroll
    for (int k = 0; k < 9; ++k) Rn.r[k] = gp.r[k];
    double acc[P2L_NSUMS];
#pragma unroll
    for (int c = 0; c < P2L_NSUMS; ++c) acc[c] = 0.0;
    const float* tgt = tgt_all + 3 * d.tgt_off;
    const float* nrm = nrm_all + 3 * d.tgt_off;
    const int64_t step = (int64_t)d.nrows * P2L_THREADS;
    for (int64_t i = (int64_t)((int)blockIdx.x - d.row_base) * P2L_THREADS + threadIdx.x; i < d.ns; i += step)
        gicp_source<PERM ? SRC_F4_PERM : SRC_F4>(acc, nullptr, src4, perm, idx, d2_in, sn_all, tgt, nrm, d.src_base + i, d.nt, max_d2, Rn, gp.e);
    const double r = block_sum<P2L_NSUMS>(acc, sh);
    if (threadIdx.x < P2L_NSUMS) rows[(int64_t)blockIdx.x * P2L_NSUMS + threadIdx.x] = r;
}

// ---- symmetric ICP (kss_symm.hip's kernel, per pair) ------------------------------------------------------------------------
// pass[p] as above: one uniform load per workgroup
template <bool PERM>
__global__ __launch_bounds__(P2L_THREADS) void pairb_symm_rows_kernel(const float4* __restrict__ src4, const int32_t* __restrict__ perm,
                                                                      const int32_t* __restrict__ idx, const float* __restrict__ d2_in,
                                                                      const float* __restrict__ sn_all, const float* __restrict__ tgt_all,
                                                                      const float* __restrict__ nrm_all, const PairbDesc* __restrict__ desc,
                                                                      const int32_t* __restrict__ row_pair, const PairState* __restrict__ state,
                                                                      const SymmPass* __restrict__ pass, double max_d2,
                                                                      double* __restrict__ rows) {
    __shared__ double sh[P2L_THREADS / 64][P2L_NSUMS];
    const int p = row_pair[blockIdx.x];
    if (!pairb_active(state, p)) return;
    const PairbDesc d = desc[p];
    const SymmPass sp = pass[p];
    GicpRot Rn;
#pragma unroll
    for (int k = 0; k < 9; ++k) Rn.r[k] = sp.r[k];
    double acc[P2L_NSUMS];
#pragma unroll
    for (int c = 0; c < P2L_NSUMS; ++c) acc[c] = 0.0;
    const float* tgt = tgt_all + 3 * d.tgt_off;
    const float* nrm = nrm_all + 3 * d.tgt_off;
    const int64_t step = (int64_t)d.nrows * P2L_THREADS;
    for (int64_t i = (int64_t)((int)blockIdx.x - d.row_base) * P2L_THREADS + threadIdx.x; i < d.ns; i += step)
        symm_source<PERM ? SRC_F4_PERM : SRC_F4>(acc, nullptr, src4, perm, idx, d2_in, sn_all, tgt, nrm, d.src_base + i, d.nt, max_d2, Rn, sp.align);
    const double r = block_sum<P2L_NSUMS>(acc, sh);
    if (threadIdx.x < P2L_NSUMS) rows[(int64_t)blockIdx.x * P2L_NSUMS + threadIdx.x] = r;
}

// ---- robust ICP (kss_robust.hip's kernels, per pair) ------------------------------------------------------------------------
__device__ __forceinline__ bool pairb_robust_selects(const PairState* __restrict__ state, const RobustScale* __restrict__ rs, int p) {
    return pairb_active(state, p) && rs[p].autoscale != 0;
}

template <bool PERM>
__global__ __launch_bounds__(P2L_THREADS) void pairb_robust_keys_kernel(const float4* __restrict__ src4, const int32_t* __restrict__ perm,
                                                                        const int32_t* __restrict__ idx, const float* __restrict__ d2_in,
                                                                        const float* __restrict__ tgt_all, const float* __restrict__ nrm_all,
                                                                        const PairbDesc* __restrict__ desc, const int32_t* __restrict__ row_pair,
                                                                        const PairState* __restrict__ state, const RobustScale* __restrict__ rs,
                                                                        double max_d2, float* __restrict__ keys) {
    const int p = row_pair[blockIdx.x];
    if (!pairb_robust_selects(state, rs, p)) return;
    const PairbDesc d = desc[p];
    const float* tgt = tgt_all + 3 * d.tgt_off;
    const float* nrm = nrm_all + 3 * d.tgt_off;
    const int64_t step = (int64_t)d.nrows * P2L_THREADS;
    for (int64_t i = (int64_t)((int)blockIdx.x - d.row_base) * P2L_THREADS + threadIdx.x; i < d.ns; i += step) {
        float key = __uint_as_float(0x7fc00000u);
        RobustArg ra;
        ra.key = &key;
        double acc[P2L_NSUMS];   // (never read in this mode)
        p2l_source<PERM ? SRC_F4_PERM : SRC_F4, true, PAIR_KEY>(acc, nullptr, src4, perm, idx, d2_in, tgt, nrm, d.src_base + i, d.nt, max_d2, ra);
        keys[d.src_base + i] = key;
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

template <bool PLANE, bool PERM>
__global__ __launch_bounds__(P2L_THREADS) void pairb_robust_rows_kernel(const float4* __restrict__ src4, const int32_t* __restrict__ perm,
                                                                        const int32_t* __restrict__ idx, const float* __restrict__ d2_in,
                                                                        const float* __restrict__ tgt_all, const float* __restrict__ nrm_all,
                                                                        const PairbDesc* __restrict__ desc, const int32_t* __restrict__ row_pair,
                                                                        const PairState* __restrict__ state, const RobustScale* __restrict__ rs,
                                                                        const TrimState* __restrict__ ts, double max_d2, double* __restrict__ rows) {
    constexpr int NC = PLANE ? P2L_NSUMS : NSUMS;
    __shared__ double sh[P2L_THREADS / 64][NC];
    const int p = row_pair[blockIdx.x];
    if (!pairb_active(state, p)) return;
    const PairbDesc d = desc[p];
    double acc[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = 0.0;
    const RobustScale s = rs[p];
    RobustArg ra;
    ra.loss = s.loss;
    ra.c2 = robust_pass_c2(s, PLANE, ts + p);
    const float* tgt = tgt_all + 3 * d.tgt_off;
    const int64_t step = (int64_t)d.nrows * P2L_THREADS;
    for (int64_t i = (int64_t)((int)blockIdx.x - d.row_base) * P2L_THREADS + threadIdx.x; i < d.ns; i += step) {
        if constexpr (PLANE)
            p2l_source<PERM ? SRC_F4_PERM : SRC_F4, true, PAIR_ROBUST>(acc, nullptr, src4, perm, idx, d2_in, tgt, nrm_all + 3 * d.tgt_off,
                                                                       d.src_base + i, d.nt, max_d2, ra);
        else
            trim_point_source<PERM, PAIR_ROBUST, false>(acc, src4, perm, idx, d2_in, tgt, d.src_base + i, d.nt, max_d2, nullptr, ra);
    }
    const double r = block_sum<NC>(acc, sh);
    if (threadIdx.x < NC) rows[(int64_t)blockIdx.x * NC + threadIdx.x] = r;
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

// ---- robust symmetric ICP (kss_symm_robust.hip's kernels, per pair) ---------------------------------------------------------
// pass[p] as for pairb_symm_rows_kernel: one uniform load per workgroup
template <bool PERM>
__global__ __launch_bounds__(P2L_THREADS) void pairb_symm_robust_keys_kernel(const float4* __restrict__ src4, const int32_t* __restrict__ perm,
                                                                             const int32_t* __restrict__ idx, const float* __restrict__ d2_in,
                                                                             const float* __restrict__ sn_all, const float* __restrict__ tgt_all,
                                                                             const float* __restrict__ nrm_all, const PairbDesc* __restrict__ desc,
                                                                             const int32_t* __restrict__ row_pair, const PairState* __restrict__ state,
                                                                             const RobustScale* __restrict__ rs, const SymmPass* __restrict__ pass,
                                                                             double max_d2, float* __restrict__ keys) {
    const int p = row_pair[blockIdx.x];
    if (!pairb_robust_selects(state, rs, p)) return;
    const PairbDesc d = desc[p];
    const SymmPass sp = pass[p];
    GicpRot Rn;
#pragma unroll
    for (int k = 0; k < 9; ++k) Rn.r[k] = sp.r[k];
    const float* tgt = tgt_all + 3 * d.tgt_off;
    const float* nrm = nrm_all + 3 * d.tgt_off;
    const int64_t step = (int64_t)d.nrows * P2L_THREADS;
    for (int64_t i = (int64_t)((int)blockIdx.x - d.row_base) * P2L_THREADS + threadIdx.x; i < d.ns; i += step) {
        float key = __uint_as_float(0x7fc00000u);
        RobustArg ra;
        ra.key = &key;
        double acc[P2L_NSUMS];   // (never read in this mode)
        symm_source<PERM ? SRC_F4_PERM : SRC_F4, PAIR_KEY>(acc, nullptr, src4, perm, idx, d2_in, sn_all, tgt, nrm, d.src_base + i, d.nt, max_d2, Rn,
                                                           sp.align, ra);
        keys[d.src_base + i] = key;
    }
}

template <bool PERM>
__global__ __launch_bounds__(P2L_THREADS) void pairb_symm_robust_rows_kernel(const float4* __restrict__ src4, const int32_t* __restrict__ perm,
                                                                             const int32_t* __restrict__ idx, const float* __restrict__ d2_in,
                                                                             const float* __restrict__ sn_all, const float* __restrict__ tgt_all,
                                                                             const float* __restrict__ nrm_all, const PairbDesc* __restrict__ desc,
                                                                             const int32_t* __restrict__ row_pair, const PairState* __restrict__ state,
                                                                             const RobustScale* __restrict__ rs, const TrimState* __restrict__ ts,
                                                                             const SymmPass* __restrict__ pass, double max_d2,
                                                                             double* __restrict__ rows) {
    __shared__ double sh[P2L_THREADS / 64][P2L_NSUMS];
    const int p = row_pair[blockIdx.x];
    if (!pairb_active(state, p)) return;
    const PairbDesc d = desc[p];
    const SymmPass sp = pass[p];
    GicpRot Rn;
#pragma unroll
    for (int k = 0; k < 9; ++k) Rn.r[k] = sp.r[k];
    double acc[P2L_NSUMS];
#pragma unroll
    for (int c = 0; c < P2L_NSUMS; ++c) acc[c] = 0.0;
    const RobustScale s = rs[p];
    RobustArg ra;
    ra.loss = s.loss;
    ra.c2 = robust_pass_c2(s, true, ts + p);
    const float* tgt = tgt_all + 3 * d.tgt_off;
    const float* nrm = nrm_all + 3 * d.tgt_off;
    const int64_t step = (int64_t)d.nrows * P2L_THREADS;
    for (int64_t i = (int64_t)((int)blockIdx.x - d.row_base) * P2L_THREADS + threadIdx.x; i < d.ns; i += step)
        symm_source<PERM ? SRC_F4_PERM : SRC_F4, PAIR_ROBUST>(acc, nullptr, src4, perm, idx, d2_in, sn_all, tgt, nrm, d.src_base + i, d.nt, max_d2, Rn,
                                                              sp.align, ra);
    const double r = block_sum<P2L_NSUMS>(acc, sh);
    if (threadIdx.x < P2L_NSUMS) rows[(int64_t)blockIdx.x * P2L_NSUMS + threadIdx.x] = r;
}

void launch_pairb_select(hipStream_t st, const float* d_d2, const PairbDesc* d_desc, int npairs, const PairState* d_state, double max_d2,
                         TrimState* d_ts, double* d_info) {
    hipLaunchKernelGGL(pairb_select_kernel, dim3(npairs), dim3(TRIM_HIST_THREADS), 0, st, d_d2, d_desc, d_state, max_d2, d_ts, d_info);
}

void launch_pairb_sums(hipStream_t st, bool plane, bool trimmed, const float4* d_src4, const int32_t* d_perm, const int32_t* d_idx,
                       const float* d_d2, const float* d_tgt3, const float* d_nrm3, const PairbDesc* d_desc, const int32_t* d_row_pair,
                       int total_rows, int npairs, const PairState* d_state, const TrimState* d_ts, double max_d2, double* d_rows,
                       double* d_out) {
    const dim3 g(total_rows), b(P2L_THREADS);
#define KSS_PAIRB_ROWS(PLANE, TRIM, PERM) \
    hipLaunchKernelGGL((pairb_rows_kernel<PLANE, TRIM, PERM>), g, b, 0, st, d_src4, d_perm, d_idx, d_d2, d_tgt3, d_nrm3, d_desc, d_row_pair, d_state, d_ts, max_d2, d_rows)
    if (plane) {
        if (trimmed) { if (d_perm) KSS_PAIRB_ROWS(true, true, true); else KSS_PAIRB_ROWS(true, true, false); }
        else { if (d_perm) KSS_PAIRB_ROWS(true, false, true); else KSS_PAIRB_ROWS(true, false, false); }
        hipLaunchKernelGGL(pairb_final_kernel<true>, dim3(npairs), b, 0, st, (const double*)d_rows, d_desc, d_state, d_out);
    } else {   // (the untrimmed point metric is kss_icp_batch's)
        if (d_perm) KSS_PAIRB_ROWS(false, true, true); else KSS_PAIRB_ROWS(false, true, false);
        hipLaunchKernelGGL(pairb_final_kernel<false>, dim3(npairs), b, 0, st, (const double*)d_rows, d_desc, d_state, d_out);
    }
#undef KSS_PAIRB_ROWS
}

void launch_pairb_gicp_sums(hipStream_t st, const float4* d_src4, const int32_t* d_perm, const int32_t* d_idx, const float* d_d2,
                            const float* d_sn3, const float* d_tgt3, const float* d_nrm3, const PairbDesc* d_desc, const int32_t* d_row_pair,
                            int total_rows, int npairs, const PairState* d_state, const GicpPass* d_pass, double max_d2, double* d_rows,
                            double* d_out) {
    const dim3 g(total_rows), b(P2L_THREADS);
    if (d_perm)
        hipLaunchKernelGGL(pairb_gicp_rows_kernel<true>, g, b, 0, st, d_src4, d_perm, d_idx, d_d2, d_sn3, d_tgt3, d_nrm3, d_desc, d_row_pair, d_state, d_pass, max_d2, d_rows);
    else
        hipLaunchKernelGGL(pairb_gicp_rows_kernel<false>, g, b, 0, st, d_src4, d_perm, d_idx, d_d2, d_sn3, d_tgt3, d_nrm3, d_desc, d_row_pair, d_state, d_pass, max_d2, d_rows);
    hipLaunchKernelGGL(pairb_final_kernel<true>, dim3(npairs), b, 0, st, (const double*)d_rows, d_desc, d_state, d_out);
}

void launch_pairb_symm_sums(hipStream_t st, const float4* d_src4, const int32_t* d_perm, const int32_t* d_idx, const float* d_d2,
                            const float* d_sn3, const float* d_tgt3, const float* d_nrm3, const PairbDesc* d_desc, const int32_t* d_row_pair,
                            int total_rows, int npairs, const PairState* d_state, const SymmPass* d_pass, double max_d2, double* d_rows,
                            double* d_out) {
    const dim3 g(total_rows), b(P2L_THREADS);
    if (d_perm)
        hipLaunchKernelGGL(pairb_symm_rows_kernel<true>, g, b, 0, st, d_src4, d_perm, d_idx, d_d2, d_sn3, d_tgt3, d_nrm3, d_desc, d_row_pair, d_state, d_pass, max_d2, d_rows);
    else
        hipLaunchKernelGGL(pairb_symm_rows_kernel<false>, g, b, 0, st, d_src4, d_perm, d_idx, d_d2, d_sn3, d_tgt3, d_nrm3, d_desc, d_row_pair, d_state, d_pass, max_d2, d_rows);
    hipLaunchKernelGGL(pairb_final_kernel<true>, dim3(npairs), b, 0, st, (const double*)d_rows, d_desc, d_state, d_out);
}

void launch_pairb_robust_select(hipStream_t st, bool plane, const float4* d_src4, const int32_t* d_perm, const int32_t* d_idx, const float* d_d2,
                                const float* d_tgt3, const float* d_nrm3, const PairbDesc* d_desc, const int32_t* d_row_pair, int total_rows,
                                int npairs, const PairState* d_state, const RobustScale* d_rs, double max_d2, float* d_keys, TrimState* d_ts) {
    const float* keys = d_d2;   // the point metric's keys are the NN pass's d2, the plane metric's are written here
    double bound = max_d2;
    if (plane) {
        const dim3 g(total_rows), b(P2L_THREADS);
        if (d_perm)
            hipLaunchKernelGGL(pairb_robust_keys_kernel<true>, g, b, 0, st, d_src4, d_perm, d_idx, d_d2, d_tgt3, d_nrm3, d_desc, d_row_pair, d_state, d_rs, max_d2, d_keys);
        else
            hipLaunchKernelGGL(pairb_robust_keys_kernel<false>, g, b, 0, st, d_src4, d_perm, d_idx, d_d2, d_tgt3, d_nrm3, d_desc, d_row_pair, d_state, d_rs, max_d2, d_keys);
        keys = d_keys;
        bound = __builtin_huge_val();
    }
    hipLaunchKernelGGL(pairb_robust_select_kernel, dim3(npairs), dim3(TRIM_HIST_THREADS), 0, st, keys, d_desc, d_state, d_rs, bound, d_ts);
}

void launch_pairb_robust_sums(hipStream_t st, bool plane, const float4* d_src4, const int32_t* d_perm, const int32_t* d_idx, const float* d_d2,
                              const float* d_tgt3, const float* d_nrm3, const PairbDesc* d_desc, const int32_t* d_row_pair, int total_rows,
                              int npairs, const PairState* d_state, const RobustScale* d_rs, const TrimState* d_ts, double max_d2,
                              double* d_rows, double* d_out, double* d_info) {
    const dim3 g(total_rows), b(P2L_THREADS);
#define KSS_PAIRB_ROBUST_ROWS(PLANE, PERM) \
    hipLaunchKernelGGL((pairb_robust_rows_kernel<PLANE, PERM>), g, b, 0, st, d_src4, d_perm, d_idx, d_d2, d_tgt3, d_nrm3, d_desc, d_row_pair, d_state, d_rs, d_ts, max_d2, d_rows)
    if (plane) {
        if (d_perm) KSS_PAIRB_ROBUST_ROWS(true, true); else KSS_PAIRB_ROBUST_ROWS(true, false);
        hipLaunchKernelGGL(pairb_robust_final_kernel<true>, dim3(npairs), b, 0, st, (const double*)d_rows, d_desc, d_state, d_rs, d_ts, d_out, d_info);
    } else {
        if (d_perm) KSS_PAIRB_ROBUST_ROWS(false, true); else KSS_PAIRB_ROBUST_ROWS(false, false);
        hipLaunchKernelGGL(pairb_robust_final_kernel<false>, dim3(npairs), b, 0, st, (const double*)d_rows, d_desc, d_state, d_rs, d_ts, d_out, d_info);
    }
#undef KSS_PAIRB_ROBUST_ROWS
}

void launch_pairb_symm_robust_select(hipStream_t st, const float4* d_src4, const int32_t* d_perm, const int32_t* d_idx, const float* d_d2,
                                     const float* d_sn3, const float* d_tgt3, const float* d_nrm3, const PairbDesc* d_desc,
                                     const int32_t* d_row_pair, int total_rows, int npairs, const PairState* d_state, const RobustScale* d_rs,
                                     const SymmPass* d_pass, double max_d2, float* d_keys, TrimState* d_ts) {
    const dim3 g(total_rows), b(P2L_THREADS);
    if (d_perm)
        hipLaunchKernelGGL(pairb_symm_robust_keys_kernel<true>, g, b, 0, st, d_src4, d_perm, d_idx, d_d2, d_sn3, d_tgt3, d_nrm3, d_desc, d_row_pair, d_state, d_rs, d_pass, max_d2, d_keys);
    else
        hipLaunchKernelGGL(pairb_symm_robust_keys_kernel<false>, g, b, 0, st, d_src4, d_perm, d_idx, d_d2, d_sn3, d_tgt3, d_nrm3, d_desc, d_row_pair, d_state, d_rs, d_pass, max_d2, d_keys);
    // the keys carry the whole candidate test (a NaN is none): no bound
    hipLaunchKernelGGL(pairb_robust_select_kernel, dim3(npairs), dim3(TRIM_HIST_THREADS), 0, st, (const float*)d_keys, d_desc, d_state, d_rs,
                       __builtin_huge_val(), d_ts);
}

void launch_pairb_symm_robust_sums(hipStream_t st, const float4* d_src4, const int32_t* d_perm, const int32_t* d_idx, const float* d_d2,
                                   const float* d_sn3, const float* d_tgt3, const float* d_nrm3, const PairbDesc* d_desc,
                                   const int32_t* d_row_pair, int total_rows, int npairs, const PairState* d_state, const RobustScale* d_rs,
                                   const TrimState* d_ts, const SymmPass* d_pass, double max_d2, double* d_rows, double* d_out, double* d_info) {
    const dim3 g(total_rows), b(P2L_THREADS);
    if (d_perm)
        hipLaunchKernelGGL(pairb_symm_robust_rows_kernel<true>, g, b, 0, st, d_src4, d_perm, d_idx, d_d2, d_sn3, d_tgt3, d_nrm3, d_desc, d_row_pair, d_state, d_rs, d_ts, d_pass, max_d2, d_rows);
    else
        hipLaunchKernelGGL(pairb_symm_robust_rows_kernel<false>, g, b, 0, st, d_src4, d_perm, d_idx, d_d2, d_sn3, d_tgt3, d_nrm3, d_desc, d_row_pair, d_state, d_rs, d_ts, d_pass, max_d2, d_rows);
    hipLaunchKernelGGL(pairb_robust_final_kernel<true>, dim3(npairs), b, 0, st, (const double*)d_rows, d_desc, d_state, d_rs, d_ts, d_out, d_info);
}

}  // namespace kss
