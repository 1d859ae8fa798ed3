// kss_trim.hip -- trimmed ICP (Chetverikov et al., TrICP): the exact k-th smallest squared distance of a pass,
// found on the device, and the point-metric sums over the correspondences at or below it.
//
// Selection.  A candidate is a d2 with 0 <= d2 <= max_d2 (ordered compares in double: a NaN is none); its KEY is its bit
// pattern, -0.0f taken as +0.0f: non-negative floats order as unsigned integers.  Radix select over the 31 key bits in three
// digits (11 + 10 + 10 bits, most significant first), FOUR plain launches:
//   trim_step_kernel<d>  d = 0, 1, 2: trim_hist_blocks(n) workgroups of 256.  For d > 0 every workgroup first RESOLVES digit
//                        d - 1 for itself (trim_resolve: column sums of the previous launch's histogram rows -- integers, any
//                        order gives the same count --, a workgroup prefix scan, the bin that holds the rank; the same answer in
//                        every workgroup, workgroup 0 also stores it as TrimState[d]).  Then it counts its keys that carry the
//                        prefix into a 2048-bin LDS histogram (integer LDS atomics) and writes it out as ONE PLAIN ROW of its
//                        own.  Resolving digit 0 also yields m (all candidates) and k = trim_rank_of(m, overlap).
//   trim_last_kernel     one workgroup: resolves digit 2: tau, the cut for the sums kernels and the info record (TrimState[3]
//                        in device memory for the sums kernels of the same pass + host-mapped memory).
// No counter, no flag, no atomic across workgroups: the hand-over is the launch boundary, and nothing has to be zero at rest
// (rows are rewritten in full; the row buffers of consecutive digits alternate, step d reads TrimState[d] and writes [d + 1]).
// m, k, tau are functions of the input values alone: the grid size only decides which row a key is counted in.
// (First form: a one-workgroup scan launch behind every histogram launch, six launches of 5-8 us each = 37 us at 100k keys;
// every launch costs that whatever it does, so the scans moved into the launches that need their answer.)
//
// Point-metric sums.  The rows are pair_rows_kernel<PointTrimMetric, SRC>'s (kss_pair.hip: the walk of every pair metric, on
// accumulate_corr's arithmetic); trim_point_final_kernel adds them with rows_column_sum's fixed order.  The plane metric uses
// pair_rows_kernel<PlaneMetric<true>, SRC>, which reads the same cut.
#pragma clang fp contract(off)

#include "kss_pair_device.hpp"

namespace kss {

// (TRIM_BINS, the digits, trim_key and the resolution of a digit from bin counts: kss_pair_device.hpp, shared with the batch)
constexpr int TRIM_KEYS_PER_BLOCK = 4096;       // >= 16 keys per lane before another histogram row (8 KB) is added
constexpr int TRIM_MAX_BLOCKS = 128;            // every workgroup of the next step reads all rows (L2): 1 MB each at most

int trim_hist_blocks(int64_t n) {
    int64_t b = (n + TRIM_KEYS_PER_BLOCK - 1) / TRIM_KEYS_PER_BLOCK;
    if (b > TRIM_MAX_BLOCKS) b = TRIM_MAX_BLOCKS;
    if (b < 1) b = 1;
    return (int)b;
}

// Resolves digit DIGIT from its histogram rows: the state after it (prefix, rank inside the keys that carry it, m, k; after the
// last digit cut and kept) in *out (LDS), valid for every lane after the call.  st[DIGIT] is the state before it (digit 0 has
// none: m is the total of the rows).  Needs blockDim.x == TRIM_HIST_THREADS; lane t owns the bins 8t .. 8t + 7.
template <int DIGIT>
__device__ __forceinline__ void trim_resolve(const unsigned* __restrict__ rows, int nrows, double overlap,
                                             const TrimState* __restrict__ st, TrimState* out, unsigned* wave_tot) {
    const int t = threadIdx.x;
    unsigned c[TRIM_LANE_BINS];
#pragma unroll
    for (int q = 0; q < TRIM_LANE_BINS; ++q) c[q] = 0u;
    {
        // Eight rows = sixteen 16-byte loads in flight per lane: the loop is a chain of memory latencies, not of bytes (two
        // rows at a time cost 6 us at 25 rows).  Rows past the end are loaded from the batch's first row and not added.
        const uint4* r4 = (const uint4*)rows + 2 * t;
        for (int r = 0; r < nrows; r += 8) {
            uint4 a[8], b[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const size_t row = (size_t)(r + u < nrows ? r + u : r) * (TRIM_BINS / 4);
                a[u] = r4[row]; b[u] = r4[row + 1];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if (r + u < nrows) {
                    c[0] += a[u].x; c[1] += a[u].y; c[2] += a[u].z; c[3] += a[u].w;
                    c[4] += b[u].x; c[5] += b[u].y; c[6] += b[u].z; c[7] += b[u].w;
                }
            }
        }
    }
    trim_resolve_counts<DIGIT>(c, overlap, st + DIGIT, out, wave_tot);
}

template <int DIGIT>
__global__ __launch_bounds__(TRIM_HIST_THREADS) void trim_step_kernel(const float* __restrict__ d2, int64_t n, double max_d2, double overlap,
                                                                      const unsigned* __restrict__ rows_prev, int nrows_prev,
                                                                      TrimState* __restrict__ st, unsigned* __restrict__ rows) {
    __shared__ unsigned hist[TRIM_BINS];
    __shared__ TrimState cur;
    __shared__ unsigned wave_tot[TRIM_HIST_THREADS / 64];
    for (int b = threadIdx.x; b < TRIM_BINS; b += TRIM_HIST_THREADS) hist[b] = 0u;
    unsigned prefix = 0u;
    bool any = true;
    if constexpr (DIGIT > 0) {
        trim_resolve<DIGIT - 1>(rows_prev, nrows_prev, overlap, st, &cur, wave_tot);
        prefix = cur.prefix;
        any = cur.rank > 0;     // no candidate at all: nothing to count
        if (blockIdx.x == 0 && threadIdx.x == 0) st[DIGIT] = cur;
    } else {
        __syncthreads();
    }
    if (any) {
        // eight loads in flight per lane (one at a time is one memory latency per key: 16 keys per lane took 8 us); a slot past
        // the end holds a NaN, which is no candidate
        const int64_t stride = (int64_t)gridDim.x * TRIM_HIST_THREADS;
        for (int64_t i0 = (int64_t)blockIdx.x * TRIM_HIST_THREADS + threadIdx.x; i0 < n; i0 += 8 * stride) {
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
    unsigned* row = rows + (size_t)blockIdx.x * TRIM_BINS;
    for (int b = threadIdx.x; b < TRIM_BINS; b += TRIM_HIST_THREADS) row[b] = hist[b];
}

__global__ __launch_bounds__(TRIM_HIST_THREADS) void trim_last_kernel(const unsigned* __restrict__ rows_prev, int nrows_prev, double overlap,
                                                                      TrimState* __restrict__ st, double* __restrict__ info_out) {
    __shared__ TrimState cur;
    __shared__ unsigned wave_tot[TRIM_HIST_THREADS / 64];
    trim_resolve<2>(rows_prev, nrows_prev, overlap, st, &cur, wave_tot);
    if (threadIdx.x == 0) {
        st[3] = cur;
        if (info_out) {
            info_out[0] = (double)cur.m; info_out[1] = (double)cur.k;
            info_out[2] = cur.rank > 0 ? cur.cut : 0.0;
            info_out[3] = (double)cur.kept;
        }
    }
}

// d_rows: two row buffers of trim_hist_blocks(n) rows each (consecutive digits alternate between them)
void launch_trim_select(hipStream_t st, const float* d_d2, int64_t n, double max_d2, double overlap, unsigned* d_rows,
                        TrimState* d_state, double* d_info) {
    const int nb = trim_hist_blocks(n);
    unsigned* ra = d_rows;
    unsigned* rb = d_rows + (size_t)nb * TRIM_BINS;
    const dim3 g(nb), b(TRIM_HIST_THREADS);
    hipLaunchKernelGGL(trim_step_kernel<0>, g, b, 0, st, d_d2, n, max_d2, overlap, (const unsigned*)nullptr, 0, d_state, ra);
    hipLaunchKernelGGL(trim_step_kernel<1>, g, b, 0, st, d_d2, n, max_d2, overlap, (const unsigned*)ra, nb, d_state, rb);
    hipLaunchKernelGGL(trim_step_kernel<2>, g, b, 0, st, d_d2, n, max_d2, overlap, (const unsigned*)rb, nb, d_state, ra);
    hipLaunchKernelGGL(trim_last_kernel, dim3(1), b, 0, st, (const unsigned*)ra, nb, overlap, d_state, d_info);
}

size_t trim_rows_bytes(int64_t n) { return 2 * (size_t)trim_hist_blocks(n) * TRIM_BINS * sizeof(unsigned); }

// ---- point-metric sums over the kept correspondences: the final launch ----------------------------------------------------
// slots 17 and 18 stay 0 as in an ICP iteration of kss_icp, 19 is 0
__global__ __launch_bounds__(TRIM_THREADS) void trim_point_final_kernel(const double* __restrict__ rows, int nrows, double* __restrict__ out) {
    __shared__ double shg[ROWSUM_GROUPS][NSUMS];
    const double v = rows_column_sum(rows, nrows, shg);
    if (threadIdx.x < NSUMS) out[threadIdx.x] = threadIdx.x >= 17 ? 0.0 : v;
}

// similarity ICP: the same column sums, slot 17 (the kept sources' sum of squares) kept, 18 and 19 are 0
__global__ __launch_bounds__(TRIM_THREADS) void sim_final_kernel(const double* __restrict__ rows, int nrows, double* __restrict__ out) {
    __shared__ double shg[ROWSUM_GROUPS][NSUMS];
    const double v = rows_column_sum(rows, nrows, shg);
    if (threadIdx.x < NSUMS) out[threadIdx.x] = threadIdx.x >= 18 ? 0.0 : v;
}

void launch_sim_final(hipStream_t st, const double* d_rows, int nrows, double* d_out) {
    hipLaunchKernelGGL(sim_final_kernel, dim3(1), dim3(TRIM_THREADS), 0, st, d_rows, nrows, d_out);
}

void launch_trim_point_final(hipStream_t st, const double* d_rows, int nrows, double* d_out) {
    hipLaunchKernelGGL(trim_point_final_kernel, dim3(1), dim3(TRIM_THREADS), 0, st, d_rows, nrows, d_out);
}

}  // namespace kss
