// kss_o2o.hip -- one-to-one rejection in front of the trimmed pass (PCL's CorrespondenceRejectorOneToOne; the
// definition at kss_icp_o2o in include/kssicp.h): of all sources that chose one target, only the closest keeps its correspondence.
// Per pass THREE launches over the NN pass's idx / d2 (by original source index):
//   reset    hipMemsetAsync to all ones of the CLAIM TABLE -- one uint64 per target, for a batch one table over all its targets,
//            target j of a pair at PairbDesc::tgt_off + j -- and of the two uint32 counters per pair that lie behind it.
//   claim    o2o_claim_kernel: every candidate (idx in [0, nt), 0 <= d2 <= max_d2 in ordered double compares) issues ONE 64-bit
//            unsigned atomicMin, no return value, of key = (bits(d2) & 0x7fffffff) << 32 | i into its target's slot (i: the source's
//            index inside its pair).  A minimum does not depend on the order of its operands: the table is the same in every run.
//            Candidates are counted per wave by ballot and popcount; ONE integer atomic per workgroup adds them to the pair's counter 0.
//   resolve  o2o_resolve_kernel: a candidate whose key is its slot's value is the WINNER and keeps idx / d2 bit for bit; a loser gets
//            idx = -1 and d2 = the quiet NaN 0x7fc00000; a source that is no candidate passes through.  Winners are counted the same
//            way into counter 1.  The first workgroup of a pair publishes m -- counter 0, complete since the claim launch ended -- to
//            the info record where one is given.
// A counter starts at all ones like the table: it holds its count MINUS ONE (mod 2^32), and whoever reads it adds one.
// The grid is pairb_rows_kernel's: stream_blocks(ns_p) workgroups of 256 per pair through the row -> pair table; a single pair is
// a batch of one descriptor without the table.  Workgroups of a pair that is no longer active leave at once and write nothing.
// The filtered arrays feed the selection, the rows and the final launches unchanged: every per-source body skips an idx outside
// [0, nt) and the selection takes a NaN d2 as no candidate.
#include "kss_o2o_device.hpp"

namespace kss {

// row_pair null: one pair, desc[0]
template <bool RESOLVE>
__global__ __launch_bounds__(O2O_THREADS) void o2o_kernel(const O2oArgs a) {
    __shared__ unsigned wave_cnt[O2O_THREADS / 64];
    const int p = a.row_pair ? a.row_pair[blockIdx.x] : 0;
    if (a.state && a.state[p].active == 0) return;
    const PairbDesc d = a.desc[p];
    const int32_t* idx = a.idx + d.src_base;
    const float* d2 = a.d2 + d.src_base;
    unsigned long long* table = a.table + d.tgt_off;
    unsigned* counters = a.counters + 2 * (int64_t)p;
    const int64_t first = (int64_t)((int)blockIdx.x - d.row_base) * O2O_THREADS;
    const int64_t step = (int64_t)d.nrows * O2O_THREADS;
    unsigned cnt = 0u;
    for (int64_t i0 = first; i0 < d.ns; i0 += step) {   // (i0 is the same in every lane: the ballots below are whole waves')
        const int64_t i = i0 + threadIdx.x;
        const bool live = i < d.ns;
        const int32_t j = live ? idx[i] : -1;
        const float v = live ? d2[i] : __uint_as_float(0x7fc00000u);
        const bool cand = live && o2o_candidate(j, v, d.nt, a.max_d2);
        if constexpr (!RESOLVE) {
            if (cand) atomicMin(&table[j], o2o_key(v, i));
            cnt += (unsigned)__popcll(__ballot(cand));
        } else {
            const bool win = cand && table[j] == o2o_key(v, i);
            if (live) {
                if (a.idx_out) a.idx_out[d.src_base + i] = cand && !win ? -1 : j;
                if (a.d2_out) a.d2_out[d.src_base + i] = cand && !win ? __uint_as_float(0x7fc00000u) : v;
            }
            cnt += (unsigned)__popcll(__ballot(win));
        }
    }
    o2o_count(cnt, wave_cnt, counters + (RESOLVE ? 1 : 0));
    if constexpr (RESOLVE) {
        if (a.info_m && (int)blockIdx.x == d.row_base && threadIdx.x == 0) a.info_m[p] = (double)(counters[0] + 1u);
    }
}

size_t o2o_table_bytes(int64_t total_tgt, int npairs) { return (size_t)total_tgt * sizeof(unsigned long long) + (size_t)npairs * 2 * sizeof(unsigned); }

// the three launches; a.table holds o2o_table_bytes(total_tgt, npairs), a.counters lies behind the total_tgt slots
int launch_o2o(hipStream_t st, int total_rows, int64_t total_tgt, int npairs, const O2oArgs& a) {
    const hipError_t e = hipMemsetAsync(a.table, 0xff, o2o_table_bytes(total_tgt, npairs), st);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(o2o_kernel<false>, dim3(total_rows), dim3(O2O_THREADS), 0, st, a);
    hipLaunchKernelGGL(o2o_kernel<true>, dim3(total_rows), dim3(O2O_THREADS), 0, st, a);
    return 0;
}

}  // namespace kss
