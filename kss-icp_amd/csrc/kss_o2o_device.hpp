// kss_o2o_device.hpp -- the candidate test, the claim key and the workgroup count of the correspondence rejectors: kss_o2o.hip
// (one-to-one) and kss_recip.hip (reciprocal) state them once, here.
#pragma once
#include "kss_internal.hpp"

namespace kss {

constexpr int O2O_THREADS = 256;

__device__ __forceinline__ bool o2o_candidate(int32_t j, float d2f, int64_t nt, double max_d2) {
    const double d = (double)d2f;
    return j >= 0 && (int64_t)j < nt && d >= 0.0 && d <= max_d2;
}
__device__ __forceinline__ unsigned long long o2o_key(float d2f, int64_t i) {
    return ((unsigned long long)(__float_as_uint(d2f) & 0x7fffffffu) << 32) | (unsigned long long)(unsigned)i;
}

// adds the number of lanes with `flag` set, over the workgroup's whole walk, to *counter: ballot + popcount per step in cnt (the
// same value in every lane of a wave), here the waves' totals through LDS and one atomic
__device__ __forceinline__ void o2o_count(unsigned cnt, unsigned* wave_cnt, unsigned* counter) {
    if ((threadIdx.x & 63) == 0) wave_cnt[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned tot = 0u;
        for (int w = 0; w < O2O_THREADS / 64; ++w) tot += wave_cnt[w];
        if (tot) atomicAdd(counter, tot);
    }
}

}  // namespace kss
