// kss_device.hpp -- device-side helpers shared by kss_kernels.hip and kss_grid.hip (gfx950).
#pragma once
#include <hip/hip_runtime.h>

#include "kss_internal.hpp"

namespace kss {

template <bool FMA>
__device__ __forceinline__ float dist2(float sx, float sy, float sz, float tx, float ty, float tz) {
    const float dx = sx - tx, dy = sy - ty, dz = sz - tz;
    if constexpr (FMA) {
        return __builtin_fmaf(dx, dx, __builtin_fmaf(dy, dy, dz * dz));
    } else {
        return (dx * dx + dy * dy) + dz * dz;   // FLANN L2_Simple: result += diff*diff in x,y,z order
    }
}

// cell of a coordinate in a uniform grid (clamped to the grid: queries outside the bbox belong to the border cells)
__device__ __forceinline__ int cell_coord(float v, float o, float inv_h, int g) {
    int c = (int)floorf((v - o) * inv_h);
    c = c < 0 ? 0 : c;
    return c >= g ? g - 1 : c;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// Block-wide sum of NV doubles per thread (256 threads = 4 waves). Result valid in thread c < NV.
template <int NV>
__device__ __forceinline__ double block_sum(const double (&v)[NV], double (*sh)[NV]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < NV; ++c) {
        const double r = wave_sum(v[c]);
        if (lane == 0) sh[wave][c] = r;
    }
    __syncthreads();
    double out = 0.0;
    if (threadIdx.x < NV) {
        const int nw = (blockDim.x + 63) >> 6;
        for (int w = 0; w < nw; ++w) out += sh[w][threadIdx.x];   // fixed order: reproducible
    }
    return out;
}


// Column sums of `nrows` partial rows (NSUMS doubles each) by one 256-lane workgroup, bitwise reproducible:
// lane (g, c) = (tid / NSUMS, tid % NSUMS) adds rows g, g+12, g+24, ... of column c with four independent
// accumulators (many loads in flight: the rows come from other CUs' L2 / HBM), then the 12 group totals are
// added in group order.  Returns the column total in lanes tid < NSUMS.  Needs blockDim.x == 256.
constexpr int ROWSUM_GROUPS = 12;   // 12 * 20 = 240 of the 256 lanes
__device__ __forceinline__ double rows_column_sum(const double* __restrict__ rows, int nrows, double (*shg)[NSUMS]) {
    const int g = threadIdx.x / NSUMS, c = threadIdx.x % NSUMS;
    if (g < ROWSUM_GROUPS) {
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, a4 = 0.0, a5 = 0.0, a6 = 0.0, a7 = 0.0;
        int k = g;
        constexpr int G = ROWSUM_GROUPS;
        for (; k + 7 * G < nrows; k += 8 * G) {
            a0 += rows[(int64_t)(k) * NSUMS + c];
            a1 += rows[(int64_t)(k + G) * NSUMS + c];
            a2 += rows[(int64_t)(k + 2 * G) * NSUMS + c];
            a3 += rows[(int64_t)(k + 3 * G) * NSUMS + c];
            a4 += rows[(int64_t)(k + 4 * G) * NSUMS + c];
            a5 += rows[(int64_t)(k + 5 * G) * NSUMS + c];
            a6 += rows[(int64_t)(k + 6 * G) * NSUMS + c];
            a7 += rows[(int64_t)(k + 7 * G) * NSUMS + c];
        }
        for (; k < nrows; k += G) a0 += rows[(int64_t)k * NSUMS + c];
        a0 = (a0 + a1) + (a2 + a3);
        a2 = (a4 + a5) + (a6 + a7);
        a1 = 0.0; a3 = 0.0;
        a0 = a0 + a2; a2 = 0.0;
        shg[g][c] = (a0 + a1) + (a2 + a3);
    }
    __syncthreads();
    double v = 0.0;
    if (threadIdx.x < NSUMS)
        for (int gg = 0; gg < ROWSUM_GROUPS; ++gg) v += shg[gg][threadIdx.x];
    return v;
}

// ---- row hand-over: the one way a reduction's rows reach the workgroup that adds them up --------------------------------
// Every workgroup of a reduction that spans several leaves one row of sums.  Each value travels as a GRANULE {bits(value),
// sequence number of its launch or pass}, written by ONE 16-byte write-through (sc1) store: no drain, no flag, no counter.
// The reducer accepts a granule when it carries the number it expects, so nothing has to be reset between launches (a
// granule of another launch carries another number; a granule buffer is zeroed when it is (re)allocated, and numbers
// start at 1).  A reducer that waits inside its launch holds a workgroup slot while it polls: it may wait there only where
// the launch has at most one waiter per compute unit -- the other workgroups never wait, so they all get to run (HIP
// promises no dispatch order).  Otherwise the rows are added up by the next launch.
// granule `col` of a row: `row` is the same in every lane (a scalar base; the lane's offset is formed inside the asm, where
// the compiler cannot hoist it and keep it live across the kernel: two registers and one wave per SIMD in cand_pass_kernel)
__device__ __forceinline__ void row_put(Granule* row, int col, double v, unsigned long long seq) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    u32x4 o;
    o.x = (unsigned)b; o.y = (unsigned)(b >> 32); o.z = (unsigned)seq; o.w = (unsigned)(seq >> 32);
    unsigned off;
    asm volatile("v_lshlrev_b32 %0, 4, %2\n\tglobal_store_dwordx4 %0, %1, %3 sc1" : "=&v"(off) : "v"(o), "v"(col), "s"(row) : "memory");
}

// Sum of column `col` over the rows first, first + stride, ... < n (ncols granules per row), added in increasing row
// order, eight sc1 loads in flight per poll.  A batch of eight is accepted when every granule carries `seq`; the wave sleeps
// between polls (the ballot keeps the loads convergent).  More than `polls` polls, or stop() (asked every 32 polls),
// ends the wait: returns false.  `rows` is the same in every lane (scalar base + 32-bit lane offsets: half the address
// registers) and spans less than 4 GB.
struct NoStop { __device__ bool operator()() const { return false; } };
template <typename Stop = NoStop>
__device__ __forceinline__ bool rows_take(const Granule* __restrict__ rows, int ncols, int col, int first, int stride, int n,
                                          unsigned long long seq, int polls, double& sum, Stop stop = Stop()) {
    const unsigned lo = (unsigned)seq, hi = (unsigned)(seq >> 32);
    double acc = 0.0;
    for (int k = first; k < n; k += 8 * stride) {
        unsigned o[8];   // byte offsets
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (unsigned)((k + j * stride < n ? k + j * stride : k) * ncols + col) * (unsigned)sizeof(Granule);
        u32x4 t0, t1, t2, t3, t4, t5, t6, t7;
        int spins = 0;
        for (;;) {
            asm volatile(
                "global_load_dwordx4 %0, %8, %16 sc1\n\tglobal_load_dwordx4 %1, %9, %16 sc1\n\t"
                "global_load_dwordx4 %2, %10, %16 sc1\n\tglobal_load_dwordx4 %3, %11, %16 sc1\n\t"
                "global_load_dwordx4 %4, %12, %16 sc1\n\tglobal_load_dwordx4 %5, %13, %16 sc1\n\t"
                "global_load_dwordx4 %6, %14, %16 sc1\n\tglobal_load_dwordx4 %7, %15, %16 sc1\n\t"
                "s_waitcnt vmcnt(0)"
                : "=&v"(t0), "=&v"(t1), "=&v"(t2), "=&v"(t3), "=&v"(t4), "=&v"(t5), "=&v"(t6), "=&v"(t7)
                : "v"(o[0]), "v"(o[1]), "v"(o[2]), "v"(o[3]), "v"(o[4]), "v"(o[5]), "v"(o[6]), "v"(o[7]), "s"(rows)
                : "memory");
            const bool ok = t0.z == lo && t0.w == hi && t1.z == lo && t1.w == hi && t2.z == lo && t2.w == hi && t3.z == lo && t3.w == hi &&
                            t4.z == lo && t4.w == hi && t5.z == lo && t5.w == hi && t6.z == lo && t6.w == hi && t7.z == lo && t7.w == hi;
            if (__builtin_amdgcn_ballot_w64(!ok) == 0ull) break;
            if (++spins > polls || ((spins & 31) == 0 && stop())) return false;
            __builtin_amdgcn_s_sleep(1);
        }
        const u32x4 tt[8] = {t0, t1, t2, t3, t4, t5, t6, t7};
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (k + j * stride < n) acc += __longlong_as_double((long long)(((unsigned long long)tt[j].y << 32) | tt[j].x));
    }
    sum = acc;
    return true;
}

// The reducer's column totals of n rows of NSUMS granules: lane slot (g, c) adds rows g, g + G, g + 2G, ... of column c
// (rows_take), then the G group totals are added in group order -- a function of the rows only.  The result is valid in
// lanes tid < NSUMS; false (in every lane) when a row never came.  shg: G x NSUMS doubles of LDS.
template <int G, typename Stop = NoStop>
__device__ __forceinline__ bool rows_total(const Granule* __restrict__ rows, int n, unsigned long long seq, int polls,
                                           double (*shg)[NSUMS], int* s_ok, double& v, Stop stop = Stop()) {
    if (threadIdx.x == 0) *s_ok = 1;
    __syncthreads();
    for (int t = (int)threadIdx.x; t < G * NSUMS; t += (int)blockDim.x) {
        const int g = t / NSUMS, c = t % NSUMS;
        if (!rows_take(rows, NSUMS, c, g, G, n, seq, polls, shg[g][c], stop)) *s_ok = 0;
    }
    __syncthreads();
    v = 0.0;
    if (threadIdx.x < NSUMS)
        for (int gg = 0; gg < G; ++gg) v += shg[gg][threadIdx.x];
    return *s_ok != 0;
}

// One published value: {bits(v), low word of seq, check word of those three} as ONE aligned 16-byte system-scope store into
// host-mapped memory (slot `slot` of pub).  The host takes a slot when the number matches and the check word fits, so no
// flag has to be ordered after the data and no L2 write-back is needed (the reader: slots_collect, kss_handover.hpp).  torn_xor != 0 (test hook only): the bits are
// stored altered, the check word of the true ones -- a slot as a torn read would see it.
__device__ __forceinline__ void pub_put(unsigned long long* pub, int64_t slot, double v, unsigned long long seq, unsigned torn_xor = 0u) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    u32x4 o;
    o.x = (unsigned)b; o.y = (unsigned)(b >> 32); o.z = (unsigned)seq; o.w = kss_mix3(o.x, o.y, o.z);
    o.x ^= torn_xor;
    unsigned long long* dst = pub + 2 * slot;
    asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1" ::"v"(dst), "v"(o) : "memory");
}

// ---- the canonical summation order of the fused cell-list pass (grid_pass_kernel) ------------------------------
// One ROW = the sums over one CHUNK of 512 consecutive (cell-sorted) sources of a pair: lane t holds source
// 512 * chunk + t.  Per f64 column the row value is a fixed binary tree over the 64 lanes of each wave -- partners at lane
// distance 32, then 16, 8, 4, 2, 1 -- followed by the 8 wave totals added in wave order.  The pair total adds the rows
// k = g, g + 25, g + 50, ... sequentially for each of 25 groups g, then the 25 group totals in group order.  Everything
// is a function of the pair's source count only, so a pair gives the same bits alone or inside a batch, whatever the
// grid size, and IEEE addition being commutative the tree can be evaluated with any exchange primitive.
constexpr int PASS_BS = 512;                  // lanes per workgroup == sources per chunk / row
constexpr int PASS_FG = PASS_BS / NSUMS;      // 25 row groups of the pair total

template <typename F>
__device__ __forceinline__ double dpp_f64(double x, F f) {
    const int lo = f(__double2loint(x)), hi = f(__double2hiint(x));
    return __hiloint2double(hi, lo);
}
// value of lane (l ^ d) for d = 8, 4, 2, 1 (inside a row of 16 lanes: DPP, no LDS)
// (every lane is written: no "old" value to keep -- with one, the compiler copies the register first, two moves per exchange)
__device__ __forceinline__ double xor8(double x) { return dpp_f64(x, [](int v) { return __builtin_amdgcn_mov_dpp(v, 0x128, 0xf, 0xf, false); }); }   // row_ror:8
__device__ __forceinline__ double xor4(double x) {
    return dpp_f64(x, [](int v) {
        int r = __builtin_amdgcn_mov_dpp(v, 0x104, 0xf, 0x5, false);         // row_shl:4 into banks 0, 2 (lanes with bit 2 clear)
        return __builtin_amdgcn_update_dpp(r, v, 0x114, 0xf, 0xa, false);    // row_shr:4 into banks 1, 3
    });
}
__device__ __forceinline__ double xor2(double x) { return dpp_f64(x, [](int v) { return __builtin_amdgcn_mov_dpp(v, 0x4e, 0xf, 0xf, false); }); }    // quad_perm [2,3,0,1]
__device__ __forceinline__ double xor1(double x) { return dpp_f64(x, [](int v) { return __builtin_amdgcn_mov_dpp(v, 0xb1, 0xf, 0xf, false); }); }    // quad_perm [1,0,3,2]

// a: lanes with the distance bit clear keep a (and receive the partner's a); b: lanes with the bit set keep b.
// Returns a_own + a_partner in the "clear" lanes and b_partner + b_own in the "set" lanes: one tree level of TWO
// columns for the price of one (v_permlane32_swap / v_permlane16_swap exchange half-waves / odd-even rows in place).
// The swaps work IN PLACE on their two registers: as inline asm with read-write operands they need no copies (the builtin
// returns a pair and the compiler copies both inputs first: two moves per swap, fifty-six per tree).  gfx950 wants two wait
// states between a VALU write of either operand and the swap that reads it; the compiler inserts them for the builtin but
// cannot see inside an asm string, so `s_nop 1` stands on both sides of the swap INSIDE the string (cdna_hip_programming.md T21: the
// documented hazard is the one before the swap; the one behind it is what the compiler's own code shows).  Without it the low
// words came back stale, every sum of every engine was off by ~1e-8 relative, and only tools/tree_check.hip (now a test)
// noticed -- because every engine was off alike.
__device__ __forceinline__ double level32(double a, double b) {
    unsigned alo = (unsigned)__double2loint(a), ahi = (unsigned)__double2hiint(a), blo = (unsigned)__double2loint(b), bhi = (unsigned)__double2hiint(b);
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(alo), "+v"(blo));
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(ahi), "+v"(bhi));
    return __hiloint2double((int)ahi, (int)alo) + __hiloint2double((int)bhi, (int)blo);
}
__device__ __forceinline__ double level16(double a, double b) {
    unsigned alo = (unsigned)__double2loint(a), ahi = (unsigned)__double2hiint(a), blo = (unsigned)__double2loint(b), bhi = (unsigned)__double2hiint(b);
    asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1\n\ts_nop 1" : "+v"(alo), "+v"(blo));
    asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1\n\ts_nop 1" : "+v"(ahi), "+v"(bhi));
    return __hiloint2double((int)ahi, (int)alo) + __hiloint2double((int)bhi, (int)blo);
}
__device__ __forceinline__ double tree_low4(double x) {   // levels 8, 4, 2, 1: every lane of a 16-lane row ends with the row total
    x += xor8(x); x += xor4(x); x += xor2(x); x += xor1(x);
    return x;
}

// Wave totals of 16 columns: afterwards lane 16 * q (q = 0..3) holds columns 4q .. 4q+3 in v[0..3].
__device__ __forceinline__ void wave_tree16(double (&v)[16]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = level32(v[j], v[j + 8]);     // lanes < 32: columns 0-7, lanes >= 32: columns 8-15
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = level16(v[j], v[j + 4]);     // bit 4 clear: first four of those, set: the other four
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = tree_low4(v[j]);
}
// Wave totals of 2 columns: lane 0 holds a, lane 32 holds b (same tree per column as above).
__device__ __forceinline__ double wave_tree2(double a, double b) {
    double x = level32(a, b);
    x = level16(x, x);
    return tree_low4(x);
}

// correspondence sums of one (source, matched target) pair; see KSS_NSUMS in include/kssicp.h
__device__ __forceinline__ void accumulate_corr(double (&acc)[NSUMS], float px, float py, float pz,
                                                float qx, float qy, float qz, float d2f, double max_d2) {
    const double d2 = (double)d2f;
    acc[17] += d2;
    acc[18] += sqrt(d2);
    if (!(d2 > max_d2)) {   // PCL: `if (distance[0] > max_dist_sqr) continue;`
        const double p[3] = {(double)px, (double)py, (double)pz};
        const double q[3] = {(double)qx, (double)qy, (double)qz};
        acc[0] += 1.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) { acc[1 + k] += p[k]; acc[4 + k] += q[k]; }
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int l = 0; l < 3; ++l) acc[7 + 3 * k + l] += p[k] * q[l];
        acc[16] += d2;
    }
}


}  // namespace kss
