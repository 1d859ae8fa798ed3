// kss_handover.hpp -- the hand-over between host and device of every engine that runs more than one ICP pass per launch,
// stated once: writer next to reader, host next to device.  Three formats, each a 16-byte granule that is
// written by ONE aligned 16-byte store and carries a check word of its other three words, so that no flag has to be ordered
// behind the data and a granule seen torn -- or stale -- fails its check and is simply read again:
//   gate record   host -> device, fine-grained device memory through the BAR: 15 words as five granules
//                 {w[3g], w[3g + 1], w[3g + 2], stamp + kss_mix3(those three)}.   gate_record_store -> gate_record_take / _stopped
//   result slot   device -> host, host-mapped: {bits of an f64, low word of seq | check << 32}.   pub_put (kss_device.hpp) -> slots_collect
//   exit flag     device -> host, host-mapped, one per pair: {tag | pair << 32, note | check << 32}.   res_store_exit_flag -> exit_flag_read
// The host parts need neither a device nor a context (tools/handover_host_check.hip).  Not here: grid_pass_kernel's own poll
// (kss_grid.hip), the host-mapped h_xf record of that gate without a large BAR, and the row hand-over (kss_device.hpp).
#pragma once
#include <hip/hip_runtime.h>
#include <emmintrin.h>
#include <chrono>
#include <cstring>

namespace kss {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// the 32-bit check word of a granule's three data words
__host__ __device__ inline unsigned kss_mix3(unsigned a, unsigned b, unsigned c) {
    unsigned h = (a + 0x9E3779B1u) * 0x85EBCA77u;
    h ^= h >> 15;
    h = (h ^ (b + 0x7F4A7C15u)) * 0xC2B2AE3Du;
    h ^= h >> 13;
    h = (h ^ (c + 0x165667B1u)) * 0x27D4EB2Fu;
    h ^= h >> 16;
    return h;
}

// ---- gate records -----------------------------------------------------------------------------------------------------
// Words 0 .. 11 are the transform; 12 .. 14: {active, apply, skip} (the single pair's PairState) or {1, apply, mode} (resident
// engines).  Resident stamps: every launch owns 4096; stamp0 + k opens pass k (k <= 4002), stamp0 + RES_STAMP_ANY is accepted at
// ANY pass -- the host's order to stop, which may overwrite a record some workgroups have not read yet.
constexpr unsigned RES_STAMP_ANY = 4095u;
constexpr int GATE_TORN_GRANULE = 1;   // the granule the test hooks alter: transform words in both layouts

// the five stores (their order does not matter) and the fence that pushes them out of the write-combining buffers; slot: 16-byte
// aligned, 20 words.  altered: granule GATE_TORN_GRANULE with a word that does not fit its check, as a torn store would look
__attribute__((always_inline)) inline void gate_record_write(unsigned* slot, const unsigned w[15], unsigned stamp, bool altered) {
    for (int g = 0; g < 5; ++g) {
        const unsigned tag = stamp + kss_mix3(w[3 * g], w[3 * g + 1], w[3 * g + 2]);   // stamp + check of the granule's three words
        const unsigned w1 = altered && g == GATE_TORN_GRANULE ? w[3 * g + 1] ^ 0x00010000u : w[3 * g + 1];
        _mm_store_si128((__m128i*)(slot + 4 * g), _mm_set_epi32((int)tag, (int)w[3 * g + 2], (int)w1, (int)w[3 * g]));
    }
    _mm_sfence();
}
// torn_first (test hooks; which record is the n-th is the caller's count): first the altered record, 200 us later the right one
__attribute__((always_inline)) inline void gate_record_store(unsigned* slot, const unsigned w[15], unsigned stamp, bool torn_first) {
    if (torn_first) {
        gate_record_write(slot, w, stamp, true);
        const auto t0 = std::chrono::steady_clock::now();
        while (std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() < 200.0) __builtin_ia32_pause();
    }
    gate_record_write(slot, w, stamp, false);
}

// The poll of the resident kernels, called by lanes tid < 8 of the workgroup (one wave): lane min(tid, 4) reads granule
// min(tid, 4) until all five carry `expect` or all five carry `any`, at most `polls` times; then the 15 words are in lds15.
// False: nobody answered in time.  (polls by reference and tid from the caller: the bound is read where the kernels' own text
// read it, the lane number is the value the kernel holds; otherwise the kernels come out an instruction longer)
__device__ __forceinline__ bool gate_record_take(const unsigned* rec, unsigned expect, unsigned any, const int& polls, int* lds15, int tid) {
    const unsigned int* src = rec + 4 * min(tid, 4);
    u32x4 v;
    int n = 0;
    bool ok = true;
    for (;;) {
        asm volatile("global_load_dwordx4 %0, %1, off sc0 sc1\n\ts_waitcnt vmcnt(0)" : "=&v"(v) : "v"(src) : "memory");   // system scope: the writer is the host
        const unsigned tag = v.w - kss_mix3(v.x, v.y, v.z);
        if (__builtin_amdgcn_ballot_w64(tag == expect) == 0xffull) break;
        if (__builtin_amdgcn_ballot_w64(tag == any) == 0xffull) break;   // "whatever pass you wait for": a stop order
        __builtin_amdgcn_s_sleep(2);
        if (++n > polls) { ok = false; break; }
    }
    if (tid < 5) { lds15[3 * tid] = (int)v.x; lds15[3 * tid + 1] = (int)v.y; lds15[3 * tid + 2] = (int)v.z; }
    return ok;
}
// one look at a record's first granule: does it carry the order to stop?  (A waiting lane of the candidate kernel's row total.)
__device__ __forceinline__ bool gate_record_stopped(const unsigned* rec, unsigned any) {
    u32x4 g;
    asm volatile("global_load_dwordx4 %0, %1, off sc0 sc1\n\ts_waitcnt vmcnt(0)" : "=&v"(g) : "v"(rec) : "memory");
    return g.w - kss_mix3(g.x, g.y, g.z) == any;
}

// ---- result slots -------------------------------------------------------------------------------------------------------
// the first n slots under number `want` as doubles, if they have all landed (two 8-byte loads a slot; the highest usually lands last)
inline bool slots_collect(const unsigned long long* sl, int n, unsigned long long want, double* out) {
    for (int k = n - 1; k >= 0; --k) {
        const unsigned long long w = __atomic_load_n(&sl[2 * k + 1], __ATOMIC_ACQUIRE);
        if ((unsigned)w != (unsigned)want) return false;
        const unsigned long long bits = __atomic_load_n(&sl[2 * k], __ATOMIC_RELAXED);
        if ((unsigned)(w >> 32) != kss_mix3((unsigned)bits, (unsigned)(bits >> 32), (unsigned)w)) return false;
        std::memcpy(&out[k], &bits, sizeof(double));
    }
    return true;
}

// ---- exit flags ---------------------------------------------------------------------------------------------------------
// "this pair's workgroups have all left": the host learns that a resident kernel is gone from these flags, not from HIP (a
// HIP call of a serving thread can wait on locks other threads hold for as long as THEIR kernels run)
__device__ __forceinline__ void res_store_exit_flag(unsigned long long* flags, int pair, unsigned tag, unsigned note = 0u) {
    u32x4 o;
    o.x = tag; o.y = (unsigned)pair; o.z = note; o.w = kss_mix3(o.x, o.y, o.z);
    unsigned long long* dst = flags + 2 * (int64_t)pair;
    asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1" ::"v"(dst), "v"(o) : "memory");
}
// has pair `pair` stored its flag under `tag`?  note (optional): the flag's note word
inline bool exit_flag_read(const unsigned long long* flags, int pair, unsigned tag, unsigned* note) {
    const unsigned long long w0 = __atomic_load_n(&flags[2 * pair], __ATOMIC_ACQUIRE), w1 = __atomic_load_n(&flags[2 * pair + 1], __ATOMIC_RELAXED);
    if ((unsigned)w0 != tag || (unsigned)(w0 >> 32) != (unsigned)pair || (unsigned)(w1 >> 32) != kss_mix3((unsigned)w0, (unsigned)(w0 >> 32), (unsigned)w1)) return false;
    if (note) *note = (unsigned)w1;
    return true;
}

}  // namespace kss
