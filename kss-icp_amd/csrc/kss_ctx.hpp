// kss_ctx.hpp -- the context behind the opaque kss_ctx of include/kssicp.h, and the small helpers every host-side
// translation unit of libkssicp.so uses (error reporting, grow-only device buffers, pinned staging, HIP-event timing).
// Internal to the library.
#pragma once
#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "kss_internal.hpp"
#include "kss_host_pool.hpp"

using namespace kss;

// ---------------------------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------------------------
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
};
struct BarBuf : DevBuf { bool failed = false; };   // fine-grained device memory the host stores into (bar_ensure)

// A voxel map (kss_vmap_create): its own device arrays, never part of a context's grow-only workspace, so no other call on the
// context can move or overwrite them.  The context lists its live maps: an entry point takes a handle only when it is on the
// list of the context it is called on, and kss_ctx_destroy frees what is still listed.
struct kss_vmap {
    kss_ctx* ctx = nullptr;
    VmapBuilt b;
    double leaf = 0.0;
    int nb = 1;   // the neighbourhood every lookup of this map uses (kss_vmap_set_neighbourhood): 1, 7 or 27; a header field, host side
    VmapDev dev() const { return VmapDev{b.cell, b.rec, {b.lo[0], b.lo[1], b.lo[2]}, b.inv, {b.dims[0], b.dims[1], b.dims[2]},
                                        {b.base[0], b.base[1], b.base[2]}}; }
};

struct kss_ctx {
    int device = 0;
    int cu_count = 0;                   // compute units of the device (0: not asked yet)
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::string err;
    int nn_mode = KSS_NN_AUTO;
    double grid_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    double last_setup_ms = 0, last_loop_ms = 0;
    double t_launch_us = 0, t_wait_us = 0, t_host_us = 0;   // KSS_TIMING breakdown of the fused single-pair loop
    bool timing = false;
    bool tables_staged = false;
    int64_t stats_ns = -1, stats_nt = -1;

    // grow-only device workspace
    DevBuf tgt4, src0, cur[2], keys, partials, sums, nn_work, red_work, pair_red, state, cs, scratch_a,
        scratch_b, scratch_c, stage_src, stage_tgt, stage_idx, stage_d2, stage_out, g_counts, g_slot, g_start, g_cursor,
        g_bsums, g_sorted, g_list, g_count, g_bbox, g_partials, g_start2, g_pairs, g_stamps, g_pos, g_nnst, res_pos, res_wc, res_perm, pack_seg, reg_s, reg_t, reg_p, reg_all, reg_f, reg_g, oct_pts, oct_cen, oct_a, oct_b, oct_tmp, pre_partials, pre_state, g_rowpair, g_gate;
    // point-to-plane ICP (kss_pair.hip): per-pass idx / d2, source slot of each original index, partial rows, float normals
    // (staged or computed) and their f64 form from the normals kernel
    DevBuf p2l_idx, p2l_d2, p2l_perm, p2l_rows, p2l_nrm, p2l_n64;
    // trimmed ICP (kss_trim.hip): the selection's histogram rows (one per workgroup, rewritten by every digit) and its
    // TRIM_NSTATE TrimState records; neither has to hold anything between passes
    DevBuf trim_rows, trim_state;
    // robust ICP (kss_pair.hip): the keys its median is selected over where they are not the NN pass's d2
    DevBuf rob_keys;
    // generalized ICP (kss_pair.hip): the source's float normals (staged or computed)
    DevBuf gicp_snrm;
    // the same for many pairs per call (kss_pairb.hip): per-pair descriptors, row -> pair table, packed normals computed at setup
    DevBuf pb_desc, pb_rowpair, pb_nrm;
    // robust ICP for many pairs: one RobustScale per pair, uploaded once per call
    DevBuf pb_rscale;
    // generalized and symmetric ICP for many pairs: the packed source normals (staged or computed), and the
    // per-pair PairPass table: the host writes the pinned copy after every host step, one copy per pass takes it to the device table
    DevBuf pb_snrm, pb_gicp;
    // one-to-one rejection (kss_o2o.hip): the claim table (one uint64 per target of the call, two uint32 counters per
    // pair behind it; set to all ones before every pass, so nothing has to hold between passes) and the filtered idx / d2
    DevBuf o2o_table, o2o_idx, o2o_d2;
    // reciprocal rejection, one pair or many (kss_recip.hip): its workspace is o2o_table's buffer (the claim table
    // over the call's targets, four counters per pair, every pair's cell counts; set to all ones before every pass) and the filtered
    // idx / d2 are o2o_idx / o2o_d2; recip_sorted: the call's sources in cell order, rewritten by every pass; recip_box: the per-pair
    // box partials of the call's targets; the per-pair {grid, first cell} table derived from them: the host copy (kept here so that
    // its upload needs no synchronisation of its own), the device copy and the call's cell total.  A single pair is entry 0.
    DevBuf recip_sorted, recip_box, recip_grids;
    std::vector<RecipPairDev> h_recip_grids;
    int64_t recip_total_cells = 0;
    void* h_gicp = nullptr; size_t h_gicp_cap = 0;
    void* h_gicp_dev = nullptr;   // (the pinned copy as the device sees it: KSS_GICP_TABLE_MAPPED, an A/B switch)
    const PairState* last_state_dev = nullptr;   // the per-pair state table the last batched NN pass read (null: none, a single pair)
    HostPool pool;   // per-pair host work of batched iterations
    std::vector<kss_vmap*> vmaps;   // the live voxel maps created on this context (kss_vmap_create .. kss_vmap_destroy)
    std::vector<kss_ctx*> workers;   // contexts of kss_register_batch's worker threads (same device, own streams)
    std::vector<unsigned long long> last_stamps;
    int stamps_nblk = 0; unsigned long long stamps_seq = 0;   // KSS_GRID_STAMPS=2
    std::vector<float> h_bbox;   // bbox partials of the last single-pair target (host copy)
    unsigned int* h_box = nullptr; unsigned int* h_box_dev = nullptr; size_t h_box_bytes = 0;   // host-mapped: the same partials as checked granules, written by the pack kernel
    unsigned box_tag = 0; int box_rows = 0;   // tag and row count of the partials the last pack launch publishes there (0: none)
    double evals_sum = 0.0, evals_launches = 0.0;   // diagnostic runs: distance evaluations of the fused grid launches
    // pinned host staging
    void* h_sums = nullptr;  size_t h_sums_cap = 0;   // host-mapped: kernels write it through h_sums_dev
    void* h_sums_dev = nullptr;
    void* h_p2l = nullptr; size_t h_p2l_cap = 0;     // host-mapped: the KSS_P2L_NSUMS record, written through h_p2l_dev
    void* h_p2l_dev = nullptr;
    unsigned long long* h_seq = nullptr;       // host-mapped result of the fused grid kernel: NSUMS x {bits(sum), sequence number}
    unsigned long long* h_seq_dev = nullptr;
    size_t h_seq_bytes = 0;
    // gated launches (kss_engine.hip): the next iteration's fused kernel is enqueued while the current one runs and polls
    // the host-mapped record h_xf[slot]; the host answers it with the transform and the launch's stamp
    struct Gated {
        int supported = -1;                 // -1 unknown, 0 no, 1 yes
        bool want_next = false;             // set by the ICP loop: another regular iteration may follow this pass
        bool pending = false;               // a pre-enqueued launch is waiting at its gate ...
        bool chain = false;                 // ... it is a chained launch (more than one pass) ...
        int steps_left = 0;                 // ... with this many passes still to be released (a chained launch runs several)
        int max_steps = 1;                  // set by the ICP loop: regular iterations that may still follow this pass
        int slot = 0;
        unsigned long long seq = 0;
        int32_t stamp = 0;
        const void* d_in = nullptr; void* d_out = nullptr;
        bool fma = false, full = false, want_full = false; double max_d2 = 0.0;
    } gated;
    // g_count and g_counts are ZERO AT REST: every kernel that uses them leaves them zeroed (the unresolved-list length is
    // reset when the list is consumed; the cell counts are zeroed by the scan that reads them -- a single pair, whose scatter
    // takes its slots from g_slot -- or counted back down by the scatter -- a batch), so a registration needs no memset of
    // its own.  A call that fails midway sets ws_dirty and the next one clears them first; ensure_zeroed() clears
    // a buffer it had to (re)allocate.
    bool ws_dirty = false;
    bool defer_wait = false;   // batched fused pass: the ICP loop polls the pairs' result slots itself
    PairState* h_xf = nullptr; PairState* h_xf_dev = nullptr;
    bool fit_last = false;            // the fitness pass: PairState::pad[0] names the buffer of each pair's last pass
    bool nn_have = false;             // the cell-list pass has written nn_win / nn_state for the current lists
    // the single pair's two gate records, 128 bytes apart; the pair-resident engines' 128-byte record per pair; the batched pass's per-pair states
    BarBuf gate_bar, res_gate, bar_state;
    int large_bar = -1;                 // the device property, asked once per context (-1: not yet)
    unsigned res_launches = 0;          // the pair-resident engines' launches so far (every launch has its own range of gate stamps)
    double res_passes = 0.0;            // ... (pair, pass) units its profiled launches ran
    int cand_cap = 0, cand_cap_pad = -1, cand_cap_fma = -1;   // candidate-resident kernel: workgroups resident at once for this target size
    // kss_register runs the judge ICP and the candidate ICPs as ONE speculative batch: pair spec_judge is the judge; once its
    // fitness is known and does not exceed spec_threshold the candidates are told to stop (their results are not used).
    // spec_ran: the batch ran that way (otherwise the caller takes the sequential route); spec_cancelled: candidates were stopped
    int spec_judge = -1; double spec_threshold = 0.0; bool spec_ran = false, spec_cancelled = false;
    // a resident launch that had to be given up (a workgroup nobody answered in time: another process on the GPU, a starved host)
    // keeps its engine off for this context for a while: the next calls go straight to the launch-per-pass form
    std::chrono::steady_clock::time_point res_backoff[2] = {};
    unsigned long long seq = 0;
    void* h_state = nullptr; size_t h_state_cap = 0;

    // profiling
    int prof = 0;                       // 0 = off, n = event-time every n-th launch of each kernel class
    unsigned prof_tick[KSS_K_COUNT] = {};
    struct EvPair { hipEvent_t a, b; };
    std::vector<EvPair> ev[KSS_K_COUNT];
    std::vector<EvPair> ev_pool;   // recycled event pairs: no hipEventCreate/Destroy inside timed loops
    double prof_ms[KSS_K_COUNT] = {0};
    int64_t prof_n[KSS_K_COUNT] = {0};
};

static inline int set_err(kss_ctx* c, int code, const char* what, hipError_t e = hipSuccess) {
    if (c) {
        c->err = what;
        if (e != hipSuccess) { c->err += ": "; c->err += hipGetErrorString(e); }
    }
    return code;
}

#define HIPCHK(ctx, call)                                                        \
    do {                                                                         \
        hipError_t e_ = (call);                                                  \
        if (e_ != hipSuccess) return set_err((ctx), KSS_ERR_HIP, #call, e_);     \
    } while (0)

static inline int ensure(kss_ctx* c, DevBuf& b, size_t bytes) {
    if (bytes <= b.cap) return KSS_OK;
    if (b.p) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipFree(b.p));
        b.p = nullptr; b.cap = 0;
    }
    size_t want = bytes + bytes / 8 + 256;
    hipError_t e = hipMalloc(&b.p, want);
    if (e != hipSuccess) { b.p = nullptr; return set_err(c, KSS_ERR_NOMEM, "hipMalloc", e); }
    b.cap = want;
    return KSS_OK;
}

static inline int ensure_zeroed(kss_ctx* c, DevBuf& b, size_t bytes) {
    const size_t before = b.cap;   // (not the pointer: a freed block can come back at the same address with a larger size)
    const int rc = ensure(c, b, bytes);
    if (rc != KSS_OK) return rc;
    if (b.cap != before && hipMemsetAsync(b.p, 0, b.cap, c->stream) != hipSuccess) return set_err(c, KSS_ERR_HIP, "hipMemsetAsync(zero-at-rest buffer)");
    return KSS_OK;
}

// At least `bytes` of fine-grained device memory the host can store into directly; null without a large BAR, with KSS_GATE_BAR=0,
// or after a failure (latched: the caller's other form runs from then on).  Growing waits for the stream first (nothing may still
// read the old block); a new block is zeroed, and a device-wide synchronise puts the zeroes there before the host's first store
// (on allocation only).  bar_state needs no zeroes -- mirror_state stores every entry before a kernel reads it -- and gets them too.
inline void* bar_ensure(kss_ctx* c, BarBuf& b, size_t bytes) {
    static const bool want_bar = getenv("KSS_GATE_BAR") == nullptr || atoi(getenv("KSS_GATE_BAR")) != 0;
    if (!want_bar || b.failed) return nullptr;
    if (b.p && b.cap >= bytes) return b.p;
    hipDeviceProp_t prop;
    if (c->large_bar < 0) c->large_bar = hipGetDeviceProperties(&prop, c->device) == hipSuccess && prop.isLargeBar ? 1 : 0;
    if (b.p) { hipStreamSynchronize(c->stream); hipFree(b.p); b.p = nullptr; b.cap = 0; }
    const size_t cap = (bytes + bytes / 4 + 4095) / 4096 * 4096;
    void* p = nullptr;
    if (!c->large_bar || hipExtMallocWithFlags(&p, cap, hipDeviceMallocFinegrained) != hipSuccess || !p || hipMemset(p, 0, cap) != hipSuccess ||
        hipDeviceSynchronize() != hipSuccess) {
        (void)hipGetLastError();
        if (p) hipFree(p);
        b.failed = true;
        return nullptr;
    }
    b.p = p; b.cap = cap;
    return p;
}

static inline int ensure_pinned(kss_ctx* c, void*& p, size_t& cap, size_t bytes) {
    if (bytes <= cap) return KSS_OK;
    if (p) { HIPCHK(c, hipStreamSynchronize(c->stream)); HIPCHK(c, hipHostFree(p)); p = nullptr; cap = 0; }
    size_t want = bytes * 2 + 256;
    hipError_t e = hipHostMalloc(&p, want, hipHostMallocMapped);
    if (e != hipSuccess) { p = nullptr; return set_err(c, KSS_ERR_NOMEM, "hipHostMalloc", e); }
    cap = want;
    if (&p == &c->h_sums) {
        void* d = nullptr;
        HIPCHK(c, hipHostGetDevicePointer(&d, p, 0));
        c->h_sums_dev = d;
    }
    if (&p == &c->h_p2l) {
        void* d = nullptr;
        HIPCHK(c, hipHostGetDevicePointer(&d, p, 0));
        c->h_p2l_dev = d;
    }
    return KSS_OK;
}

#define KCHK(expr)                     \
    do {                               \
        int rc_ = (expr);              \
        if (rc_ != KSS_OK) return rc_; \
    } while (0)

struct ProfScope {   // records a start/stop event pair around a launch when profiling is on
    kss_ctx* c; int k; kss_ctx::EvPair ep; bool on;
    // every: bracket this launch whenever profiling is on (a chained launch runs tens of passes: its two events are cheap)
    ProfScope(kss_ctx* c_, int k_, bool every = false) : c(c_), k(k_), on(c_->prof > 0) {
        if (on && c->prof > 1 && !every) on = (c->prof_tick[k]++ % (unsigned)c->prof) == 0;   // sampled: the events themselves cost ~3 us
        if (!on) return;
        if (!c->ev_pool.empty()) {
            ep = c->ev_pool.back();
            c->ev_pool.pop_back();
        } else if (hipEventCreate(&ep.a) != hipSuccess || hipEventCreate(&ep.b) != hipSuccess) {
            on = false;
            return;
        }
        hipEventRecord(ep.a, c->stream);
    }
    ~ProfScope() {
        if (!on) return;
        hipEventRecord(ep.b, c->stream);
        c->ev[k].push_back(ep);
    }
};

static inline void prof_collect(kss_ctx* c) {
    for (int k = 0; k < KSS_K_COUNT; ++k) {
        for (auto& ep : c->ev[k]) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, ep.a, ep.b) == hipSuccess) {
                c->prof_ms[k] += ms; c->prof_n[k] += 1;
                if (k == KSS_K_GRID_CHAIN) c->prof_ms[KSS_K_GRID_CHAIN_PASS] += ms;   // (its count: the passes released, kss_engine.hip)
                if (k == KSS_K_RESIDENT) c->prof_ms[KSS_K_RESIDENT_PASS] += ms;       // (its count: the (pair, pass) units run)
            }
            c->ev_pool.push_back(ep);
        }
        c->ev[k].clear();
    }
}


// live contexts of this process (gated launches are used only while there is exactly one: see kss_engine.hip)
inline std::atomic<int>& kss_live_contexts() { static std::atomic<int> n{0}; return n; }

// host -> device staging of a packed cloud
static inline int upload(kss_ctx* c, DevBuf& b, const void* h, size_t bytes) {
    KCHK(ensure(c, b, bytes));
    HIPCHK(c, hipMemcpyAsync(b.p, h, bytes, hipMemcpyHostToDevice, c->stream));
    return KSS_OK;
}

// ---- the registration engine (kss_engine.hip) ---------------------------------------------------------------
namespace kss {
// packs the clouds of npairs pairs (device pointers, point offsets), builds the search structures and runs the ICP loop
int icp_run_dev(kss_ctx* c, const void* d_src, const int64_t* src_off, const void* d_tgt, const int64_t* tgt_off,
                int npairs, bool shared_target, int dtype, const kss_icp_params* p, kss_icp_result* results);
// one exact NN pass of a single pair (+ the correspondence sums when sums_out is given)
int nn_generic_dev(kss_ctx* c, const void* d_src, int64_t ns, const void* d_tgt, int64_t nt, int dtype,
                   int32_t* d_idx, float* d_d2, double sums_out[NSUMS]);
// ICP of one pair by kss_icp_p2l (plane, untrimmed), kss_icp_trimmed, kss_icp_robust (either metric), kss_icp_gicp, kss_icp_symm or kss_icp_sim:
// float clouds on the device, d_nrm the target's normals for the plane metric.  The untrimmed, unweighted point metric is icp_run_dev's.
struct PairMode {
    bool plane = false;             // point-to-plane step (d_nrm given); otherwise point-to-point
    bool trimmed = false;           // keep the closest `overlap` share of each pass's candidates
    double overlap = 1.0;
    double* trace_info = nullptr;   // trimmed / robust: KSS_TRIM_NINFO = KSS_ROBUST_NINFO doubles per traced pass
    double* last_info = nullptr;    // trimmed / robust: the same of the last pass
    bool robust = false;            // M-estimator weights (kss_icp_robust; not together with trimmed), scale and loss in rs
    RobustScale rs;
    bool gicp = false;              // generalized ICP (kss_icp_gicp; with plane, not with trimmed or robust): d_nrm and the SOURCE's
    double gicp_epsilon = 0.0;      // normals d_src_nrm (device, float triples by original source index) weigh every correspondence
    const float* d_src_nrm = nullptr;
    bool symm = false;              // symmetric ICP (kss_icp_symm; with plane, not with trimmed or gicp): the plane record on
    int symm_align = 1;             // nq +- R_F ns, ns from d_src_nrm as for gicp; the step is rigid_from_symm_sums.  With robust
                                    // (kss_icp_symm_robust, kss_icp_symm_robust_batch): the weights of rs on that record
    bool sim = false;               // similarity ICP (kss_icp_sim; with trimmed and the point metric only): the step is sim_from_sums
    double scale_min = 1.0;         // with the accumulated scale kept in [scale_min, scale_max]; trace_info / last_info / info_all
    double scale_max = 1.0;         // hold KSS_SIM_NINFO doubles per record
    bool unique = false;            // one-to-one rejection in front of the trimmed pass (kss_icp_o2o; with trimmed, not with robust, gicp,
                                    // symm or sim): the info records hold KSS_O2O_NINFO doubles, [0] = u, [4] = m
    bool mutual = false;            // reciprocal rejection in front of the trimmed pass (kss_icp_recip; with trimmed, never with unique,
                                    // robust, gicp, symm or sim; one pair or a batch): KSS_RECIP_NINFO doubles, [0] = r, [4] = m, [5] = u
};
static_assert(KSS_ROBUST_NINFO == KSS_TRIM_NINFO, "the pair loop carries both info records in the same four slots");
int pair_run_dev(kss_ctx* c, const float* d_src, int64_t ns, const float* d_tgt, int64_t nt, const float* d_nrm,
                 const kss_icp_params* p, const PairMode& mode, kss_icp_result* res);
// one pass of that loop over given correspondences d_idx (the *_sums_dev entry points): the launches of the mode (sim alone: the
// untrimmed similarity record) into sums and, robust, info; Rn: the row-major 3 x 3 the source normals turn with (null: identity)
int pair_record_dev(kss_ctx* c, const float* d_src, const float* d_tgt, const float* d_nrm, const int32_t* d_idx, int64_t n, int64_t nt,
                    double max_d2, const PairMode& mode, const float* Rn, double* sums, double* info);
int trim_threshold_dev(kss_ctx* c, const float* d_d2, int64_t n, double max_d2, double overlap, double* info);
// voxelized generalized ICP (kss_vgicp_sums_dev, kss_icp_vgicp_dev; the entry points check their arguments): n packed float triples
// d_src with the normals d_snrm against the map.  One record: rows + final launch, Rn as for pair_record_dev.  The loop:
// kss_icp_gicp's host step on a pass of two launches and no NN pass; info: KSS_VGICP_NINFO doubles or null.
int vgicp_record_dev(kss_ctx* c, const float* d_src, const float* d_snrm, int64_t n, const kss_vmap* map, double max_d2, const float* Rn,
                     double epsilon, double* sums);
// T0: the HOST float 4 x 4 the accumulated pose starts at (kss_icp_vgicp_from), null: the identity, kss_icp_vgicp's loop as it was.
int vgicp_run_dev(kss_ctx* c, const float* d_src, int64_t ns, const float* d_snrm, const kss_vmap* map, const float* T0, const kss_icp_params* p,
                  double epsilon, kss_icp_result* res, double* info);
// the ladder (kss_icp_vgicp_c2f): level l is vgicp_run_dev on maps[l] from level l - 1's pose; info: nlevels * KSS_VGICP_NINFO or null
int vgicp_c2f_run_dev(kss_ctx* c, const float* d_src, int64_t ns, const float* d_snrm, const kss_vmap* const* maps, int nlevels, const float* T0,
                      const kss_icp_params* p, double epsilon, kss_icp_result* results, double* info);
// nscans >= 1 scans against one map in lockstep (kss_icp_vgicp_batch_dev; the entry points check their arguments): d_src / d_snrm
// packed, src_off nscans + 1 offsets in points from 0, epsilons one per scan; info_all: nscans * KSS_VGICP_NINFO doubles or null
int vgicpb_run_dev(kss_ctx* c, const float* d_src, const int64_t* src_off, const float* d_snrm, int nscans, const kss_vmap* map,
                   const kss_icp_params* p, const double* epsilons, kss_icp_result* results, double* info_all);
// npairs >= 1 pairs in lockstep (kss_icp_p2l_batch, kss_icp_trimmed_batch, kss_icp_robust_batch, kss_icp_gicp_batch,
// kss_icp_symm_batch, kss_icp_symm_robust_batch -- symm with robust takes both symm_aligns and rscales): d_nrm laid
// out like d_tgt; overlaps: one per pair (trimmed; M.overlap is not read); rscales: one per pair (robust; M.rs is not read), all
// with the loss of the batch; info_all: npairs * KSS_TRIM_NINFO (M.sim: KSS_SIM_NINFO) or null; M.trace_info / M.last_info: pair 0's / unused;
// gicp_eps: one epsilon per pair (generalized; M.gicp_epsilon is not read), M.d_src_nrm laid out like d_src;
// symm_aligns: one align_normals per pair (symmetric; M.symm_align is not read), M.d_src_nrm as for generalized
int pairs_run_dev(kss_ctx* c, const float* d_src, const int64_t* src_off, const float* d_tgt, const int64_t* tgt_off, const float* d_nrm,
                  int npairs, const kss_icp_params* p, const PairMode& mode, const double* overlaps, kss_icp_result* results, double* info_all,
                  const RobustScale* rscales = nullptr, const double* gicp_eps = nullptr, const int32_t* symm_aligns = nullptr);
// the selection alone for nseg segments of d_d2 in one launch
int trim_threshold_batch_dev(kss_ctx* c, const float* d_d2, const int64_t* off, int nseg, double max_d2, const double* overlaps, double* info_all);
// the one-to-one filter alone (kss_o2o_filter[_batch]_dev) for nseg segments [off[i], off[i + 1]) of d_idx / d_d2, segment i
// against nts[i] targets, in the same three launches: the filtered arrays (either may be null or its input) and {m, u} per segment
int o2o_filter_dev(kss_ctx* c, const int32_t* d_idx, const float* d_d2, const int64_t* off, const int64_t* nts, int nseg, double max_d2,
                   int32_t* d_idx_out, float* d_d2_out, double* info_all);
// the reciprocal filter alone (kss_recip_filter[_batch]_dev): for nseg >= 1 segments, sources [off[i], off[i + 1]) of the packed float
// triples d_src with the map d_idx / d_d2 against targets [tgt_off[i], tgt_off[i + 1]) of d_tgt, both offset arrays from 0, reverse
// distances by dist2<nn_fma>; the filtered arrays (either may be null or its input) and info_all = {m, u, r} per segment.
// lone: the single-pair entry's one segment (no row -> pair table, the box partials cut by the single pair's rule)
int recip_filter_dev(kss_ctx* c, const float* d_src, const int64_t* off, const float* d_tgt, const int64_t* tgt_off, int nseg,
                     const int32_t* d_idx, const float* d_d2, double max_d2, bool nn_fma, int32_t* d_idx_out, float* d_d2_out,
                     double* info_all, bool lone = false);
// host-mapped {value, sequence number} result slots: allocate them; wait for the first nslots of launch c->seq
int ensure_pub_slots(kss_ctx* c);
int wait_slots(kss_ctx* c, int nslots, double* out);
}  // namespace kss
