// kss_api.hip -- the C-ABI of include/kssicp.h: context and profiling entry points, and the compute entry points over
// the engine (kss_engine.hip) and the kernel launchers (kss_kernels / kss_grid / kss_aivs / kss_knn / kss_octree / kss_p2l / kss_trim / kss_robust / kss_pairb / kss_o2o / kss_recip / kss_vmap .hip).
// There is no CPU compute fallback anywhere in this file.
#pragma clang fp contract(off)

#include <cmath>
#include <functional>

#include "kss_ctx.hpp"
#include "kss_gicp.hpp"
#include "kss_robust.hpp"

extern "C" {

int kss_version(void) { return KSS_VERSION; }

const char* kss_status_string(int s) {
    switch (s) {
        case KSS_OK: return "ok";
        case KSS_ERR_ARG: return "invalid argument";
        case KSS_ERR_HIP: return "HIP runtime error";
        case KSS_ERR_NOMEM: return "out of memory";
        case KSS_ERR_NODEVICE: return "no usable GPU device";
        case KSS_ERR_CAPACITY: return "output buffer too small";
        case KSS_ERR_RCCL: return "RCCL error";
        case KSS_ERR_DEGENERATE: return "degenerate point-to-plane system";
        default: return "unknown status";
    }
}

const char* kss_last_error(const kss_ctx* ctx) { return ctx ? ctx->err.c_str() : ""; }

static int ctx_create_common(int device_id, void* stream, bool borrow, kss_ctx** out) {
    if (!out) return KSS_ERR_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return KSS_ERR_NODEVICE;
    if (device_id < 0 || device_id >= n) return KSS_ERR_ARG;
    if (hipSetDevice(device_id) != hipSuccess) return KSS_ERR_NODEVICE;
    kss_ctx* c = new (std::nothrow) kss_ctx();
    if (!c) return KSS_ERR_NOMEM;
    c->device = device_id;
    if (borrow) {
        c->stream = (hipStream_t)stream;
        c->own_stream = false;
    } else {
        if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; return KSS_ERR_HIP; }
        c->own_stream = true;
    }
    kss_live_contexts().fetch_add(1);
    // launch sequence numbers are unique per PROCESS, not per context: rows handed over as {bits, number} granules are taken
    // on the number alone, and a freed workspace block can come back to the next context with the old context's rows in it
    static std::atomic<unsigned long long> ctx_serial{0};
    c->seq = (ctx_serial.fetch_add(1) + 1ull) << 40;
    *out = c;
    return KSS_OK;
}

int kss_ctx_create(int device_id, kss_ctx** out) { return ctx_create_common(device_id, nullptr, false, out); }
int kss_ctx_create_on_stream(int device_id, void* hip_stream, kss_ctx** out) {
    return ctx_create_common(device_id, hip_stream, true, out);
}

int kss_ctx_destroy(kss_ctx* c) {
    if (!c) return KSS_ERR_ARG;
    hipSetDevice(c->device);
    hipStreamSynchronize(c->stream);
    prof_collect(c);
    for (auto& ep : c->ev_pool) { hipEventDestroy(ep.a); hipEventDestroy(ep.b); }
    c->ev_pool.clear();
    DevBuf* bufs[] = {&c->tgt4, &c->src0, &c->cur[0], &c->cur[1], &c->keys, &c->partials, &c->sums, &c->nn_work,
                      &c->red_work, &c->pair_red, &c->state, &c->cs, &c->scratch_a, &c->scratch_b, &c->scratch_c,
                      &c->stage_src, &c->stage_tgt, &c->stage_idx, &c->stage_d2, &c->stage_out, &c->g_counts, &c->g_slot, &c->g_start,
                      &c->g_cursor, &c->g_bsums, &c->g_sorted, &c->g_list, &c->g_count, &c->g_bbox, &c->g_partials, &c->g_start2, &c->g_pairs, &c->g_stamps, &c->g_pos, &c->g_nnst, &c->res_pos, &c->res_wc, &c->res_perm, &c->pack_seg, &c->reg_s, &c->reg_t, &c->reg_p, &c->reg_all, &c->reg_f, &c->reg_g, &c->oct_pts, &c->oct_cen, &c->oct_a, &c->oct_b, &c->oct_tmp, &c->pre_partials, &c->pre_state, &c->g_rowpair, &c->g_gate, &c->p2l_idx, &c->p2l_d2, &c->p2l_perm, &c->p2l_rows, &c->p2l_nrm, &c->p2l_n64, &c->trim_rows, &c->trim_state, &c->rob_keys, &c->gicp_snrm, &c->pb_desc, &c->pb_rowpair, &c->pb_nrm, &c->pb_rscale, &c->pb_snrm, &c->pb_gicp, &c->o2o_table, &c->o2o_idx, &c->o2o_d2, &c->recip_sorted, &c->recip_box, &c->recip_grids, &c->gate_bar, &c->res_gate, &c->bar_state};
    for (DevBuf* b : bufs)
        if (b->p) hipFree(b->p);
    if (c->h_sums) hipHostFree(c->h_sums);
    if (c->h_seq) hipHostFree(c->h_seq);
    if (c->h_p2l) hipHostFree(c->h_p2l);
    if (c->h_gicp) hipHostFree(c->h_gicp);
    if (c->h_box) hipHostFree(c->h_box);
    if (c->h_xf) hipHostFree(c->h_xf);
    if (c->h_state) hipHostFree(c->h_state);
    for (kss_vmap* m : c->vmaps) { vmap_free(m->b); delete m; }   // voxel maps still alive go with their context (include/kssicp.h)
    c->vmaps.clear();
    for (kss_ctx* w : c->workers) kss_ctx_destroy(w);
    c->workers.clear();
    if (c->own_stream) hipStreamDestroy(c->stream);
    kss_live_contexts().fetch_sub(1);
    delete c;
    return KSS_OK;
}

int kss_ctx_synchronize(kss_ctx* c) {
    if (!c) return KSS_ERR_ARG;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return KSS_OK;
}

void* kss_ctx_stream(kss_ctx* c) { return c ? (void*)c->stream : nullptr; }

int kss_ctx_set_nn_mode(kss_ctx* c, int nn_mode) {
    if (!c || nn_mode < KSS_NN_AUTO || nn_mode > KSS_NN_GRID) return KSS_ERR_ARG;
    c->nn_mode = nn_mode;
    return KSS_OK;
}

int kss_profile_enable(kss_ctx* c, int on) {
    if (!c) return KSS_ERR_ARG;
    c->prof = on > 0 ? on : 0;
    for (int k = 0; k < KSS_K_COUNT; ++k) c->prof_tick[k] = 0;
    if (c->prof) {   // pre-create the event pairs a timed region will use
        HIPCHK(c, hipSetDevice(c->device));
        while (c->ev_pool.size() < 4096) {
            kss_ctx::EvPair ep;
            if (hipEventCreate(&ep.a) != hipSuccess) break;
            if (hipEventCreate(&ep.b) != hipSuccess) { hipEventDestroy(ep.a); break; }
            c->ev_pool.push_back(ep);
        }
    }
    return KSS_OK;
}
int kss_grid_stats(kss_ctx* c, double out[8]) {
    if (!c || !out) return KSS_ERR_ARG;
    for (int k = 0; k < 8; ++k) out[k] = c->grid_stats[k];
    return KSS_OK;
}
// diagnostic: distance evaluations of the fused grid launches since the last call (KSS_GRID_STAMPS=1): {sum, launches}
int kss_debug_grid_evals(kss_ctx* c, double out[2]) {
    if (!c || !out) return KSS_ERR_ARG;
    out[0] = c->evals_sum; out[1] = c->evals_launches;
    c->evals_sum = 0.0; c->evals_launches = 0.0;
    return KSS_OK;
}

// diagnostic: in-kernel timeline stamps of the last fused grid launch (KSS_GRID_STAMPS=1); not part of the ABI header
int kss_debug_grid_stamps(kss_ctx* c, unsigned long long* out, int64_t cap) {
    if (!c || !out) return KSS_ERR_ARG;
    if (c->stamps_nblk > 0 && c->g_stamps.p) {   // KSS_GRID_STAMPS=2: the buffer of the last launch that was waited for
        hipStreamSynchronize(c->stream);
        c->last_stamps.resize((size_t)c->stamps_nblk * 16);
        if (hipMemcpy(c->last_stamps.data(), (const unsigned long long*)c->g_stamps.p + (size_t)(c->stamps_seq & 1) * c->stamps_nblk * 16,
                      c->last_stamps.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return KSS_ERR_HIP;
    }
    const int64_t n = std::min<int64_t>(cap, (int64_t)c->last_stamps.size());
    for (int64_t i = 0; i < n; ++i) out[i] = c->last_stamps[(size_t)i];
    return (int)n;
}
int kss_profile_reset(kss_ctx* c) {
    if (!c) return KSS_ERR_ARG;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    for (int k = 0; k < KSS_K_COUNT; ++k) { c->prof_ms[k] = 0; c->prof_n[k] = 0; }
    return KSS_OK;
}
int kss_profile_event_overhead(kss_ctx* c, double* ms) {
    if (!c || !ms) return KSS_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    hipEvent_t a = nullptr, b = nullptr;
    HIPCHK(c, hipEventCreate(&a));
    HIPCHK(c, hipEventCreate(&b));
    for (int i = 0; i < 16; ++i) launch_empty(c->stream);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    double tot = 0.0;
    const int reps = 200;
    for (int i = 0; i < reps; ++i) {   // idle queue -> event, launch, event: the pattern of one fused ICP iteration
        hipEventRecord(a, c->stream);
        launch_empty(c->stream);
        hipEventRecord(b, c->stream);
        HIPCHK(c, hipStreamSynchronize(c->stream));
        float e = 0.f;
        HIPCHK(c, hipEventElapsedTime(&e, a, b));
        tot += e;
    }
    hipEventDestroy(a);
    hipEventDestroy(b);
    *ms = tot / reps;
    return KSS_OK;
}
int kss_profile_get(kss_ctx* c, int k, double* total_ms, int64_t* launches) {
    if (!c || k < 0 || k >= KSS_K_COUNT) return KSS_ERR_ARG;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    if (total_ms) *total_ms = c->prof_ms[k];
    if (launches) *launches = c->prof_n[k];
    return KSS_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// C-ABI: compute entry points
// ---------------------------------------------------------------------------------------------
extern "C" {

int kss_icp_default_params(kss_icp_params* p) {
    if (!p) return KSS_ERR_ARG;
    std::memset(p, 0, sizeof *p);
    p->max_iterations = 1000;             // Main_KSS_ICP.cpp:81
    p->max_corr_dist = 1.0;               // KSS_ICP.hpp:156
    p->transformation_epsilon = 1e-10;    // :157
    p->euclidean_fitness_epsilon = 0.001; // :158
    p->abs_mse_epsilon = 1e-12;
    p->min_correspondences = 3;
    p->compute_fitness = 1;
    return KSS_OK;
}

int kss_icp_dev(kss_ctx* c, const float* d_src, int64_t ns, const float* d_tgt, int64_t nt,
                const kss_icp_params* p, kss_icp_result* res) {
    if (!c) return KSS_ERR_ARG;
    if (ns <= 0 || nt <= 0) return set_err(c, KSS_ERR_ARG, "icp: empty cloud");
    const int64_t so[2] = {0, ns}, to[2] = {0, nt};
    return icp_run_dev(c, d_src, so, d_tgt, to, 1, false, KSS_F32, p, res);
}

int kss_icp(kss_ctx* c, const float* src, int64_t ns, const float* tgt, int64_t nt,
            const kss_icp_params* p, kss_icp_result* res) {
    if (!c || !src || !tgt) return set_err(c, KSS_ERR_ARG, "icp: null cloud");
    if (ns <= 0 || nt <= 0) return set_err(c, KSS_ERR_ARG, "icp: empty cloud");
    HIPCHK(c, hipSetDevice(c->device));
    KCHK(upload(c, c->stage_src, src, (size_t)ns * 3 * sizeof(float)));
    KCHK(upload(c, c->stage_tgt, tgt, (size_t)nt * 3 * sizeof(float)));
    return kss_icp_dev(c, (const float*)c->stage_src.p, ns, (const float*)c->stage_tgt.p, nt, p, res);
}

int kss_icp_batch_dev(kss_ctx* c, const float* d_src_all, const int64_t* src_off, const float* d_tgt_all,
                      const int64_t* tgt_off, int npairs, const kss_icp_params* p, kss_icp_result* results) {
    if (!c) return KSS_ERR_ARG;
    return icp_run_dev(c, d_src_all, src_off, d_tgt_all, tgt_off, npairs, false, KSS_F32, p, results);
}

int kss_icp_batch(kss_ctx* c, const float* src_all, const int64_t* src_off, const float* tgt_all,
                  const int64_t* tgt_off, int npairs, const kss_icp_params* p, kss_icp_result* results) {
    if (!c || !src_all || !tgt_all || !src_off || !tgt_off || npairs <= 0) return set_err(c, KSS_ERR_ARG, "icp_batch: bad argument");
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t s0 = src_off[0], s1 = src_off[npairs], t0 = tgt_off[0], t1 = tgt_off[npairs];
    if (s1 <= s0 || t1 <= t0) return set_err(c, KSS_ERR_ARG, "icp_batch: empty batch");
    KCHK(upload(c, c->stage_src, src_all + 3 * s0, (size_t)(s1 - s0) * 3 * sizeof(float)));
    KCHK(upload(c, c->stage_tgt, tgt_all + 3 * t0, (size_t)(t1 - t0) * 3 * sizeof(float)));
    std::vector<int64_t> so(npairs + 1), to(npairs + 1);
    for (int i = 0; i <= npairs; ++i) { so[i] = src_off[i] - s0; to[i] = tgt_off[i] - t0; }
    return icp_run_dev(c, c->stage_src.p, so.data(), c->stage_tgt.p, to.data(), npairs, false, KSS_F32, p, results);
}

// ---- NN -----------------------------------------------------------------------------------------
int kss_nn_dev(kss_ctx* c, const float* d_src, int64_t ns, const float* d_tgt, int64_t nt, int32_t* d_idx, float* d_d2) {
    return nn_generic_dev(c, d_src, ns, d_tgt, nt, KSS_F32, d_idx, d_d2, nullptr);
}

int kss_nn(kss_ctx* c, const float* src, int64_t ns, const float* tgt, int64_t nt, int32_t* idx, float* d2) {
    if (!c || !src || !tgt) return set_err(c, KSS_ERR_ARG, "nn: null cloud");
    if (ns <= 0 || nt <= 0) return set_err(c, KSS_ERR_ARG, "nn: empty cloud");
    HIPCHK(c, hipSetDevice(c->device));
    KCHK(upload(c, c->stage_src, src, (size_t)ns * 3 * sizeof(float)));
    KCHK(upload(c, c->stage_tgt, tgt, (size_t)nt * 3 * sizeof(float)));
    KCHK(ensure(c, c->stage_idx, (size_t)ns * sizeof(int32_t)));
    KCHK(ensure(c, c->stage_d2, (size_t)ns * sizeof(float)));
    KCHK(kss_nn_dev(c, (const float*)c->stage_src.p, ns, (const float*)c->stage_tgt.p, nt, (int32_t*)c->stage_idx.p, (float*)c->stage_d2.p));
    if (idx) HIPCHK(c, hipMemcpyAsync(idx, c->stage_idx.p, (size_t)ns * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (d2) HIPCHK(c, hipMemcpyAsync(d2, c->stage_d2.p, (size_t)ns * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return KSS_OK;
}

// ---- k-NN and normals -------------------------------------------------------------------------------
static int knn_generic_dev(kss_ctx* c, const void* d_q, int64_t nq, const void* d_t, int64_t nt, int dtype, int k, int32_t* d_idx, float* d_d2) {
    if (!c || !d_q || !d_t || !d_idx || !d_d2) return set_err(c, KSS_ERR_ARG, "knn: null argument");
    if (nq <= 0 || nt <= 0 || k < 1 || k > 64) return set_err(c, KSS_ERR_ARG, "knn: need nq, nt > 0 and 1 <= k <= 64");
    if (nq > 0x7fff0000ll || nt > 0x7fff0000ll) return set_err(c, KSS_ERR_ARG, "knn: cloud too large");
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t nt_pad = (nt + NN_TILE - 1) / NN_TILE * NN_TILE;
    KCHK(ensure(c, c->tgt4, (size_t)nt_pad * sizeof(float4)));
    KCHK(ensure(c, c->src0, (size_t)nq * sizeof(float4)));
    if (dtype == KSS_F64) {
        launch_pack_f64_to_f4(c->stream, (const double*)d_q, nq, (float4*)c->src0.p, nq, false);
        launch_pack_f64_to_f4(c->stream, (const double*)d_t, nt, (float4*)c->tgt4.p, nt_pad, true);
    } else {
        launch_pack_f3_to_f4(c->stream, (const float*)d_q, nq, (float4*)c->src0.p, nq, false);
        launch_pack_f3_to_f4(c->stream, (const float*)d_t, nt, (float4*)c->tgt4.p, nt_pad, true);
    }
    size_t part_bytes = 0;
    const int n_split = knn_plan_splits((int)nq, (int)nt_pad, k, &part_bytes);   // few queries x many targets: split the targets
    if (part_bytes) KCHK(ensure(c, c->keys, part_bytes));
    {
        ProfScope ps(c, KSS_K_NN_SWEEP);
        launch_knn_sweep(c->stream, (const float4*)c->src0.p, (int)nq, (const float4*)c->tgt4.p, (int)nt_pad, k, d_idx, d_d2, n_split,
                         part_bytes ? c->keys.p : nullptr);
    }
    HIPCHK(c, hipGetLastError());
    return KSS_OK;
}

int kss_knn_dev(kss_ctx* c, const float* d_query, int64_t nq, const float* d_tgt, int64_t nt, int k, int32_t* d_idx, float* d_d2) {
    KCHK(knn_generic_dev(c, d_query, nq, d_tgt, nt, KSS_F32, k, d_idx, d_d2));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return KSS_OK;
}

int kss_knn(kss_ctx* c, const float* query, int64_t nq, const float* tgt, int64_t nt, int k, int32_t* idx, float* d2) {
    if (!c || !query || !tgt || !idx || !d2) return set_err(c, KSS_ERR_ARG, "knn: null argument");
    if (nq <= 0 || nt <= 0 || k < 1 || k > 64) return set_err(c, KSS_ERR_ARG, "knn: need nq, nt > 0 and 1 <= k <= 64");
    HIPCHK(c, hipSetDevice(c->device));
    KCHK(upload(c, c->stage_src, query, (size_t)nq * 3 * sizeof(float)));
    KCHK(upload(c, c->stage_tgt, tgt, (size_t)nt * 3 * sizeof(float)));
    KCHK(ensure(c, c->stage_idx, (size_t)nq * k * sizeof(int32_t)));
    KCHK(ensure(c, c->stage_d2, (size_t)nq * k * sizeof(float)));
    KCHK(knn_generic_dev(c, c->stage_src.p, nq, c->stage_tgt.p, nt, KSS_F32, k, (int32_t*)c->stage_idx.p, (float*)c->stage_d2.p));
    HIPCHK(c, hipMemcpyAsync(idx, c->stage_idx.p, (size_t)nq * k * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(d2, c->stage_d2.p, (size_t)nq * k * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return KSS_OK;
}

int kss_normals(kss_ctx* c, const double* pts, int64_t n, int k, double* normals) {
    if (!c || !pts || !normals) return set_err(c, KSS_ERR_ARG, "normals: null argument");
    if (n <= 0 || k < 1 || k > 64) return set_err(c, KSS_ERR_ARG, "normals: need n > 0 and 1 <= k <= 64");
    if (k > n) k = (int)n;
    HIPCHK(c, hipSetDevice(c->device));
    KCHK(upload(c, c->scratch_a, pts, (size_t)n * 3 * sizeof(double)));
    KCHK(ensure(c, c->stage_idx, (size_t)n * k * sizeof(int32_t)));
    KCHK(ensure(c, c->stage_d2, (size_t)n * k * sizeof(float)));
    KCHK(ensure(c, c->stage_out, (size_t)n * 3 * sizeof(double)));
    // self k-NN on the float-narrowed cloud (cloud_i.x = pointsVector[i][0]); src0 then holds the cloud as float4
    KCHK(knn_generic_dev(c, c->scratch_a.p, n, c->scratch_a.p, n, KSS_F64, k, (int32_t*)c->stage_idx.p, (float*)c->stage_d2.p));
    launch_normals(c->stream, (const float4*)c->src0.p, (int)n, (const int32_t*)c->stage_idx.p, k, (double*)c->stage_out.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(normals, c->stage_out.p, (size_t)n * 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return KSS_OK;
}

// estimateNormal_RegularNormal (normalCompute.hpp:614-742): consistent orientation by level-synchronous propagation
// over the 8-NN graph from point 0.  The 8-NN of every point is the device's work (n x 8 exact neighbours); the
// propagation itself is an O(8 n) graph walk whose levels depend on each other, hundreds of them on a surface:
// it runs on the host (one pass over the lists, a per-level stamp instead of the reference's quadratic
// "already listed" scan -- same first-occurrence order, same parents, same result).
int kss_normals_orient(kss_ctx* c, const double* pts, int64_t n, double* normals) {
    if (!c || !pts || !normals) return set_err(c, KSS_ERR_ARG, "normals_orient: null argument");
    if (n <= 0 || n > 0x7fff0000ll) return set_err(c, KSS_ERR_ARG, "normals_orient: bad size");
    HIPCHK(c, hipSetDevice(c->device));
    const int Kn = 8;                                   // :639
    const int k = n < Kn ? (int)n : Kn;
    KCHK(upload(c, c->scratch_a, pts, (size_t)n * 3 * sizeof(double)));
    KCHK(ensure(c, c->stage_idx, (size_t)n * k * sizeof(int32_t)));
    KCHK(ensure(c, c->stage_d2, (size_t)n * k * sizeof(float)));
    KCHK(knn_generic_dev(c, c->scratch_a.p, n, c->scratch_a.p, n, KSS_F64, k, (int32_t*)c->stage_idx.p, (float*)c->stage_d2.p));
    std::vector<int32_t> ki((size_t)n * k);
    std::vector<float> kd((size_t)n * k);
    HIPCHK(c, hipMemcpyAsync(ki.data(), c->stage_idx.p, ki.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(kd.data(), c->stage_d2.p, kd.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::vector<char> judge((size_t)n, 0);
    std::vector<int64_t> listed((size_t)n, -1);
    std::vector<int32_t> cur(1, 0), nxt, par;
    judge[0] = 1;                                       // start = 0 (:616, :674)
    for (int64_t level = 0; !cur.empty(); ++level) {
        nxt.clear(); par.clear();
        for (const int32_t u : cur) {
            const size_t row = (size_t)u * k;
            const int first = kd[row] == 0 ? 1 : 0;      // the query itself leads the list when its distance is 0 (:660-665)
            for (int j = first; j < first + k - 1 && j < k; ++j) {
                const int32_t v = ki[row + j];
                if (judge[(size_t)v] || listed[(size_t)v] == level) continue;
                listed[(size_t)v] = level;
                nxt.push_back(v); par.push_back(u);
            }
        }
        for (size_t a = 0; a < nxt.size(); ++a) {
            const double* np_ = normals + 3 * (size_t)par[a];
            double* ns = normals + 3 * (size_t)nxt[a];
            double a1 = np_[0] * ns[0] + np_[1] * ns[1] + np_[2] * ns[2];
            double a2 = -np_[0] * ns[0] - np_[1] * ns[1] - np_[2] * ns[2];
            a1 = a1 > 1 ? 1 : (a1 < -1 ? -1 : a1);
            a2 = a2 > 1 ? 1 : (a2 < -1 ? -1 : a2);
            if (std::acos(a1) > std::acos(a2)) { ns[0] = -ns[0]; ns[1] = -ns[1]; ns[2] = -ns[2]; }   // :716-735
            judge[(size_t)nxt[a]] = 1;
        }
        cur.swap(nxt);
    }
    return KSS_OK;
}

// ---- covariance sums -----------------------------------------------------------------------------
int kss_cov_dev(kss_ctx* c, const float* d_src, const float* d_tgt, const int32_t* d_idx, int64_t n, int64_t nt,
                double max_d2, double sums[KSS_NSUMS]) {
    if (!c || !d_src || !d_tgt || !d_idx || !sums) return set_err(c, KSS_ERR_ARG, "cov: null argument");
    if (n <= 0 || nt <= 0) return set_err(c, KSS_ERR_ARG, "cov: empty input");
    HIPCHK(c, hipSetDevice(c->device));
    const int nb = stream_blocks(n);
    KCHK(ensure(c, c->partials, (size_t)nb * NSUMS * sizeof(double)));
    KCHK(ensure(c, c->sums, NSUMS * sizeof(double)));
    KCHK(ensure_pinned(c, c->h_sums, c->h_sums_cap, NSUMS * sizeof(double)));
    {
        ProfScope ps(c, KSS_K_CORR_REDUCE);
        launch_corr_reduce_idx(c->stream, d_src, d_tgt, d_idx, n, max_d2, (double*)c->partials.p, nb);
        launch_sum_columns(c->stream, (const double*)c->partials.p, nb, NSUMS, (double*)c->sums.p);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(c->h_sums, c->sums.p, NSUMS * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::memcpy(sums, c->h_sums, NSUMS * sizeof(double));
    return KSS_OK;
}

int kss_cov(kss_ctx* c, const float* src, const float* tgt, const int32_t* idx, int64_t n, int64_t nt, double max_d2,
            double sums[KSS_NSUMS]) {
    if (!c || !src || !tgt || !idx || !sums) return set_err(c, KSS_ERR_ARG, "cov: null argument");
    if (n <= 0 || nt <= 0) return set_err(c, KSS_ERR_ARG, "cov: empty input");
    for (int64_t i = 0; i < n; ++i)
        if (idx[i] < 0 || idx[i] >= nt) return set_err(c, KSS_ERR_ARG, "cov: index out of range");
    HIPCHK(c, hipSetDevice(c->device));
    KCHK(upload(c, c->stage_src, src, (size_t)n * 3 * sizeof(float)));
    KCHK(upload(c, c->stage_tgt, tgt, (size_t)nt * 3 * sizeof(float)));
    KCHK(upload(c, c->stage_idx, idx, (size_t)n * sizeof(int32_t)));
    return kss_cov_dev(c, (const float*)c->stage_src.p, (const float*)c->stage_tgt.p, (const int32_t*)c->stage_idx.p, n, nt, max_d2, sums);
}

int kss_rigid_from_sums(const double sums[KSS_NSUMS], float T[16]) {
    if (!sums || !T) return KSS_ERR_ARG;
    if (!(sums[0] >= 1.0)) return KSS_ERR_ARG;
    rigid_from_sums(sums, T);
    return KSS_OK;
}

// ---- the pair metrics --------------------------------------------------------------
// What the 48 entry points kss_*_sums, kss_icp_* and kss_icp_*_batch of p2l, trimmed, sim, robust, gicp, symm, symm_robust, o2o and
// recip (its batch: kss_icp_recip_pairs) share.  A host entry and its _dev twin call one internal function with `host` set or not, and that function reads: family
// check, shared check (pair_check / sums_check), pair_enter, pair_normals, the family's mode, the run (pair_go / pair_record_dev).
static inline bool trim_overlap_ok(double overlap) { return overlap > 0.0 && overlap <= 1.0; }   // (a NaN fails both)

// What a call brings.  Host pointers at a host entry until pair_enter has staged them, device pointers otherwise.
struct PairClouds {
    const float* src = nullptr;
    const float* tgt = nullptr;
    const float* snrm = nullptr;          // the source's normals (generalized, symmetric) and the target's; null: none given
    const float* tnrm = nullptr;
    int64_t ns = 0, nt = 0;               // one pair (*_sums: n, nt); a batch behind pair_rebase: the totals
    bool batch = false;                   // a batch: npairs + 1 offsets in points per side, from 0 behind pair_rebase
    const int64_t* src_off = nullptr;
    const int64_t* tgt_off = nullptr;
    int npairs = 1;
    std::vector<int64_t> so, to;          // (pair_rebase's offsets)
};
static PairClouds one_pair(const float* src, int64_t ns, const float* snrm, const float* tgt, int64_t nt, const float* tnrm) {
    PairClouds P;
    P.src = src; P.ns = ns; P.snrm = snrm; P.tgt = tgt; P.nt = nt; P.tnrm = tnrm;
    return P;
}
static PairClouds many_pairs(const float* src, const int64_t* src_off, const float* snrm, const float* tgt, const int64_t* tgt_off,
                             const float* tnrm, int npairs) {
    PairClouds P;
    P.src = src; P.src_off = src_off; P.snrm = snrm; P.tgt = tgt; P.tgt_off = tgt_off; P.tnrm = tnrm; P.npairs = npairs; P.batch = true;
    return P;
}

// the family check of the families whose parameters hold nothing to check beyond what pair_check reads
static int params_check(kss_ctx* c, const char* who, const void* params) {
    return params ? KSS_OK : set_err(c, KSS_ERR_ARG, (std::string(who) + ": null argument").c_str());
}

// The shared check of every kss_icp_* entry, single pair and batch.  who: the name the messages carry; out: the result(s); noun: the
// family as the allreduce refusal names it; overlap (null: not a trimmed family), metric, overlaps (may be null: *overlap for every
// pair): what the trimmed families' parameters hold.  A batch's counts come from the npairs + 1 offsets; ns / nt are not read.
static int pair_check(kss_ctx* c, const char* who, const PairClouds& P, const kss_icp_params* p, const void* out, const char* noun,
                      const double* overlap = nullptr, int metric = KSS_METRIC_PLANE, const double* overlaps = nullptr) {
    if (!c) return KSS_ERR_ARG;
    const std::string w = std::string(who) + ": ";
    auto bad = [&](const std::string& what) { return set_err(c, KSS_ERR_ARG, (w + what).c_str()); };
    if (P.batch && (!P.src_off || !P.tgt_off || P.npairs <= 0)) return bad("bad batch");
    if (!P.src || !P.tgt || !p || !out) return bad("null argument");
    if (P.batch) {
        for (int i = 0; i < P.npairs; ++i) {
            const int64_t n = P.src_off[i + 1] - P.src_off[i], m = P.tgt_off[i + 1] - P.tgt_off[i];
            if (n <= 0 || m <= 0) return bad("empty pair");
            if (n > 0x7fff0000ll || m > 0x7fff0000ll) return bad("cloud too large");
        }
        if (P.src_off[P.npairs] - P.src_off[0] > 0x7fff0000ll || P.tgt_off[P.npairs] - P.tgt_off[0] > 0x7fff0000ll) return bad("batch too large");
    } else {
        if (P.ns <= 0 || P.nt <= 0) return bad("empty cloud");
        if (P.ns > 0x7fff0000ll || P.nt > 0x7fff0000ll) return bad("cloud too large");
    }
    if (p->allreduce) return bad(std::string("the source-row split (allreduce) is not available for ") + noun);
    if (!overlap) return KSS_OK;
    if (overlaps) {
        for (int i = 0; i < P.npairs; ++i)
            if (!trim_overlap_ok(overlaps[i])) return bad("overlap must be in (0, 1]");
    } else if (!trim_overlap_ok(*overlap)) return bad("overlap must be in (0, 1]");
    if (metric != KSS_METRIC_POINT && metric != KSS_METRIC_PLANE) return bad("unknown metric");
    if (metric == KSS_METRIC_POINT && P.tnrm) return bad("the point metric takes no normals");
    return KSS_OK;
}

// the same of every kss_*_sums entry; also: the entry's further required pointers are there
static int sums_check(kss_ctx* c, const char* who, const PairClouds& P, const int32_t* idx, const double* sums, bool also = true) {
    if (!c) return KSS_ERR_ARG;
    const std::string w = std::string(who) + ": ";
    if (!P.src || !P.tgt || !idx || !sums || !also) return set_err(c, KSS_ERR_ARG, (w + "null argument").c_str());
    if (P.ns <= 0 || P.nt <= 0) return set_err(c, KSS_ERR_ARG, (w + "empty input").c_str());
    if (P.ns > 0x7fff0000ll || P.nt > 0x7fff0000ll) return set_err(c, KSS_ERR_ARG, (w + "cloud too large").c_str());
    return KSS_OK;
}

// A batch's offsets rebased to its first pair and its pointers advanced to it, so that every buffer of the call is indexed from 0
// (pointer arithmetic only: host and device pointers alike); P.ns / P.nt become the totals.
static void pair_rebase(PairClouds& P) {
    if (!P.batch) return;
    const int64_t s0 = P.src_off[0], t0 = P.tgt_off[0];
    P.so.resize((size_t)P.npairs + 1); P.to.resize((size_t)P.npairs + 1);
    for (int i = 0; i <= P.npairs; ++i) { P.so[i] = P.src_off[i] - s0; P.to[i] = P.tgt_off[i] - t0; }
    P.src_off = P.so.data(); P.tgt_off = P.to.data();
    P.ns = P.so[P.npairs]; P.nt = P.to[P.npairs];
    P.src += 3 * s0; P.tgt += 3 * t0;
    if (P.snrm) P.snrm += 3 * s0;
    if (P.tnrm) P.tnrm += 3 * t0;
}

// Host callers: the clouds, the normals given and (*_sums) the correspondences go to the device, and P / *idx hold device pointers.
// One pair: stage_src, stage_tgt, gicp_snrm, p2l_nrm; a batch: its slice of the packed arrays into stage_src, stage_tgt, pb_snrm, pb_nrm.
static int pair_stage(kss_ctx* c, PairClouds& P, const int32_t** idx) {
    const size_t sb = (size_t)P.ns * 3 * sizeof(float), tb = (size_t)P.nt * 3 * sizeof(float);
    KCHK(upload(c, c->stage_src, P.src, sb));
    KCHK(upload(c, c->stage_tgt, P.tgt, tb));
    P.src = (const float*)c->stage_src.p; P.tgt = (const float*)c->stage_tgt.p;
    if (P.snrm) {
        DevBuf& b = P.batch ? c->pb_snrm : c->gicp_snrm;
        KCHK(upload(c, b, P.snrm, sb));
        P.snrm = (const float*)b.p;
    }
    if (P.tnrm) {
        DevBuf& b = P.batch ? c->pb_nrm : c->p2l_nrm;
        KCHK(upload(c, b, P.tnrm, tb));
        P.tnrm = (const float*)b.p;
    }
    if (idx) {
        KCHK(upload(c, c->stage_idx, *idx, (size_t)P.ns * sizeof(int32_t)));
        *idx = (const int32_t*)c->stage_idx.p;
    }
    return KSS_OK;
}

// Behind the checks: the call's clouds on the device, indexed from 0.  range_who: a host *_sums entry that refuses correspondences
// outside the target under that name (kss_sim_sums and kss_robust_sums never looked at theirs).
static int pair_enter(kss_ctx* c, bool host, PairClouds& P, const int32_t** idx = nullptr, const char* range_who = nullptr) {
    if (host && range_who)
        for (int64_t i = 0; i < P.ns; ++i)
            if ((*idx)[i] < 0 || (*idx)[i] >= P.nt) return set_err(c, KSS_ERR_ARG, (std::string(range_who) + ": index out of range").c_str());
    HIPCHK(c, hipSetDevice(c->device));
    pair_rebase(P);
    return host ? pair_stage(c, P, idx) : KSS_OK;
}

// A cloud's normals where the caller gave none: kss_normals' definition (k incl. the point itself, view-point flip, renormalised
// in double) on the cloud widened to f64 -- whose float narrowing is the cloud itself -- then rounded to float, into `out`
static int cloud_normals_dev(kss_ctx* c, const float* d_pts, int64_t n, int kk, DevBuf& out, const float** d_nrm) {
    const int k = n < kk ? (int)n : kk;
    KCHK(ensure(c, c->p2l_idx, (size_t)n * k * sizeof(int32_t)));
    KCHK(ensure(c, c->p2l_d2, (size_t)n * k * sizeof(float)));
    KCHK(ensure(c, c->p2l_n64, (size_t)n * 3 * sizeof(double)));
    KCHK(ensure(c, out, (size_t)n * 3 * sizeof(float)));
    KCHK(knn_generic_dev(c, d_pts, n, d_pts, n, KSS_F32, k, (int32_t*)c->p2l_idx.p, (float*)c->p2l_d2.p));
    launch_normals(c->stream, (const float4*)c->src0.p, (int)n, (const int32_t*)c->p2l_idx.p, k, (double*)c->p2l_n64.p);
    launch_f64_to_f32(c->stream, (const double*)c->p2l_n64.p, n * 3, (float*)out.p);
    HIPCHK(c, hipGetLastError());
    *d_nrm = (const float*)out.p;
    return KSS_OK;
}
// The same for every cloud of a batch, cloud after cloud (off: npairs + 1 offsets in points from 0), into the packed buffer `out`
// laid out like the clouds (setup cost of the call, not optimised: a k-NN and a normals launch per cloud); p2l_nrm is the scratch.
static int batch_normals_dev(kss_ctx* c, const float* d_pts, const int64_t* off, int npairs, int k, DevBuf& out, const float** d_nrm) {
    KCHK(ensure(c, out, (size_t)off[npairs] * 3 * sizeof(float)));
    for (int i = 0; i < npairs; ++i) {
        const int64_t n = off[i + 1] - off[i];
        const float* one = nullptr;
        KCHK(cloud_normals_dev(c, d_pts + 3 * off[i], n, k, c->p2l_nrm, &one));
        HIPCHK(c, hipMemcpyAsync((float*)out.p + 3 * off[i], one, (size_t)n * 3 * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    }
    *d_nrm = (const float*)out.p;
    return KSS_OK;
}
// Whichever normals of the call are missing, at k (20 for the plane metric, normals_k for generalized and symmetric), from the clouds
// as passed in: the target's into p2l_nrm (a batch: pb_nrm) and, source set, the source's into gicp_snrm (pb_snrm).
static int pair_normals(kss_ctx* c, PairClouds& P, int k, bool source) {
    if (!P.tnrm) KCHK(P.batch ? batch_normals_dev(c, P.tgt, P.tgt_off, P.npairs, k, c->pb_nrm, &P.tnrm)
                              : cloud_normals_dev(c, P.tgt, P.nt, k, c->p2l_nrm, &P.tnrm));
    if (source && !P.snrm) KCHK(P.batch ? batch_normals_dev(c, P.src, P.src_off, P.npairs, k, c->pb_snrm, &P.snrm)
                                        : cloud_normals_dev(c, P.src, P.ns, k, c->gicp_snrm, &P.snrm));
    return KSS_OK;
}

static RobustScale robust_scale_of(const kss_robust_params* rp, double scale);

// The run.  One pair: pair_run_dev, info its last_info.  A batch: pairs_run_dev, info its info_all, with the per-pair tables of the
// mode: the mode's own value for every pair unless the caller's array (overlaps, scales of rp, epsilons, aligns) gives each its own.
static int pair_go(kss_ctx* c, const PairClouds& P, const kss_icp_params* p, PairMode mode, kss_icp_result* res, double* info,
                   const double* overlaps = nullptr, const kss_robust_params* rp = nullptr, const double* scales = nullptr,
                   const double* epsilons = nullptr, const int32_t* aligns = nullptr) {
    if (!P.batch) {
        mode.last_info = info;
        return pair_run_dev(c, P.src, P.ns, P.tgt, P.nt, P.tnrm, p, mode, res);
    }
    const size_t np = (size_t)P.npairs;
    std::vector<double> ov(np, mode.overlap), eps(np, mode.gicp_epsilon);
    std::vector<RobustScale> rs(np, mode.rs);
    std::vector<int32_t> al(np, mode.symm_align);
    if (overlaps) ov.assign(overlaps, overlaps + np);
    if (scales)
        for (size_t i = 0; i < np; ++i) rs[i] = robust_scale_of(rp, scales[i]);
    if (epsilons) eps.assign(epsilons, epsilons + np);
    if (aligns) al.assign(aligns, aligns + np);
    return pairs_run_dev(c, P.src, P.src_off, P.tgt, P.tgt_off, P.tnrm, P.npairs, p, mode, mode.trimmed ? ov.data() : nullptr, res, info,
                         mode.robust ? rs.data() : nullptr, mode.gicp ? eps.data() : nullptr, mode.symm ? al.data() : nullptr);
}

// ---- point-to-plane -------------------------------------------------------------
static PairMode p2l_mode_of() {
    PairMode mode;
    mode.plane = true;
    return mode;
}

static int p2l_sums_any(kss_ctx* c, bool host, PairClouds P, const int32_t* idx, double max_d2, double* sums) {
    KCHK(sums_check(c, "p2l_sums", P, idx, sums, P.tnrm != nullptr));
    KCHK(pair_enter(c, host, P, &idx, "p2l_sums"));
    return pair_record_dev(c, P.src, P.tgt, P.tnrm, idx, P.ns, P.nt, max_d2, p2l_mode_of(), nullptr, sums, nullptr);
}
int kss_p2l_sums_dev(kss_ctx* c, const float* d_src, const float* d_tgt, const float* d_nrm, const int32_t* d_idx, int64_t n,
                     int64_t nt, double max_d2, double sums[KSS_P2L_NSUMS]) {
    return p2l_sums_any(c, false, one_pair(d_src, n, nullptr, d_tgt, nt, d_nrm), d_idx, max_d2, sums);
}
int kss_p2l_sums(kss_ctx* c, const float* src, const float* tgt, const float* nrm, const int32_t* idx, int64_t n, int64_t nt,
                 double max_d2, double sums[KSS_P2L_NSUMS]) {
    return p2l_sums_any(c, true, one_pair(src, n, nullptr, tgt, nt, nrm), idx, max_d2, sums);
}

int kss_rigid_from_p2l_sums(const double sums[KSS_P2L_NSUMS], float T[16]) {
    if (!sums || !T) return KSS_ERR_ARG;
    if (!rigid_from_p2l_sums(sums, T)) {
        mat4_identity(T);
        return KSS_ERR_DEGENERATE;
    }
    return KSS_OK;
}

static int icp_p2l_any(kss_ctx* c, const char* who, bool host, PairClouds P, const kss_icp_params* p, kss_icp_result* res) {
    KCHK(pair_check(c, who, P, p, res, "point-to-plane"));
    KCHK(pair_enter(c, host, P));
    KCHK(pair_normals(c, P, 20, false));
    return pair_go(c, P, p, p2l_mode_of(), res, nullptr);
}
int kss_icp_p2l_dev(kss_ctx* c, const float* d_src, int64_t ns, const float* d_tgt, int64_t nt, const float* d_nrm,
                    const kss_icp_params* p, kss_icp_result* res) {
    return icp_p2l_any(c, "icp_p2l", false, one_pair(d_src, ns, nullptr, d_tgt, nt, d_nrm), p, res);
}
int kss_icp_p2l(kss_ctx* c, const float* src, int64_t ns, const float* tgt, int64_t nt, const float* nrm,
                const kss_icp_params* p, kss_icp_result* res) {
    if (!c || !src || !tgt) return set_err(c, KSS_ERR_ARG, "icp_p2l: null cloud");   // (its own wording, kept)
    return icp_p2l_any(c, "icp_p2l", true, one_pair(src, ns, nullptr, tgt, nt, nrm), p, res);
}
int kss_icp_p2l_batch_dev(kss_ctx* c, const float* d_src_all, const int64_t* src_off, const float* d_tgt_all, const int64_t* tgt_off,
                          const float* d_nrm_all, int npairs, const kss_icp_params* p, kss_icp_result* results) {
    return icp_p2l_any(c, "icp_p2l_batch", false, many_pairs(d_src_all, src_off, nullptr, d_tgt_all, tgt_off, d_nrm_all, npairs), p, results);
}
int kss_icp_p2l_batch(kss_ctx* c, const float* src_all, const int64_t* src_off, const float* tgt_all, const int64_t* tgt_off,
                      const float* nrm_all, int npairs, const kss_icp_params* p, kss_icp_result* results) {
    return icp_p2l_any(c, "icp_p2l_batch", true, many_pairs(src_all, src_off, nullptr, tgt_all, tgt_off, nrm_all, npairs), p, results);
}

// ---- trimmed ICP ---------------------------------------------------------------
int kss_trim_rank(int64_t m, double overlap, int64_t* k) {
    if (!k || m < 0 || !trim_overlap_ok(overlap)) return KSS_ERR_ARG;
    *k = (int64_t)trim_rank_of((long long)m, overlap);
    return KSS_OK;
}

int kss_trim_threshold_dev(kss_ctx* c, const float* d_d2, int64_t n, double max_d2, double overlap, double info[KSS_TRIM_NINFO]) {
    if (!c) return KSS_ERR_ARG;
    if (!d_d2 || !info) return set_err(c, KSS_ERR_ARG, "trim_threshold: null argument");
    if (n <= 0 || n > 0x7fff0000ll) return set_err(c, KSS_ERR_ARG, "trim_threshold: n out of range");
    if (!trim_overlap_ok(overlap)) return set_err(c, KSS_ERR_ARG, "trim_threshold: overlap must be in (0, 1]");
    return trim_threshold_dev(c, d_d2, n, max_d2, overlap, info);
}

int kss_trim_threshold(kss_ctx* c, const float* d2, int64_t n, double max_d2, double overlap, double info[KSS_TRIM_NINFO]) {
    if (!c) return KSS_ERR_ARG;
    if (!d2 || !info) return set_err(c, KSS_ERR_ARG, "trim_threshold: null argument");
    if (n <= 0 || n > 0x7fff0000ll) return set_err(c, KSS_ERR_ARG, "trim_threshold: n out of range");
    if (!trim_overlap_ok(overlap)) return set_err(c, KSS_ERR_ARG, "trim_threshold: overlap must be in (0, 1]");
    HIPCHK(c, hipSetDevice(c->device));
    KCHK(upload(c, c->stage_d2, d2, (size_t)n * sizeof(float)));
    return trim_threshold_dev(c, (const float*)c->stage_d2.p, n, max_d2, overlap, info);
}

// the trimmed pass of kss_icp_trimmed; kss_icp_o2o and kss_icp_recip put their rejection in front of it (o2o_mode_of, recip_mode_of)
static PairMode trimmed_mode(double overlap, int metric, double* trace) {
    PairMode mode;
    mode.plane = metric == KSS_METRIC_PLANE;
    mode.trimmed = true;
    mode.overlap = overlap;
    mode.trace_info = trace;
    return mode;
}
static PairMode trim_mode_of(const kss_trim_params* tp) { return trimmed_mode(tp->overlap, tp->metric, tp->trace_trim); }

// the entries of the four families on the trimmed pass (trimmed, sim, o2o, recip) behind their family check; metric: as given
static int icp_trimmed_any(kss_ctx* c, const char* who, bool host, PairClouds P, const kss_icp_params* p, const PairMode& mode, int metric,
                           const double* overlaps, kss_icp_result* res, double* info) {
    KCHK(pair_check(c, who, P, p, res, "trimmed ICP", &mode.overlap, metric, overlaps));
    KCHK(pair_enter(c, host, P));
    if (mode.plane) KCHK(pair_normals(c, P, 20, false));
    return pair_go(c, P, p, mode, res, info, overlaps);
}
int kss_icp_trimmed_dev(kss_ctx* c, const float* d_src, int64_t ns, const float* d_tgt, int64_t nt, const float* d_nrm,
                        const kss_icp_params* p, const kss_trim_params* tp, kss_icp_result* res, double last_info[KSS_TRIM_NINFO]) {
    KCHK(params_check(c, "icp_trimmed", tp));
    return icp_trimmed_any(c, "icp_trimmed", false, one_pair(d_src, ns, nullptr, d_tgt, nt, d_nrm), p, trim_mode_of(tp), tp->metric, nullptr, res,
                           last_info);
}
int kss_icp_trimmed(kss_ctx* c, const float* src, int64_t ns, const float* tgt, int64_t nt, const float* nrm,
                    const kss_icp_params* p, const kss_trim_params* tp, kss_icp_result* res, double last_info[KSS_TRIM_NINFO]) {
    KCHK(params_check(c, "icp_trimmed", tp));
    return icp_trimmed_any(c, "icp_trimmed", true, one_pair(src, ns, nullptr, tgt, nt, nrm), p, trim_mode_of(tp), tp->metric, nullptr, res,
                           last_info);
}
int kss_icp_trimmed_batch_dev(kss_ctx* c, const float* d_src_all, const int64_t* src_off, const float* d_tgt_all, const int64_t* tgt_off,
                              const float* d_nrm_all, int npairs, const kss_icp_params* p, const kss_trim_params* tp, const double* overlaps,
                              kss_icp_result* results, double* info_all) {
    KCHK(params_check(c, "icp_trimmed_batch", tp));
    return icp_trimmed_any(c, "icp_trimmed_batch", false, many_pairs(d_src_all, src_off, nullptr, d_tgt_all, tgt_off, d_nrm_all, npairs), p,
                           trim_mode_of(tp), tp->metric, overlaps, results, info_all);
}
int kss_icp_trimmed_batch(kss_ctx* c, const float* src_all, const int64_t* src_off, const float* tgt_all, const int64_t* tgt_off,
                          const float* nrm_all, int npairs, const kss_icp_params* p, const kss_trim_params* tp, const double* overlaps,
                          kss_icp_result* results, double* info_all) {
    KCHK(params_check(c, "icp_trimmed_batch", tp));
    return icp_trimmed_any(c, "icp_trimmed_batch", true, many_pairs(src_all, src_off, nullptr, tgt_all, tgt_off, nrm_all, npairs), p,
                           trim_mode_of(tp), tp->metric, overlaps, results, info_all);
}

// ---- similarity ICP ----------------------------------------------------------------
int kss_sim_default_params(kss_sim_params* sp) {
    if (!sp) return KSS_ERR_ARG;
    sp->overlap = 1.0;
    sp->scale_min = 0.5; sp->scale_max = 2.0;
    sp->trace_sim = nullptr;
    return KSS_OK;
}

int kss_sim_from_sums(const double sums[KSS_NSUMS], double lo, double hi, float T[16], double* s_k) {
    if (!sums || !T || !s_k) return KSS_ERR_ARG;
    if (!(lo > 0.0) || !(lo <= hi)) return KSS_ERR_ARG;
    return sim_from_sums(sums, lo, hi, T, s_k) ? KSS_OK : KSS_ERR_DEGENERATE;
}

// the checks of sp; the overlap is the trimmed point metric's and pair_check's
static int sim_check(kss_ctx* c, const char* who, const kss_sim_params* sp) {
    const std::string w = std::string(who) + ": ";
    if (!sp) return set_err(c, KSS_ERR_ARG, (w + "null argument").c_str());
    if (!(sp->scale_min > 0.0) || !(sp->scale_min <= 1.0) || !(sp->scale_max >= 1.0) || !std::isfinite(sp->scale_max))
        return set_err(c, KSS_ERR_ARG, (w + "the scale bounds must satisfy 0 < scale_min <= 1 <= scale_max < inf").c_str());
    return KSS_OK;
}
// sp null: kss_sim_sums' record of every correspondence within max_d2 (no trimming, no selection)
static PairMode sim_mode_of(const kss_sim_params* sp) {
    PairMode mode = sp ? trimmed_mode(sp->overlap, KSS_METRIC_POINT, sp->trace_sim) : PairMode();
    mode.sim = true;
    if (sp) { mode.scale_min = sp->scale_min; mode.scale_max = sp->scale_max; }
    return mode;
}

static int sim_sums_any(kss_ctx* c, bool host, PairClouds P, const int32_t* idx, double max_d2, double* sums) {
    KCHK(sums_check(c, "sim_sums", P, idx, sums));
    KCHK(pair_enter(c, host, P, &idx));
    return pair_record_dev(c, P.src, P.tgt, nullptr, idx, P.ns, P.nt, max_d2, sim_mode_of(nullptr), nullptr, sums, nullptr);
}
int kss_sim_sums_dev(kss_ctx* c, const float* d_src, const float* d_tgt, const int32_t* d_idx, int64_t n, int64_t nt, double max_d2,
                     double sums[KSS_NSUMS]) {
    return sim_sums_any(c, false, one_pair(d_src, n, nullptr, d_tgt, nt, nullptr), d_idx, max_d2, sums);
}
int kss_sim_sums(kss_ctx* c, const float* src, const float* tgt, const int32_t* idx, int64_t n, int64_t nt, double max_d2,
                 double sums[KSS_NSUMS]) {
    return sim_sums_any(c, true, one_pair(src, n, nullptr, tgt, nt, nullptr), idx, max_d2, sums);
}

int kss_icp_sim_dev(kss_ctx* c, const float* d_src, int64_t ns, const float* d_tgt, int64_t nt, const kss_icp_params* p,
                    const kss_sim_params* sp, kss_icp_result* res, double last_info[KSS_SIM_NINFO]) {
    KCHK(sim_check(c, "icp_sim", sp));
    return icp_trimmed_any(c, "icp_sim", false, one_pair(d_src, ns, nullptr, d_tgt, nt, nullptr), p, sim_mode_of(sp), KSS_METRIC_POINT, nullptr,
                           res, last_info);
}
int kss_icp_sim(kss_ctx* c, const float* src, int64_t ns, const float* tgt, int64_t nt, const kss_icp_params* p, const kss_sim_params* sp,
                kss_icp_result* res, double last_info[KSS_SIM_NINFO]) {
    KCHK(sim_check(c, "icp_sim", sp));
    return icp_trimmed_any(c, "icp_sim", true, one_pair(src, ns, nullptr, tgt, nt, nullptr), p, sim_mode_of(sp), KSS_METRIC_POINT, nullptr, res,
                           last_info);
}
int kss_icp_sim_batch_dev(kss_ctx* c, const float* d_src, const int64_t* src_off, const float* d_tgt, const int64_t* tgt_off, int npairs,
                          const kss_icp_params* p, const kss_sim_params* sp, const double* overlaps, kss_icp_result* results, double* info_all) {
    KCHK(sim_check(c, "icp_sim_batch", sp));
    return icp_trimmed_any(c, "icp_sim_batch", false, many_pairs(d_src, src_off, nullptr, d_tgt, tgt_off, nullptr, npairs), p, sim_mode_of(sp),
                           KSS_METRIC_POINT, overlaps, results, info_all);
}
int kss_icp_sim_batch(kss_ctx* c, const float* src, const int64_t* src_off, const float* tgt, const int64_t* tgt_off, int npairs,
                      const kss_icp_params* p, const kss_sim_params* sp, const double* overlaps, kss_icp_result* results, double* info_all) {
    KCHK(sim_check(c, "icp_sim_batch", sp));
    return icp_trimmed_any(c, "icp_sim_batch", true, many_pairs(src, src_off, nullptr, tgt, tgt_off, nullptr, npairs), p, sim_mode_of(sp),
                           KSS_METRIC_POINT, overlaps, results, info_all);
}

// ---- robust ICP ----------------------------------------------------------------
static inline bool robust_loss_ok(int loss) { return loss >= KSS_LOSS_L2 && loss <= KSS_LOSS_CAUCHY; }
static inline bool robust_metric_ok(int metric) { return metric == KSS_METRIC_POINT || metric == KSS_METRIC_PLANE; }

int kss_robust_default_params(int loss, int metric, kss_robust_params* rp) {
    if (!rp || !robust_loss_ok(loss) || !robust_metric_ok(metric)) return KSS_ERR_ARG;
    rp->loss = loss; rp->metric = metric;
    rp->scale = 0.0;
    rp->tune = loss == KSS_LOSS_HUBER ? 1.345 : loss == KSS_LOSS_TUKEY ? 4.685 : loss == KSS_LOSS_CAUCHY ? 2.385 : 1.0;
    rp->min_scale = 0.0;
    rp->trace_robust = nullptr;
    return KSS_OK;
}

int kss_robust_weight(int loss, double x, double c2, double* w) {
    if (!w || !robust_loss_ok(loss)) return KSS_ERR_ARG;
    bool kept;
    *w = robust_weight_of(loss, x, c2, kept);
    return KSS_OK;
}

// K of the automatic form: the one place it is formed
static inline double robust_K(double tune) { return (tune * 1.4826) * (tune * 1.4826); }

int kss_robust_scale2(int metric, double tune, float med_key, double min_scale, double* c2) {
    if (!c2 || !robust_metric_ok(metric)) return KSS_ERR_ARG;
    if (!(tune > 0.0) || !std::isfinite(tune) || !(min_scale >= 0.0) || !(med_key >= 0.0f)) return KSS_ERR_ARG;
    const float med = med_key == 0.0f ? 0.0f : med_key;
    *c2 = robust_scale2_of(metric == KSS_METRIC_PLANE, robust_K(tune), (double)med, min_scale * min_scale);
    return KSS_OK;
}

// the checks of rp, and of a batch's per-pair scales (null: rp->scale everywhere)
static int robust_check(kss_ctx* c, const char* who, const kss_robust_params* rp, const float* nrm, int npairs = 0, const double* scales = nullptr) {
    const std::string w = std::string(who) + ": ";
    auto bad = [&](const char* what) { return set_err(c, KSS_ERR_ARG, (w + what).c_str()); };
    if (!rp) return bad("null argument");
    if (!robust_loss_ok(rp->loss)) return bad("unknown loss");
    if (!robust_metric_ok(rp->metric)) return bad("unknown metric");
    if (!(rp->scale >= 0.0) || !std::isfinite(rp->scale)) return bad("scale must be finite and >= 0");
    const bool tune_ok = rp->tune > 0.0 && std::isfinite(rp->tune);
    if (rp->scale == 0.0 && !tune_ok) return bad("tune must be finite and > 0");
    if (!(rp->min_scale >= 0.0)) return bad("min_scale must be >= 0");
    if (rp->metric == KSS_METRIC_POINT && nrm) return bad("the point metric takes no normals");
    for (int i = 0; scales && i < npairs; ++i) {
        if (!(scales[i] >= 0.0) || !std::isfinite(scales[i])) return bad("a scale must be finite and >= 0");
        if (scales[i] == 0.0 && !tune_ok) return bad("tune must be finite and > 0");
    }
    return KSS_OK;
}

// the scale of a checked rp as the kernels take it (scale: rp->scale, or the pair's own in a batch)
static RobustScale robust_scale_of(const kss_robust_params* rp, double scale) {
    RobustScale rs;
    rs.loss = rp->loss;
    rs.autoscale = scale == 0.0;
    rs.c2 = scale * scale;
    rs.K = rs.autoscale ? robust_K(rp->tune) : 0.0;
    rs.min2 = rp->min_scale * rp->min_scale;
    return rs;
}
static PairMode robust_mode_of(const kss_robust_params* rp) {
    PairMode mode;
    mode.plane = rp->metric == KSS_METRIC_PLANE;
    mode.robust = true;
    mode.rs = robust_scale_of(rp, rp->scale);
    mode.trace_info = rp->trace_robust;
    return mode;
}

// (the point metric's keys are written by the record and carry the whole candidate test; the bound is applied again, to the same effect)
static int robust_sums_any(kss_ctx* c, bool host, PairClouds P, const int32_t* idx, double max_d2, const kss_robust_params* rp, double* sums,
                           double* info) {
    KCHK(robust_check(c, "robust_sums", rp, P.tnrm));
    KCHK(sums_check(c, "robust_sums", P, idx, sums, info && (rp->metric != KSS_METRIC_PLANE || P.tnrm)));
    KCHK(pair_enter(c, host, P, &idx));
    return pair_record_dev(c, P.src, P.tgt, P.tnrm, idx, P.ns, P.nt, max_d2, robust_mode_of(rp), nullptr, sums, info);
}
int kss_robust_sums_dev(kss_ctx* c, const float* d_src, const float* d_tgt, const float* d_nrm, const int32_t* d_idx, int64_t n, int64_t nt,
                        double max_d2, const kss_robust_params* rp, double* sums, double info[KSS_ROBUST_NINFO]) {
    return robust_sums_any(c, false, one_pair(d_src, n, nullptr, d_tgt, nt, d_nrm), d_idx, max_d2, rp, sums, info);
}
int kss_robust_sums(kss_ctx* c, const float* src, const float* tgt, const float* nrm, const int32_t* idx, int64_t n, int64_t nt,
                    double max_d2, const kss_robust_params* rp, double* sums, double info[KSS_ROBUST_NINFO]) {
    return robust_sums_any(c, true, one_pair(src, n, nullptr, tgt, nt, nrm), idx, max_d2, rp, sums, info);
}

static int icp_robust_any(kss_ctx* c, const char* who, bool host, PairClouds P, const kss_icp_params* p, const kss_robust_params* rp,
                          const double* scales, kss_icp_result* res, double* info) {
    KCHK(robust_check(c, who, rp, P.tnrm, P.npairs, scales));
    KCHK(pair_check(c, who, P, p, res, "robust ICP"));
    KCHK(pair_enter(c, host, P));
    const PairMode mode = robust_mode_of(rp);
    if (mode.plane) KCHK(pair_normals(c, P, 20, false));
    return pair_go(c, P, p, mode, res, info, nullptr, rp, scales);
}
int kss_icp_robust_dev(kss_ctx* c, const float* d_src, int64_t ns, const float* d_tgt, int64_t nt, const float* d_nrm,
                       const kss_icp_params* p, const kss_robust_params* rp, kss_icp_result* res, double last_info[KSS_ROBUST_NINFO]) {
    return icp_robust_any(c, "icp_robust", false, one_pair(d_src, ns, nullptr, d_tgt, nt, d_nrm), p, rp, nullptr, res, last_info);
}
int kss_icp_robust(kss_ctx* c, const float* src, int64_t ns, const float* tgt, int64_t nt, const float* nrm, const kss_icp_params* p,
                   const kss_robust_params* rp, kss_icp_result* res, double last_info[KSS_ROBUST_NINFO]) {
    return icp_robust_any(c, "icp_robust", true, one_pair(src, ns, nullptr, tgt, nt, nrm), p, rp, nullptr, res, last_info);
}
int kss_icp_robust_batch_dev(kss_ctx* c, const float* d_src, const int64_t* src_off, const float* d_tgt, const int64_t* tgt_off,
                             const float* d_nrm, int npairs, const kss_icp_params* p, const kss_robust_params* rp, const double* scales,
                             kss_icp_result* results, double* info_all) {
    return icp_robust_any(c, "icp_robust_batch", false, many_pairs(d_src, src_off, nullptr, d_tgt, tgt_off, d_nrm, npairs), p, rp, scales, results,
                          info_all);
}
int kss_icp_robust_batch(kss_ctx* c, const float* src, const int64_t* src_off, const float* tgt, const int64_t* tgt_off, const float* nrm,
                         int npairs, const kss_icp_params* p, const kss_robust_params* rp, const double* scales, kss_icp_result* results,
                         double* info_all) {
    return icp_robust_any(c, "icp_robust_batch", true, many_pairs(src, src_off, nullptr, tgt, tgt_off, nrm, npairs), p, rp, scales, results,
                          info_all);
}

// ---- generalized ICP -----------------------------------------------------------
static inline bool gicp_epsilon_ok(double e) { return e > 0.0 && e <= 1.0; }   // (a NaN fails both)

int kss_gicp_default_params(kss_gicp_params* gp) {
    if (!gp) return KSS_ERR_ARG;
    gp->epsilon = 1e-3;
    gp->normals_k = 20;
    return KSS_OK;
}

int kss_gicp_metric(const float nq[3], const double m[3], double epsilon, double M[6], int* ok) {
    if (!nq || !m || !M || !ok || !gicp_epsilon_ok(epsilon)) return KSS_ERR_ARG;
    const double n64[3] = {(double)nq[0], (double)nq[1], (double)nq[2]};
    for (int k = 0; k < 6; ++k) M[k] = 0.0;
    bool fin = true;
    for (int k = 0; k < 3; ++k) fin = fin && std::isfinite(n64[k]) && std::isfinite(m[k]);
    *ok = fin && gicp_metric_of(n64, m, 1.0 - epsilon, M) ? 1 : 0;
    return KSS_OK;
}

// the checks of gp (need_k: a set of normals is to be computed), and of a batch's per-pair epsilons (null: gp->epsilon everywhere)
static int gicp_check(kss_ctx* c, const char* who, const kss_gicp_params* gp, bool need_k, int npairs = 0, const double* epsilons = nullptr) {
    const std::string w = std::string(who) + ": ";
    auto bad = [&](const char* what) { return set_err(c, KSS_ERR_ARG, (w + what).c_str()); };
    if (!gp) return bad("null argument");
    if (!gicp_epsilon_ok(gp->epsilon)) return bad("epsilon must be in (0, 1]");
    if (need_k && (gp->normals_k < 3 || gp->normals_k > 64)) return bad("normals_k must be in 3..64");
    for (int i = 0; epsilons && i < npairs; ++i)
        if (!gicp_epsilon_ok(epsilons[i])) return bad("every epsilon must be in (0, 1]");
    return KSS_OK;
}
// d_snrm: the source's normals on the device, given or computed
static PairMode gicp_mode_of(const kss_gicp_params* gp, const float* d_snrm) {
    PairMode mode;
    mode.plane = true;
    mode.gicp = true;
    mode.gicp_epsilon = gp->epsilon;
    mode.d_src_nrm = d_snrm;
    return mode;
}

static int gicp_sums_any(kss_ctx* c, bool host, PairClouds P, const int32_t* idx, double max_d2, const float* Rn, const kss_gicp_params* gp,
                         double* sums) {
    KCHK(gicp_check(c, "gicp_sums", gp, !P.snrm || !P.tnrm));
    KCHK(sums_check(c, "gicp_sums", P, idx, sums));
    KCHK(pair_enter(c, host, P, &idx, "gicp_sums"));
    KCHK(pair_normals(c, P, gp->normals_k, true));
    return pair_record_dev(c, P.src, P.tgt, P.tnrm, idx, P.ns, P.nt, max_d2, gicp_mode_of(gp, P.snrm), Rn, sums, nullptr);
}
int kss_gicp_sums_dev(kss_ctx* c, const float* d_src, const float* d_src_normals, const float* d_tgt, const float* d_tgt_normals,
                      const int32_t* d_idx, int64_t n, int64_t nt, double max_d2, const float Rn[9], const kss_gicp_params* gp,
                      double sums[KSS_P2L_NSUMS]) {
    return gicp_sums_any(c, false, one_pair(d_src, n, d_src_normals, d_tgt, nt, d_tgt_normals), d_idx, max_d2, Rn, gp, sums);
}
int kss_gicp_sums(kss_ctx* c, const float* src, const float* src_normals, const float* tgt, const float* tgt_normals, const int32_t* idx,
                  int64_t n, int64_t nt, double max_d2, const float Rn[9], const kss_gicp_params* gp, double sums[KSS_P2L_NSUMS]) {
    return gicp_sums_any(c, true, one_pair(src, n, src_normals, tgt, nt, tgt_normals), idx, max_d2, Rn, gp, sums);
}

static int icp_gicp_any(kss_ctx* c, const char* who, bool host, PairClouds P, const kss_icp_params* p, const kss_gicp_params* gp,
                        const double* epsilons, kss_icp_result* res) {
    KCHK(gicp_check(c, who, gp, !P.snrm || !P.tnrm, P.npairs, epsilons));
    KCHK(pair_check(c, who, P, p, res, "generalized ICP"));
    KCHK(pair_enter(c, host, P));
    KCHK(pair_normals(c, P, gp->normals_k, true));
    return pair_go(c, P, p, gicp_mode_of(gp, P.snrm), res, nullptr, nullptr, nullptr, nullptr, epsilons);
}
int kss_icp_gicp_dev(kss_ctx* c, const float* d_src, int64_t ns, const float* d_src_normals, const float* d_tgt, int64_t nt,
                     const float* d_tgt_normals, const kss_icp_params* p, const kss_gicp_params* gp, kss_icp_result* res) {
    return icp_gicp_any(c, "icp_gicp", false, one_pair(d_src, ns, d_src_normals, d_tgt, nt, d_tgt_normals), p, gp, nullptr, res);
}
int kss_icp_gicp(kss_ctx* c, const float* src, int64_t ns, const float* src_normals, const float* tgt, int64_t nt, const float* tgt_normals,
                 const kss_icp_params* p, const kss_gicp_params* gp, kss_icp_result* res) {
    return icp_gicp_any(c, "icp_gicp", true, one_pair(src, ns, src_normals, tgt, nt, tgt_normals), p, gp, nullptr, res);
}
int kss_icp_gicp_batch_dev(kss_ctx* c, const float* d_src, const int64_t* src_off, const float* d_src_normals, const float* d_tgt,
                           const int64_t* tgt_off, const float* d_tgt_normals, int npairs, const kss_icp_params* p,
                           const kss_gicp_params* gp, const double* epsilons, kss_icp_result* results) {
    return icp_gicp_any(c, "icp_gicp_batch", false, many_pairs(d_src, src_off, d_src_normals, d_tgt, tgt_off, d_tgt_normals, npairs), p, gp,
                        epsilons, results);
}
int kss_icp_gicp_batch(kss_ctx* c, const float* src, const int64_t* src_off, const float* src_normals, const float* tgt,
                       const int64_t* tgt_off, const float* tgt_normals, int npairs, const kss_icp_params* p, const kss_gicp_params* gp,
                       const double* epsilons, kss_icp_result* results) {
    return icp_gicp_any(c, "icp_gicp_batch", true, many_pairs(src, src_off, src_normals, tgt, tgt_off, tgt_normals, npairs), p, gp, epsilons,
                        results);
}

// ---- voxelized generalized ICP against a voxel map ------------------------------------
// There is no target cloud in a registration here, so these entries have a path of their own: the map's check (vmap_live), the
// source's staging and normals as pair_stage / cloud_normals_dev do them, then vgicp_record_dev / vgicp_run_dev.
int kss_vmap_default_params(kss_vmap_params* vp) {
    if (!vp) return KSS_ERR_ARG;
    vp->leaf = 0.0;   // no default: the caller sets it
    vp->normals_k = 20;
    return KSS_OK;
}

// the handle is one of this context's live maps (a map of another context, a destroyed one and null are not)
static bool vmap_live(const kss_ctx* c, const kss_vmap* m) {
    return m && std::find(c->vmaps.begin(), c->vmaps.end(), m) != c->vmaps.end();
}

// A cloud of n points and its normals onto the device: a host caller's into pts_buf and nrm_buf, normals that are not given
// computed at normals_k into nrm_buf.  pts and nrm then point at what the kernels read
static int cloud_stage(kss_ctx* c, bool host, const float*& pts, const float*& nrm, int64_t n, int normals_k, DevBuf& pts_buf, DevBuf& nrm_buf) {
    if (host) {
        const size_t bytes = (size_t)n * 3 * sizeof(float);
        KCHK(upload(c, pts_buf, pts, bytes));
        pts = (const float*)pts_buf.p;
        if (nrm) {
            KCHK(upload(c, nrm_buf, nrm, bytes));
            nrm = (const float*)nrm_buf.p;
        }
    }
    if (!nrm) KCHK(cloud_normals_dev(c, pts, n, normals_k, nrm_buf, &nrm));
    return KSS_OK;
}

// A new handle around what make(VmapBuilt&) builds, listed with the context's live maps.  make's 1 / 2 / 3 are KSS_ERR_ARG with
// the entry's `refused`, KSS_ERR_NOMEM and KSS_ERR_HIP with its `failed`, and nothing is held
static int vmap_register(kss_ctx* c, const char* who, const char* refused, const char* failed, const kss_vmap_params* vp, kss_vmap** out,
                         const std::function<int(VmapBuilt&)>& make) {
    kss_vmap* m = new (std::nothrow) kss_vmap();
    if (!m) return KSS_ERR_NOMEM;
    const int rc = make(m->b);
    if (rc != 0) {
        delete m;
        const std::string w = std::string(who) + ": ";
        if (rc == 1) return set_err(c, KSS_ERR_ARG, (w + refused).c_str());
        return rc == 2 ? set_err(c, KSS_ERR_NOMEM, (w + "hipMalloc").c_str()) : set_err(c, KSS_ERR_HIP, (w + failed).c_str());
    }
    m->ctx = c;
    m->leaf = vp->leaf;
    c->vmaps.push_back(m);
    *out = m;
    return KSS_OK;
}

static int vmap_create_any(kss_ctx* c, bool host, const float* tgt, int64_t nt, const float* nrm, const kss_vmap_params* vp, kss_vmap** out) {
    if (!c) return KSS_ERR_ARG;
    auto bad = [&](const char* what) { return set_err(c, KSS_ERR_ARG, (std::string("vmap_create: ") + what).c_str()); };
    if (out) *out = nullptr;
    if (!tgt || !vp || !out) return bad("null argument");
    if (nt <= 0) return bad("empty cloud");
    if (nt > 0x7fff0000ll) return bad("cloud too large");
    if (!(vp->leaf > 0.0) || !std::isfinite(vp->leaf)) return bad("leaf must be finite and > 0");
    if (!nrm && (vp->normals_k < 3 || vp->normals_k > 64)) return bad("normals_k must be in 3..64");
    HIPCHK(c, hipSetDevice(c->device));
    KCHK(cloud_stage(c, host, tgt, nrm, nt, vp->normals_k, c->stage_tgt, c->p2l_nrm));
    return vmap_register(c, "vmap_create", "no target with finite coordinates and normal, or a grid that is not finite or has more than 2^26 cells",
                         "the build failed", vp, out, [&](VmapBuilt& b) { return vmap_build(c->stream, tgt, nrm, nt, 1.0f / (float)vp->leaf, b); });
}
int kss_vmap_create_dev(kss_ctx* c, const float* d_tgt, int64_t nt, const float* d_tgt_normals, const kss_vmap_params* vp, kss_vmap** out) {
    return vmap_create_any(c, false, d_tgt, nt, d_tgt_normals, vp, out);
}
int kss_vmap_create(kss_ctx* c, const float* tgt, int64_t nt, const float* tgt_normals, const kss_vmap_params* vp, kss_vmap** out) {
    return vmap_create_any(c, true, tgt, nt, tgt_normals, vp, out);
}

int kss_vmap_destroy(kss_ctx* c, kss_vmap* m) {
    if (!c) return KSS_ERR_ARG;
    if (!vmap_live(c, m)) return set_err(c, KSS_ERR_ARG, "vmap_destroy: not a live map of this context");
    hipSetDevice(c->device);
    hipStreamSynchronize(c->stream);
    c->vmaps.erase(std::find(c->vmaps.begin(), c->vmaps.end(), m));
    vmap_free(m->b);
    delete m;
    return KSS_OK;
}

int kss_vmap_info(const kss_vmap* m, double info[KSS_VMAP_NINFO]) {
    if (!m || !info) return KSS_ERR_ARG;
    info[0] = (double)m->b.mapped; info[1] = (double)m->b.nvox;
    for (int a = 0; a < 3; ++a) { info[2 + a] = (double)m->b.dims[a]; info[6 + a] = (double)m->b.lo[a]; }
    info[5] = m->leaf;
    info[9] = (double)m->b.inv;
    return KSS_OK;
}

int kss_vmap_read(kss_ctx* c, const kss_vmap* m, int64_t* lin, double* stats, int64_t capacity, int64_t* nvox) {
    if (!c) return KSS_ERR_ARG;
    if (!vmap_live(c, m)) return set_err(c, KSS_ERR_ARG, "vmap_read: not a live map of this context");
    if (!nvox) return set_err(c, KSS_ERR_ARG, "vmap_read: null argument");
    *nvox = m->b.nvox;
    if ((!lin && !stats) || m->b.nvox == 0) return KSS_OK;   // the count alone; a box map nothing was inserted into has no record
    if (capacity < m->b.nvox) return set_err(c, KSS_ERR_CAPACITY, "vmap_read: output buffer too small");
    HIPCHK(c, hipSetDevice(c->device));
    if (lin) HIPCHK(c, hipMemcpyAsync(lin, m->b.lin, (size_t)m->b.nvox * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    if (stats) HIPCHK(c, hipMemcpyAsync(stats, m->b.rec, (size_t)m->b.nvox * KSS_VMAP_NSTAT * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return KSS_OK;
}

// ---- a map that grows ----
int kss_vmap_create_box(kss_ctx* c, const float lo[3], const float hi[3], const kss_vmap_params* vp, kss_vmap** out) {
    if (!c) return KSS_ERR_ARG;
    auto bad = [&](const char* what) { return set_err(c, KSS_ERR_ARG, (std::string("vmap_create_box: ") + what).c_str()); };
    if (out) *out = nullptr;
    if (!lo || !hi || !vp || !out) return bad("null argument");
    if (!(vp->leaf > 0.0) || !std::isfinite(vp->leaf)) return bad("leaf must be finite and > 0");
    HIPCHK(c, hipSetDevice(c->device));
    return vmap_register(c, "vmap_create_box", "a box that is not finite, has hi < lo, or a grid that is not finite or has more than 2^26 cells",
                         "the table's fill failed", vp, out, [&](VmapBuilt& b) { return vmap_empty(c->stream, lo, hi, 1.0f / (float)vp->leaf, b); });
}

// the cloud and its normals on the device (cloud_stage), then vmap_insert
static int vmap_insert_any(kss_ctx* c, bool host, kss_vmap* m, const float* pts, int64_t n, const float* nrm, const float* T, int normals_k,
                           double* info) {
    if (!c) return KSS_ERR_ARG;
    auto bad = [&](const char* what) { return set_err(c, KSS_ERR_ARG, (std::string("vmap_insert: ") + what).c_str()); };
    if (!pts) return bad("null argument");
    if (!vmap_live(c, m)) return bad("not a live map of this context");
    if (n <= 0) return bad("empty cloud");
    if (n > 0x7fff0000ll) return bad("cloud too large");
    if (!nrm && (normals_k < 3 || normals_k > 64)) return bad("normals_k must be in 3..64");
    for (int k = 0; T && k < 16; ++k)
        if (!std::isfinite(T[k])) return bad("T must be finite");
    HIPCHK(c, hipSetDevice(c->device));
    KCHK(cloud_stage(c, host, pts, nrm, n, normals_k, c->stage_src, c->gicp_snrm));
    int64_t counts[KSS_VMAP_NINSERT] = {0, 0, 0, 0};
    const int rc = vmap_insert(c->stream, m->b, pts, nrm, n, T, counts);
    if (rc != 0) return rc == 2 ? set_err(c, KSS_ERR_NOMEM, "vmap_insert: hipMalloc") : set_err(c, KSS_ERR_HIP, "vmap_insert: the insert failed");
    for (int k = 0; info && k < KSS_VMAP_NINSERT; ++k) info[k] = (double)counts[k];
    return KSS_OK;
}
int kss_vmap_insert_dev(kss_ctx* c, kss_vmap* m, const float* d_pts, int64_t n, const float* d_normals, const float T[16], int normals_k,
                        double info[KSS_VMAP_NINSERT]) {
    return vmap_insert_any(c, false, m, d_pts, n, d_normals, T, normals_k, info);
}
int kss_vmap_insert(kss_ctx* c, kss_vmap* m, const float* pts, int64_t n, const float* normals, const float T[16], int normals_k,
                    double info[KSS_VMAP_NINSERT]) {
    return vmap_insert_any(c, true, m, pts, n, normals, T, normals_k, info);
}

// ---- a window that slides over the lattice ----
int kss_vmap_window(const kss_vmap* m, int64_t base[3]) {
    if (!m || !base) return KSS_ERR_ARG;
    for (int a = 0; a < 3; ++a) base[a] = m->b.base[a];
    return KSS_OK;
}

// the shift by k of a live map of c; who: the entry's name in the error text
static int vmap_shift_checked(kss_ctx* c, const char* who, kss_vmap* m, const int64_t k[3], double* info) {
    constexpr int64_t LIM = 1ll << 24;   // beyond it f is not an exact integer in float
    for (int a = 0; a < 3; ++a) {
        if (k[a] > 2 * LIM || k[a] < -2 * LIM) return set_err(c, KSS_ERR_ARG, (std::string(who) + ": the window would leave +-2^24 cells").c_str());
        const int64_t nb = m->b.base[a] + k[a];
        if (nb < -LIM || nb + m->b.dims[a] > LIM) return set_err(c, KSS_ERR_ARG, (std::string(who) + ": the window would leave +-2^24 cells").c_str());
    }
    HIPCHK(c, hipSetDevice(c->device));
    int64_t counts[KSS_VMAP_NSHIFT] = {0, 0, 0, 0};
    const int rc = vmap_shift(c->stream, m->b, k, counts);
    if (rc != 0) return rc == 2 ? set_err(c, KSS_ERR_NOMEM, (std::string(who) + ": hipMalloc").c_str()) : set_err(c, KSS_ERR_HIP, (std::string(who) + ": the shift failed").c_str());
    for (int i = 0; info && i < KSS_VMAP_NSHIFT; ++i) info[i] = (double)counts[i];
    return KSS_OK;
}

int kss_vmap_shift(kss_ctx* c, kss_vmap* m, const int64_t k[3], double info[KSS_VMAP_NSHIFT]) {
    if (!c) return KSS_ERR_ARG;
    if (!k) return set_err(c, KSS_ERR_ARG, "vmap_shift: null argument");
    if (!vmap_live(c, m)) return set_err(c, KSS_ERR_ARG, "vmap_shift: not a live map of this context");
    return vmap_shift_checked(c, "vmap_shift", m, k, info);
}

int kss_vmap_recentre(kss_ctx* c, kss_vmap* m, const float centre[3], int64_t slack, int64_t k_out[3], double info[KSS_VMAP_NSHIFT]) {
    if (!c) return KSS_ERR_ARG;
    auto bad = [&](const char* what) { return set_err(c, KSS_ERR_ARG, (std::string("vmap_recentre: ") + what).c_str()); };
    if (!centre) return bad("null argument");
    if (!vmap_live(c, m)) return bad("not a live map of this context");
    if (!std::isfinite(centre[0]) || !std::isfinite(centre[1]) || !std::isfinite(centre[2])) return bad("centre must be finite");
    if (slack < 0) return bad("slack must be >= 0");
    int64_t k[3];
    if (!vmap_recentre_k(m->b, centre, slack, k)) return bad("the centre's cell is beyond +-2^24");
    const int rc = vmap_shift_checked(c, "vmap_recentre", m, k, info);
    if (rc == KSS_OK && k_out)
        for (int a = 0; a < 3; ++a) k_out[a] = k[a];
    return rc;
}

// ---- the pyramid ----
// what both coarsen entries refuse; who: the entry's name in the error text
static int vmap_coarsen_check(kss_ctx* c, const char* who, const kss_vmap* m, int k) {
    if (!vmap_live(c, m)) return set_err(c, KSS_ERR_ARG, (std::string(who) + ": not a live map of this context").c_str());
    if (k < 2 || k > 8) return set_err(c, KSS_ERR_ARG, (std::string(who) + ": k must be in 2..8").c_str());
    return KSS_OK;
}

int kss_vmap_coarsen(kss_ctx* c, const kss_vmap* m, int k, kss_vmap** out) {
    if (!c) return KSS_ERR_ARG;
    if (out) *out = nullptr;
    if (!out) return set_err(c, KSS_ERR_ARG, "vmap_coarsen: null argument");
    KCHK(vmap_coarsen_check(c, "vmap_coarsen", m, k));
    HIPCHK(c, hipSetDevice(c->device));
    kss_vmap_params vp;
    vp.leaf = (double)k * m->leaf;
    vp.normals_k = 0;   // (not read)
    return vmap_register(c, "vmap_coarsen", "", "the merge failed", &vp, out, [&](VmapBuilt& b) {
        vmap_coarsen_header(m->b, k, vp.leaf, b);
        int rc = vmap_coarsen_table(b);
        if (rc == 0) rc = vmap_coarsen_into(c->stream, m->b, k, b);
        if (rc != 0) vmap_free(b);
        return rc;
    });
}

int kss_vmap_coarsen_into(kss_ctx* c, const kss_vmap* m, int k, kss_vmap* dst) {
    if (!c) return KSS_ERR_ARG;
    auto bad = [&](const char* what) { return set_err(c, KSS_ERR_ARG, (std::string("vmap_coarsen_into: ") + what).c_str()); };
    KCHK(vmap_coarsen_check(c, "vmap_coarsen_into", m, k));
    if (!vmap_live(c, dst)) return bad("the destination is not a live map of this context");
    if (dst == m) return bad("the destination is the map itself");
    VmapBuilt h;
    const double leaf = (double)k * m->leaf;
    vmap_coarsen_header(m->b, k, leaf, h);
    // bit for bit what kss_vmap_coarsen would give (base is the refresh's to set)
    if (std::memcmp(&dst->leaf, &leaf, sizeof leaf) != 0 || std::memcmp(&dst->b.inv, &h.inv, sizeof h.inv) != 0 ||
        std::memcmp(dst->b.lo, h.lo, sizeof h.lo) != 0 || std::memcmp(dst->b.dims, h.dims, sizeof h.dims) != 0)
        return bad("the destination's lo, leaf, inv or dims are not kss_vmap_coarsen's for this map and k");
    HIPCHK(c, hipSetDevice(c->device));
    const int rc = vmap_coarsen_into(c->stream, m->b, k, dst->b);
    if (rc != 0) return rc == 2 ? set_err(c, KSS_ERR_NOMEM, "vmap_coarsen_into: hipMalloc") : set_err(c, KSS_ERR_HIP, "vmap_coarsen_into: the merge failed");
    return KSS_OK;
}

// ---- the neighbourhood of every lookup ----
// a header field on the host: nothing is launched, and the next call that looks the map up reads it (kss_vmap::nb)
int kss_vmap_set_neighbourhood(kss_ctx* c, kss_vmap* m, int nb) {
    if (!c) return KSS_ERR_ARG;
    if (!vmap_live(c, m)) return set_err(c, KSS_ERR_ARG, "vmap_set_neighbourhood: not a live map of this context");
    if (nb != KSS_VMAP_NB_1 && nb != KSS_VMAP_NB_7 && nb != KSS_VMAP_NB_27) return set_err(c, KSS_ERR_ARG, "vmap_set_neighbourhood: nb must be 1, 7 or 27");
    m->nb = nb;
    return KSS_OK;
}

int kss_vmap_neighbourhood(const kss_vmap* m, int* nb) {
    if (!m || !nb) return KSS_ERR_ARG;
    *nb = m->nb;
    return KSS_OK;
}

// what both the record and the loop check and stage: the source on the device with its normals, given or computed
static int vgicp_enter(kss_ctx* c, const char* who, bool host, const float*& src, const float*& snrm, int64_t n, const kss_vmap* m,
                       const kss_gicp_params* gp, const void* out) {
    if (!c) return KSS_ERR_ARG;
    const std::string w = std::string(who) + ": ";
    auto bad = [&](const char* what) { return set_err(c, KSS_ERR_ARG, (w + what).c_str()); };
    if (!src || !out) return bad("null argument");
    if (!vmap_live(c, m)) return bad("not a live map of this context");
    if (n <= 0) return bad("empty cloud");
    if (n > 0x7fff0000ll) return bad("cloud too large");
    KCHK(gicp_check(c, who, gp, !snrm));
    HIPCHK(c, hipSetDevice(c->device));
    return cloud_stage(c, host, src, snrm, n, gp->normals_k, c->stage_src, c->gicp_snrm);
}

static int vgicp_sums_any(kss_ctx* c, bool host, const float* src, const float* snrm, int64_t n, const kss_vmap* m, double max_d2, const float* Rn,
                          const kss_gicp_params* gp, double* sums) {
    KCHK(vgicp_enter(c, "vgicp_sums", host, src, snrm, n, m, gp, sums));
    return vgicp_record_dev(c, src, snrm, n, m, max_d2, Rn, gp->epsilon, sums);
}
int kss_vgicp_sums_dev(kss_ctx* c, const float* d_src, const float* d_src_normals, int64_t n, const kss_vmap* m, double max_d2, const float Rn[9],
                       const kss_gicp_params* gp, double sums[KSS_P2L_NSUMS]) {
    return vgicp_sums_any(c, false, d_src, d_src_normals, n, m, max_d2, Rn, gp, sums);
}
int kss_vgicp_sums(kss_ctx* c, const float* src, const float* src_normals, int64_t n, const kss_vmap* m, double max_d2, const float Rn[9],
                   const kss_gicp_params* gp, double sums[KSS_P2L_NSUMS]) {
    return vgicp_sums_any(c, true, src, src_normals, n, m, max_d2, Rn, gp, sums);
}

// who: the entry's name in the error text; T0: kss_icp_vgicp_from's start pose, or null
static int icp_vgicp_check(kss_ctx* c, const char* who, const float* T0, const kss_icp_params* p) {
    auto bad = [&](const char* what) { return set_err(c, KSS_ERR_ARG, (std::string(who) + ": " + what).c_str()); };
    if (!p) return bad("null argument");
    if (p->allreduce) return bad("the source-row split (allreduce) is not available for voxelized generalized ICP");
    if (p->fitness_idx || p->fitness_d2) return bad("there are no correspondences to return: fitness_idx and fitness_d2 must be NULL");
    for (int k = 0; T0 && k < 16; ++k)
        if (!std::isfinite(T0[k])) return bad("T0 must be finite");
    return KSS_OK;
}
static int icp_vgicp_any(kss_ctx* c, const char* who, bool host, const float* src, int64_t ns, const float* snrm, const kss_vmap* m, const float* T0,
                         const kss_icp_params* p, const kss_gicp_params* gp, kss_icp_result* res, double* last_info) {
    if (!c) return KSS_ERR_ARG;
    KCHK(icp_vgicp_check(c, who, T0, p));
    KCHK(vgicp_enter(c, who, host, src, snrm, ns, m, gp, res));
    return vgicp_run_dev(c, src, ns, snrm, m, T0, p, gp->epsilon, res, last_info);
}
int kss_icp_vgicp_dev(kss_ctx* c, const float* d_src, int64_t ns, const float* d_src_normals, const kss_vmap* m, const kss_icp_params* p,
                      const kss_gicp_params* gp, kss_icp_result* res, double last_info[KSS_VGICP_NINFO]) {
    return icp_vgicp_any(c, "icp_vgicp", false, d_src, ns, d_src_normals, m, nullptr, p, gp, res, last_info);
}
int kss_icp_vgicp(kss_ctx* c, const float* src, int64_t ns, const float* src_normals, const kss_vmap* m, const kss_icp_params* p,
                  const kss_gicp_params* gp, kss_icp_result* res, double last_info[KSS_VGICP_NINFO]) {
    return icp_vgicp_any(c, "icp_vgicp", true, src, ns, src_normals, m, nullptr, p, gp, res, last_info);
}
int kss_icp_vgicp_from_dev(kss_ctx* c, const float* d_src, int64_t ns, const float* d_src_normals, const kss_vmap* m, const float T0[16],
                           const kss_icp_params* p, const kss_gicp_params* gp, kss_icp_result* res, double last_info[KSS_VGICP_NINFO]) {
    return icp_vgicp_any(c, "icp_vgicp_from", false, d_src, ns, d_src_normals, m, T0, p, gp, res, last_info);
}
int kss_icp_vgicp_from(kss_ctx* c, const float* src, int64_t ns, const float* src_normals, const kss_vmap* m, const float T0[16],
                       const kss_icp_params* p, const kss_gicp_params* gp, kss_icp_result* res, double last_info[KSS_VGICP_NINFO]) {
    return icp_vgicp_any(c, "icp_vgicp_from", true, src, ns, src_normals, m, T0, p, gp, res, last_info);
}

// The ladder: every check before anything is staged or launched, the scan staged and its normals computed ONCE (vgicp_enter on
// the first level's map), then vgicp_c2f_run_dev
static int icp_vgicp_c2f_any(kss_ctx* c, bool host, const float* src, int64_t ns, const float* snrm, const kss_vmap* const* maps, int nlevels,
                             const float* T0, const kss_icp_params* p, const kss_gicp_params* gp, kss_icp_result* results, double* last_info) {
    if (!c) return KSS_ERR_ARG;
    const char* who = "icp_vgicp_c2f";
    auto bad = [&](const char* what) { return set_err(c, KSS_ERR_ARG, (std::string(who) + ": " + what).c_str()); };
    if (!maps || !results) return bad("null argument");
    if (nlevels < 1 || nlevels > KSS_VGICP_MAX_LEVELS) return bad("nlevels must be in 1..8");
    for (int l = 0; l < nlevels; ++l)
        if (!vmap_live(c, maps[l])) return bad("a level is not a live map of this context");
    KCHK(icp_vgicp_check(c, who, T0, p));
    KCHK(vgicp_enter(c, who, host, src, snrm, ns, maps[0], gp, results));
    return vgicp_c2f_run_dev(c, src, ns, snrm, maps, nlevels, T0, p, gp->epsilon, results, last_info);
}
int kss_icp_vgicp_c2f_dev(kss_ctx* c, const float* d_src, int64_t ns, const float* d_src_normals, const kss_vmap* const* maps, int nlevels,
                          const float T0[16], const kss_icp_params* p, const kss_gicp_params* gp, kss_icp_result* results, double* last_info) {
    return icp_vgicp_c2f_any(c, false, d_src, ns, d_src_normals, maps, nlevels, T0, p, gp, results, last_info);
}
int kss_icp_vgicp_c2f(kss_ctx* c, const float* src, int64_t ns, const float* src_normals, const kss_vmap* const* maps, int nlevels,
                      const float T0[16], const kss_icp_params* p, const kss_gicp_params* gp, kss_icp_result* results, double* last_info) {
    return icp_vgicp_c2f_any(c, true, src, ns, src_normals, maps, nlevels, T0, p, gp, results, last_info);
}

// Many scans against one map.  Every check comes before anything touches the device; then the scans as
// pair_rebase / pair_stage bring a batch in (indexed from 0, a host caller's slice into stage_src / pb_snrm), the normals that are
// missing scan by scan as kss_icp_vgicp computes them (batch_normals_dev into pb_snrm), and vgicpb_run_dev.
static int icp_vgicp_batch_any(kss_ctx* c, bool host, const float* src, const int64_t* src_off, const float* snrm, int nscans, const kss_vmap* m,
                               const kss_icp_params* p, const kss_gicp_params* gp, const double* epsilons, kss_icp_result* res, double* last_info) {
    if (!c) return KSS_ERR_ARG;
    const char* who = "icp_vgicp_batch";
    auto bad = [&](const char* what) { return set_err(c, KSS_ERR_ARG, (std::string(who) + ": " + what).c_str()); };
    if (!src || !src_off || !p || !gp || !res) return bad("null argument");
    if (nscans <= 0) return bad("bad batch");
    if (src_off[0] < 0) return bad("negative offset");
    int64_t rows = 0;
    for (int i = 0; i < nscans; ++i) {
        const int64_t n = src_off[i + 1] - src_off[i];
        if (n <= 0) return bad("empty scan");
        if (n > 0x7fff0000ll) return bad("cloud too large");
        rows += stream_blocks(n);
        if (rows > PAIRB_INDEX_MAX) return bad("batch too large for 32-bit indexing");
    }
    if (!vmap_live(c, m)) return bad("not a live map of this context");
    KCHK(gicp_check(c, who, gp, !snrm, nscans, epsilons));
    if (p->allreduce) return bad("the source-row split (allreduce) is not available for voxelized generalized ICP");
    if (p->fitness_idx || p->fitness_d2) return bad("there are no correspondences to return: fitness_idx and fitness_d2 must be NULL");
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t s0 = src_off[0];
    std::vector<int64_t> so((size_t)nscans + 1);
    for (int i = 0; i <= nscans; ++i) so[i] = src_off[i] - s0;
    src += 3 * s0;
    if (snrm) snrm += 3 * s0;
    if (host) {
        const size_t sb = (size_t)so[nscans] * 3 * sizeof(float);
        KCHK(upload(c, c->stage_src, src, sb));
        src = (const float*)c->stage_src.p;
        if (snrm) {
            KCHK(upload(c, c->pb_snrm, snrm, sb));
            snrm = (const float*)c->pb_snrm.p;
        }
    }
    if (!snrm) KCHK(batch_normals_dev(c, src, so.data(), nscans, gp->normals_k, c->pb_snrm, &snrm));
    std::vector<double> eps((size_t)nscans, gp->epsilon);
    if (epsilons) eps.assign(epsilons, epsilons + nscans);
    return vgicpb_run_dev(c, src, so.data(), snrm, nscans, m, p, eps.data(), res, last_info);
}
int kss_icp_vgicp_batch_dev(kss_ctx* c, const float* d_src_all, const int64_t* src_off, const float* d_src_normals_all, int nscans, const kss_vmap* m,
                            const kss_icp_params* p, const kss_gicp_params* gp, const double* epsilons, kss_icp_result* results, double* last_info) {
    return icp_vgicp_batch_any(c, false, d_src_all, src_off, d_src_normals_all, nscans, m, p, gp, epsilons, results, last_info);
}
int kss_icp_vgicp_batch(kss_ctx* c, const float* src_all, const int64_t* src_off, const float* src_normals_all, int nscans, const kss_vmap* m,
                        const kss_icp_params* p, const kss_gicp_params* gp, const double* epsilons, kss_icp_result* results, double* last_info) {
    return icp_vgicp_batch_any(c, true, src_all, src_off, src_normals_all, nscans, m, p, gp, epsilons, results, last_info);
}

// ---- symmetric ICP and its robust form -----------------------------
int kss_symm_default_params(kss_symm_params* sp) {
    if (!sp) return KSS_ERR_ARG;
    sp->normals_k = 20;
    sp->align_normals = 1;
    return KSS_OK;
}

int kss_rigid_from_symm_sums(const double sums[KSS_P2L_NSUMS], float T[16]) {
    if (!sums || !T) return KSS_ERR_ARG;
    if (!rigid_from_symm_sums(sums, T)) {
        mat4_identity(T);
        return KSS_ERR_DEGENERATE;
    }
    return KSS_OK;
}

// the checks of sp (need_k: a set of normals is to be computed), and of a batch's per-pair aligns (null: sp->align_normals everywhere)
static int symm_check(kss_ctx* c, const char* who, const kss_symm_params* sp, bool need_k, int npairs = 0, const int32_t* aligns = nullptr) {
    const std::string w = std::string(who) + ": ";
    auto bad = [&](const char* what) { return set_err(c, KSS_ERR_ARG, (w + what).c_str()); };
    if (!sp) return bad("null argument");
    if (sp->align_normals != 0 && sp->align_normals != 1) return bad("align_normals must be 0 or 1");
    if (need_k && (sp->normals_k < 3 || sp->normals_k > 64)) return bad("normals_k must be in 3..64");
    for (int i = 0; aligns && i < npairs; ++i)
        if (aligns[i] != 0 && aligns[i] != 1) return bad("every align must be 0 or 1");
    return KSS_OK;
}
// symm_check and, rp given, robust_check composed; the residual is a signed plane distance and the scale rule the plane metric's
static int symm_robust_check(kss_ctx* c, const char* who, const kss_symm_params* sp, const kss_robust_params* rp, bool robust, bool need_k,
                      int npairs = 0, const int32_t* aligns = nullptr, const double* scales = nullptr) {
    KCHK(symm_check(c, who, sp, need_k, npairs, aligns));
    if (!robust) return KSS_OK;
    KCHK(robust_check(c, who, rp, nullptr, npairs, scales));
    if (rp->metric != KSS_METRIC_PLANE) return set_err(c, KSS_ERR_ARG, (std::string(who) + ": the metric must be KSS_METRIC_PLANE").c_str());
    return KSS_OK;
}
// d_snrm: the source's normals on the device, given or computed; robust: the weights of rp on the symmetric record
static PairMode symm_mode_of(const kss_symm_params* sp, const float* d_snrm, const kss_robust_params* rp, bool robust) {
    PairMode mode = robust ? robust_mode_of(rp) : PairMode();
    mode.plane = true;
    mode.symm = true;
    mode.symm_align = sp->align_normals;
    mode.d_src_nrm = d_snrm;
    return mode;
}

// kss_symm_sums (robust false: rp and info are not read) and kss_symm_robust_sums
static int symm_sums_any(kss_ctx* c, const char* who, bool host, PairClouds P, const int32_t* idx, double max_d2, const float* Rn,
                         const kss_symm_params* sp, const kss_robust_params* rp, bool robust, double* sums, double* info) {
    KCHK(symm_robust_check(c, who, sp, rp, robust, !P.snrm || !P.tnrm));
    KCHK(sums_check(c, who, P, idx, sums, info || !robust));
    KCHK(pair_enter(c, host, P, &idx, who));
    KCHK(pair_normals(c, P, sp->normals_k, true));
    return pair_record_dev(c, P.src, P.tgt, P.tnrm, idx, P.ns, P.nt, max_d2, symm_mode_of(sp, P.snrm, rp, robust), Rn, sums, info);
}
int kss_symm_sums_dev(kss_ctx* c, const float* d_src, const float* d_src_normals, const float* d_tgt, const float* d_tgt_normals,
                      const int32_t* d_idx, int64_t n, int64_t nt, double max_d2, const float Rn[9], const kss_symm_params* sp,
                      double sums[KSS_P2L_NSUMS]) {
    return symm_sums_any(c, "symm_sums", false, one_pair(d_src, n, d_src_normals, d_tgt, nt, d_tgt_normals), d_idx, max_d2, Rn, sp, nullptr, false,
                         sums, nullptr);
}
int kss_symm_sums(kss_ctx* c, const float* src, const float* src_normals, const float* tgt, const float* tgt_normals, const int32_t* idx,
                  int64_t n, int64_t nt, double max_d2, const float Rn[9], const kss_symm_params* sp, double sums[KSS_P2L_NSUMS]) {
    return symm_sums_any(c, "symm_sums", true, one_pair(src, n, src_normals, tgt, nt, tgt_normals), idx, max_d2, Rn, sp, nullptr, false, sums,
                         nullptr);
}
int kss_symm_robust_sums_dev(kss_ctx* c, const float* d_src, const float* d_src_normals, const float* d_tgt, const float* d_tgt_normals,
                             const int32_t* d_idx, int64_t n, int64_t nt, double max_d2, const float Rn[9], const kss_symm_params* sp,
                             const kss_robust_params* rp, double sums[KSS_P2L_NSUMS], double info[KSS_ROBUST_NINFO]) {
    return symm_sums_any(c, "symm_robust_sums", false, one_pair(d_src, n, d_src_normals, d_tgt, nt, d_tgt_normals), d_idx, max_d2, Rn, sp, rp,
                         true, sums, info);
}
int kss_symm_robust_sums(kss_ctx* c, const float* src, const float* src_normals, const float* tgt, const float* tgt_normals,
                         const int32_t* idx, int64_t n, int64_t nt, double max_d2, const float Rn[9], const kss_symm_params* sp,
                         const kss_robust_params* rp, double sums[KSS_P2L_NSUMS], double info[KSS_ROBUST_NINFO]) {
    return symm_sums_any(c, "symm_robust_sums", true, one_pair(src, n, src_normals, tgt, nt, tgt_normals), idx, max_d2, Rn, sp, rp, true, sums,
                         info);
}

// kss_icp_symm[_batch] (robust false: rp, scales and info are not read) and kss_icp_symm_robust[_batch]
static int icp_symm_any(kss_ctx* c, const char* who, bool host, PairClouds P, const kss_icp_params* p, const kss_symm_params* sp,
                        const int32_t* aligns, const kss_robust_params* rp, bool robust, const double* scales, kss_icp_result* res, double* info) {
    KCHK(symm_robust_check(c, who, sp, rp, robust, !P.snrm || !P.tnrm, P.npairs, aligns, scales));
    KCHK(pair_check(c, who, P, p, res, "symmetric ICP"));
    KCHK(pair_enter(c, host, P));
    KCHK(pair_normals(c, P, sp->normals_k, true));
    return pair_go(c, P, p, symm_mode_of(sp, P.snrm, rp, robust), res, info, nullptr, rp, scales, nullptr, aligns);
}
int kss_icp_symm_dev(kss_ctx* c, const float* d_src, int64_t ns, const float* d_src_normals, const float* d_tgt, int64_t nt,
                     const float* d_tgt_normals, const kss_icp_params* p, const kss_symm_params* sp, kss_icp_result* res) {
    return icp_symm_any(c, "icp_symm", false, one_pair(d_src, ns, d_src_normals, d_tgt, nt, d_tgt_normals), p, sp, nullptr, nullptr, false, nullptr,
                        res, nullptr);
}
int kss_icp_symm(kss_ctx* c, const float* src, int64_t ns, const float* src_normals, const float* tgt, int64_t nt, const float* tgt_normals,
                 const kss_icp_params* p, const kss_symm_params* sp, kss_icp_result* res) {
    return icp_symm_any(c, "icp_symm", true, one_pair(src, ns, src_normals, tgt, nt, tgt_normals), p, sp, nullptr, nullptr, false, nullptr, res,
                        nullptr);
}
int kss_icp_symm_batch_dev(kss_ctx* c, const float* d_src, const int64_t* src_off, const float* d_src_normals, const float* d_tgt,
                           const int64_t* tgt_off, const float* d_tgt_normals, int npairs, const kss_icp_params* p,
                           const kss_symm_params* sp, const int32_t* aligns, kss_icp_result* results) {
    return icp_symm_any(c, "icp_symm_batch", false, many_pairs(d_src, src_off, d_src_normals, d_tgt, tgt_off, d_tgt_normals, npairs), p, sp,
                        aligns, nullptr, false, nullptr, results, nullptr);
}
int kss_icp_symm_batch(kss_ctx* c, const float* src, const int64_t* src_off, const float* src_normals, const float* tgt,
                       const int64_t* tgt_off, const float* tgt_normals, int npairs, const kss_icp_params* p, const kss_symm_params* sp,
                       const int32_t* aligns, kss_icp_result* results) {
    return icp_symm_any(c, "icp_symm_batch", true, many_pairs(src, src_off, src_normals, tgt, tgt_off, tgt_normals, npairs), p, sp, aligns,
                        nullptr, false, nullptr, results, nullptr);
}
int kss_icp_symm_robust_dev(kss_ctx* c, const float* d_src, int64_t ns, const float* d_src_normals, const float* d_tgt, int64_t nt,
                            const float* d_tgt_normals, const kss_icp_params* p, const kss_symm_params* sp, const kss_robust_params* rp,
                            kss_icp_result* res, double last_info[KSS_ROBUST_NINFO]) {
    return icp_symm_any(c, "icp_symm_robust", false, one_pair(d_src, ns, d_src_normals, d_tgt, nt, d_tgt_normals), p, sp, nullptr, rp, true,
                        nullptr, res, last_info);
}
int kss_icp_symm_robust(kss_ctx* c, const float* src, int64_t ns, const float* src_normals, const float* tgt, int64_t nt,
                        const float* tgt_normals, const kss_icp_params* p, const kss_symm_params* sp, const kss_robust_params* rp,
                        kss_icp_result* res, double last_info[KSS_ROBUST_NINFO]) {
    return icp_symm_any(c, "icp_symm_robust", true, one_pair(src, ns, src_normals, tgt, nt, tgt_normals), p, sp, nullptr, rp, true, nullptr, res,
                        last_info);
}
int kss_icp_symm_robust_batch_dev(kss_ctx* c, const float* d_src, const int64_t* src_off, const float* d_src_normals, const float* d_tgt,
                                  const int64_t* tgt_off, const float* d_tgt_normals, int npairs, const kss_icp_params* p,
                                  const kss_symm_params* sp, const int32_t* aligns, const kss_robust_params* rp, const double* scales,
                                  kss_icp_result* results, double* info_all) {
    return icp_symm_any(c, "icp_symm_robust_batch", false, many_pairs(d_src, src_off, d_src_normals, d_tgt, tgt_off, d_tgt_normals, npairs), p,
                        sp, aligns, rp, true, scales, results, info_all);
}
int kss_icp_symm_robust_batch(kss_ctx* c, const float* src, const int64_t* src_off, const float* src_normals, const float* tgt,
                              const int64_t* tgt_off, const float* tgt_normals, int npairs, const kss_icp_params* p, const kss_symm_params* sp,
                              const int32_t* aligns, const kss_robust_params* rp, const double* scales, kss_icp_result* results,
                              double* info_all) {
    return icp_symm_any(c, "icp_symm_robust_batch", true, many_pairs(src, src_off, src_normals, tgt, tgt_off, tgt_normals, npairs), p, sp,
                        aligns, rp, true, scales, results, info_all);
}

// ---- one-to-one ICP: the trimmed families' path with PairMode::unique ----------------
int kss_o2o_default_params(kss_o2o_params* op) {
    if (!op) return KSS_ERR_ARG;
    op->overlap = 1.0;
    op->metric = KSS_METRIC_POINT;
    op->trace_o2o = nullptr;
    return KSS_OK;
}

static PairMode o2o_mode_of(const kss_o2o_params* op) {
    PairMode mode = trimmed_mode(op->overlap, op->metric, op->trace_o2o);
    mode.unique = true;
    return mode;
}

int kss_icp_o2o_dev(kss_ctx* c, const float* d_src, int64_t ns, const float* d_tgt, int64_t nt, const float* d_nrm,
                    const kss_icp_params* p, const kss_o2o_params* op, kss_icp_result* res, double last_info[KSS_O2O_NINFO]) {
    KCHK(params_check(c, "icp_o2o", op));
    return icp_trimmed_any(c, "icp_o2o", false, one_pair(d_src, ns, nullptr, d_tgt, nt, d_nrm), p, o2o_mode_of(op), op->metric, nullptr, res,
                           last_info);
}
int kss_icp_o2o(kss_ctx* c, const float* src, int64_t ns, const float* tgt, int64_t nt, const float* nrm,
                const kss_icp_params* p, const kss_o2o_params* op, kss_icp_result* res, double last_info[KSS_O2O_NINFO]) {
    KCHK(params_check(c, "icp_o2o", op));
    return icp_trimmed_any(c, "icp_o2o", true, one_pair(src, ns, nullptr, tgt, nt, nrm), p, o2o_mode_of(op), op->metric, nullptr, res, last_info);
}
int kss_icp_o2o_batch_dev(kss_ctx* c, const float* d_src_all, const int64_t* src_off, const float* d_tgt_all, const int64_t* tgt_off,
                          const float* d_nrm_all, int npairs, const kss_icp_params* p, const kss_o2o_params* op, const double* overlaps,
                          kss_icp_result* results, double* info_all) {
    KCHK(params_check(c, "icp_o2o_batch", op));
    return icp_trimmed_any(c, "icp_o2o_batch", false, many_pairs(d_src_all, src_off, nullptr, d_tgt_all, tgt_off, d_nrm_all, npairs), p,
                           o2o_mode_of(op), op->metric, overlaps, results, info_all);
}
int kss_icp_o2o_batch(kss_ctx* c, const float* src_all, const int64_t* src_off, const float* tgt_all, const int64_t* tgt_off,
                      const float* nrm_all, int npairs, const kss_icp_params* p, const kss_o2o_params* op, const double* overlaps,
                      kss_icp_result* results, double* info_all) {
    KCHK(params_check(c, "icp_o2o_batch", op));
    return icp_trimmed_any(c, "icp_o2o_batch", true, many_pairs(src_all, src_off, nullptr, tgt_all, tgt_off, nrm_all, npairs), p, o2o_mode_of(op),
                           op->metric, overlaps, results, info_all);
}

// the filter alone: the arguments of the four entry points
static int o2o_filter_check(kss_ctx* c, const void* idx, const void* d2, const int64_t* off, const int64_t* nts, int nseg, const double* info) {
    if (!idx || !d2 || !off || !nts || !info) return set_err(c, KSS_ERR_ARG, "o2o_filter: null argument");
    if (nseg <= 0) return set_err(c, KSS_ERR_ARG, "o2o_filter: no segment");
    for (int i = 0; i < nseg; ++i) {
        const int64_t n = off[i + 1] - off[i];
        if (n <= 0 || n > 0x7fff0000ll || nts[i] <= 0 || nts[i] > 0x7fff0000ll) return set_err(c, KSS_ERR_ARG, "o2o_filter: segment or target count empty or out of range");
    }
    if (off[nseg] - off[0] > 0x7fff0000ll) return set_err(c, KSS_ERR_ARG, "o2o_filter: batch too large");
    return KSS_OK;
}

int kss_o2o_filter_batch_dev(kss_ctx* c, const int32_t* d_idx_all, const float* d_d2_all, const int64_t* off, const int64_t* nts, int nseg,
                             double max_d2, int32_t* d_idx_out_all, float* d_d2_out_all, double* info_all) {
    if (!c) return KSS_ERR_ARG;
    KCHK(o2o_filter_check(c, d_idx_all, d_d2_all, off, nts, nseg, info_all));
    return o2o_filter_dev(c, d_idx_all, d_d2_all, off, nts, nseg, max_d2, d_idx_out_all, d_d2_out_all, info_all);
}

int kss_o2o_filter_batch(kss_ctx* c, const int32_t* idx_all, const float* d2_all, const int64_t* off, const int64_t* nts, int nseg,
                         double max_d2, int32_t* idx_out_all, float* d2_out_all, double* info_all) {
    if (!c) return KSS_ERR_ARG;
    KCHK(o2o_filter_check(c, idx_all, d2_all, off, nts, nseg, info_all));
    HIPCHK(c, hipSetDevice(c->device));
    const int64_t o0 = off[0], n = off[nseg] - o0;
    KCHK(upload(c, c->stage_idx, idx_all + o0, (size_t)n * sizeof(int32_t)));
    KCHK(upload(c, c->stage_d2, d2_all + o0, (size_t)n * sizeof(float)));
    std::vector<int64_t> o(nseg + 1);
    for (int i = 0; i <= nseg; ++i) o[i] = off[i] - o0;
    // filtered in place on the staged copies, then back to whichever outputs the caller gave
    KCHK(o2o_filter_dev(c, (const int32_t*)c->stage_idx.p, (const float*)c->stage_d2.p, o.data(), nts, nseg, max_d2,
                        idx_out_all ? (int32_t*)c->stage_idx.p : nullptr, d2_out_all ? (float*)c->stage_d2.p : nullptr, info_all));
    if (idx_out_all) HIPCHK(c, hipMemcpyAsync(idx_out_all + o0, c->stage_idx.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (d2_out_all) HIPCHK(c, hipMemcpyAsync(d2_out_all + o0, c->stage_d2.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return KSS_OK;
}

int kss_o2o_filter_dev(kss_ctx* c, const int32_t* d_idx, const float* d_d2, int64_t n, int64_t nt, double max_d2, int32_t* d_idx_out,
                       float* d_d2_out, double info[2]) {
    const int64_t off[2] = {0, n};
    return kss_o2o_filter_batch_dev(c, d_idx, d_d2, off, &nt, 1, max_d2, d_idx_out, d_d2_out, info);
}

int kss_o2o_filter(kss_ctx* c, const int32_t* idx, const float* d2, int64_t n, int64_t nt, double max_d2, int32_t* idx_out, float* d2_out,
                   double info[2]) {
    const int64_t off[2] = {0, n};
    return kss_o2o_filter_batch(c, idx, d2, off, &nt, 1, max_d2, idx_out, d2_out, info);
}

// ---- reciprocal ICP: the trimmed families' path with PairMode::mutual, one pair and many pairs per call --
int kss_recip_default_params(kss_recip_params* rp) {
    if (!rp) return KSS_ERR_ARG;
    rp->overlap = 1.0;
    rp->metric = KSS_METRIC_POINT;
    rp->trace_recip = nullptr;
    return KSS_OK;
}

static PairMode recip_mode_of(const kss_recip_params* rp) {
    PairMode mode = trimmed_mode(rp->overlap, rp->metric, rp->trace_recip);
    mode.mutual = true;
    return mode;
}

int kss_icp_recip_dev(kss_ctx* c, const float* d_src, int64_t ns, const float* d_tgt, int64_t nt, const float* d_nrm,
                      const kss_icp_params* p, const kss_recip_params* rp, kss_icp_result* res, double last_info[KSS_RECIP_NINFO]) {
    KCHK(params_check(c, "icp_recip", rp));
    return icp_trimmed_any(c, "icp_recip", false, one_pair(d_src, ns, nullptr, d_tgt, nt, d_nrm), p, recip_mode_of(rp), rp->metric, nullptr, res,
                           last_info);
}
int kss_icp_recip(kss_ctx* c, const float* src, int64_t ns, const float* tgt, int64_t nt, const float* nrm,
                  const kss_icp_params* p, const kss_recip_params* rp, kss_icp_result* res, double last_info[KSS_RECIP_NINFO]) {
    KCHK(params_check(c, "icp_recip", rp));
    return icp_trimmed_any(c, "icp_recip", true, one_pair(src, ns, nullptr, tgt, nt, nrm), p, recip_mode_of(rp), rp->metric, nullptr, res,
                           last_info);
}

// the filter alone: the arguments of both entry points
static int recip_filter_check(kss_ctx* c, const void* src, const void* tgt, const void* idx, const void* d2, int64_t n, int64_t nt, const double* info) {
    if (!src || !tgt || !idx || !d2 || !info) return set_err(c, KSS_ERR_ARG, "recip_filter: null argument");
    if (n <= 0 || n > 0x7fff0000ll || nt <= 0 || nt > 0x7fff0000ll) return set_err(c, KSS_ERR_ARG, "recip_filter: source or target count empty or out of range");
    return KSS_OK;
}

int kss_recip_filter_dev(kss_ctx* c, const float* d_src, int64_t n, const float* d_tgt, int64_t nt, const int32_t* d_idx, const float* d_d2,
                         double max_d2, int nn_fma, int32_t* d_idx_out, float* d_d2_out, double info[3]) {
    if (!c) return KSS_ERR_ARG;
    KCHK(recip_filter_check(c, d_src, d_tgt, d_idx, d_d2, n, nt, info));
    const int64_t off[2] = {0, n}, tgt_off[2] = {0, nt};   // (one segment: info_all is the three doubles)
    return recip_filter_dev(c, d_src, off, d_tgt, tgt_off, 1, d_idx, d_d2, max_d2, nn_fma != 0, d_idx_out, d_d2_out, info, true);
}

int kss_recip_filter(kss_ctx* c, const float* src, int64_t n, const float* tgt, int64_t nt, const int32_t* idx, const float* d2, double max_d2,
                     int nn_fma, int32_t* idx_out, float* d2_out, double info[3]) {
    if (!c) return KSS_ERR_ARG;
    KCHK(recip_filter_check(c, src, tgt, idx, d2, n, nt, info));
    HIPCHK(c, hipSetDevice(c->device));
    KCHK(upload(c, c->stage_src, src, (size_t)n * 3 * sizeof(float)));
    KCHK(upload(c, c->stage_tgt, tgt, (size_t)nt * 3 * sizeof(float)));
    KCHK(upload(c, c->stage_idx, idx, (size_t)n * sizeof(int32_t)));
    KCHK(upload(c, c->stage_d2, d2, (size_t)n * sizeof(float)));
    // filtered in place on the staged copies, then back to whichever outputs the caller gave
    const int64_t off[2] = {0, n}, tgt_off[2] = {0, nt};
    KCHK(recip_filter_dev(c, (const float*)c->stage_src.p, off, (const float*)c->stage_tgt.p, tgt_off, 1, (const int32_t*)c->stage_idx.p,
                          (const float*)c->stage_d2.p, max_d2, nn_fma != 0, idx_out ? (int32_t*)c->stage_idx.p : nullptr,
                          d2_out ? (float*)c->stage_d2.p : nullptr, info, true));
    if (idx_out) HIPCHK(c, hipMemcpyAsync(idx_out, c->stage_idx.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (d2_out) HIPCHK(c, hipMemcpyAsync(d2_out, c->stage_d2.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return KSS_OK;
}

// many pairs per call.  The C symbols are spelled _pairs: see include/kssicp.h
int kss_icp_recip_pairs_dev(kss_ctx* c, const float* d_src_all, const int64_t* src_off, const float* d_tgt_all, const int64_t* tgt_off,
                            const float* d_nrm_all, int npairs, const kss_icp_params* p, const kss_recip_params* rp, const double* overlaps,
                            kss_icp_result* results, double* info_all) {
    KCHK(params_check(c, "icp_recip_pairs", rp));
    return icp_trimmed_any(c, "icp_recip_pairs", false, many_pairs(d_src_all, src_off, nullptr, d_tgt_all, tgt_off, d_nrm_all, npairs), p,
                           recip_mode_of(rp), rp->metric, overlaps, results, info_all);
}
int kss_icp_recip_pairs(kss_ctx* c, const float* src_all, const int64_t* src_off, const float* tgt_all, const int64_t* tgt_off,
                        const float* nrm_all, int npairs, const kss_icp_params* p, const kss_recip_params* rp, const double* overlaps,
                        kss_icp_result* results, double* info_all) {
    KCHK(params_check(c, "icp_recip_pairs", rp));
    return icp_trimmed_any(c, "icp_recip_pairs", true, many_pairs(src_all, src_off, nullptr, tgt_all, tgt_off, nrm_all, npairs), p,
                           recip_mode_of(rp), rp->metric, overlaps, results, info_all);
}

// the filter alone for nseg segments: the arguments of both entry points
static int recip_filter_batch_check(kss_ctx* c, const void* src, const int64_t* off, const void* tgt, const int64_t* tgt_off, int nseg,
                                    const void* idx, const void* d2, const double* info) {
    if (!src || !off || !tgt || !tgt_off || !idx || !d2 || !info) return set_err(c, KSS_ERR_ARG, "recip_filter_batch: null argument");
    if (nseg <= 0) return set_err(c, KSS_ERR_ARG, "recip_filter_batch: no segment");
    for (int i = 0; i < nseg; ++i) {
        const int64_t n = off[i + 1] - off[i], nt = tgt_off[i + 1] - tgt_off[i];
        if (n <= 0 || n > 0x7fff0000ll || nt <= 0 || nt > 0x7fff0000ll)
            return set_err(c, KSS_ERR_ARG, "recip_filter_batch: segment or target count empty or out of range");
    }
    if (off[nseg] - off[0] > 0x7fff0000ll || tgt_off[nseg] - tgt_off[0] > 0x7fff0000ll)
        return set_err(c, KSS_ERR_ARG, "recip_filter_batch: batch too large");
    return KSS_OK;
}
// both offset arrays rebased to their first entry
static void recip_filter_rebase(const int64_t* off, const int64_t* tgt_off, int nseg, std::vector<int64_t>& o, std::vector<int64_t>& to) {
    o.resize((size_t)nseg + 1); to.resize((size_t)nseg + 1);
    for (int i = 0; i <= nseg; ++i) { o[i] = off[i] - off[0]; to[i] = tgt_off[i] - tgt_off[0]; }
}

int kss_recip_filter_batch_dev(kss_ctx* c, const float* d_src_all, const int64_t* off, const float* d_tgt_all, const int64_t* tgt_off, int nseg,
                               const int32_t* d_idx_all, const float* d_d2_all, double max_d2, int nn_fma, int32_t* d_idx_out_all,
                               float* d_d2_out_all, double* info_all) {
    if (!c) return KSS_ERR_ARG;
    KCHK(recip_filter_batch_check(c, d_src_all, off, d_tgt_all, tgt_off, nseg, d_idx_all, d_d2_all, info_all));
    std::vector<int64_t> o, to;
    recip_filter_rebase(off, tgt_off, nseg, o, to);
    const int64_t o0 = off[0], t0 = tgt_off[0];
    return recip_filter_dev(c, d_src_all + 3 * o0, o.data(), d_tgt_all + 3 * t0, to.data(), nseg, d_idx_all + o0, d_d2_all + o0, max_d2,
                            nn_fma != 0, d_idx_out_all ? d_idx_out_all + o0 : nullptr, d_d2_out_all ? d_d2_out_all + o0 : nullptr, info_all);
}

int kss_recip_filter_batch(kss_ctx* c, const float* src_all, const int64_t* off, const float* tgt_all, const int64_t* tgt_off, int nseg,
                           const int32_t* idx_all, const float* d2_all, double max_d2, int nn_fma, int32_t* idx_out_all, float* d2_out_all,
                           double* info_all) {
    if (!c) return KSS_ERR_ARG;
    KCHK(recip_filter_batch_check(c, src_all, off, tgt_all, tgt_off, nseg, idx_all, d2_all, info_all));
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<int64_t> o, to;
    recip_filter_rebase(off, tgt_off, nseg, o, to);
    const int64_t o0 = off[0], t0 = tgt_off[0], n = o[nseg], nt = to[nseg];
    KCHK(upload(c, c->stage_src, src_all + 3 * o0, (size_t)n * 3 * sizeof(float)));
    KCHK(upload(c, c->stage_tgt, tgt_all + 3 * t0, (size_t)nt * 3 * sizeof(float)));
    KCHK(upload(c, c->stage_idx, idx_all + o0, (size_t)n * sizeof(int32_t)));
    KCHK(upload(c, c->stage_d2, d2_all + o0, (size_t)n * sizeof(float)));
    // filtered in place on the staged copies, then back to whichever outputs the caller gave
    KCHK(recip_filter_dev(c, (const float*)c->stage_src.p, o.data(), (const float*)c->stage_tgt.p, to.data(), nseg,
                          (const int32_t*)c->stage_idx.p, (const float*)c->stage_d2.p, max_d2, nn_fma != 0,
                          idx_out_all ? (int32_t*)c->stage_idx.p : nullptr, d2_out_all ? (float*)c->stage_d2.p : nullptr, info_all));
    if (idx_out_all) HIPCHK(c, hipMemcpyAsync(idx_out_all + o0, c->stage_idx.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (d2_out_all) HIPCHK(c, hipMemcpyAsync(d2_out_all + o0, c->stage_d2.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return KSS_OK;
}

static int trim_batch_check(kss_ctx* c, const float* d2, const int64_t* off, int nseg, const double* overlaps, const double* info_all) {
    if (!d2 || !off || !overlaps || !info_all) return set_err(c, KSS_ERR_ARG, "trim_threshold_batch: null argument");
    if (nseg <= 0) return set_err(c, KSS_ERR_ARG, "trim_threshold_batch: no segment");
    for (int i = 0; i < nseg; ++i) {
        const int64_t n = off[i + 1] - off[i];
        if (n <= 0 || n > 0x7fff0000ll) return set_err(c, KSS_ERR_ARG, "trim_threshold_batch: segment empty or out of range");
        if (!trim_overlap_ok(overlaps[i])) return set_err(c, KSS_ERR_ARG, "trim_threshold_batch: overlap must be in (0, 1]");
    }
    return KSS_OK;
}

int kss_trim_threshold_batch_dev(kss_ctx* c, const float* d_d2_all, const int64_t* off, int nseg, double max_d2, const double* overlaps,
                                 double* info_all) {
    if (!c) return KSS_ERR_ARG;
    KCHK(trim_batch_check(c, d_d2_all, off, nseg, overlaps, info_all));
    return trim_threshold_batch_dev(c, d_d2_all, off, nseg, max_d2, overlaps, info_all);
}

int kss_trim_threshold_batch(kss_ctx* c, const float* d2_all, const int64_t* off, int nseg, double max_d2, const double* overlaps,
                             double* info_all) {
    if (!c) return KSS_ERR_ARG;
    KCHK(trim_batch_check(c, d2_all, off, nseg, overlaps, info_all));
    HIPCHK(c, hipSetDevice(c->device));
    KCHK(upload(c, c->stage_d2, d2_all + off[0], (size_t)(off[nseg] - off[0]) * sizeof(float)));
    std::vector<int64_t> o(nseg + 1);
    for (int i = 0; i <= nseg; ++i) o[i] = off[i] - off[0];
    return trim_threshold_batch_dev(c, (const float*)c->stage_d2.p, o.data(), nseg, max_d2, overlaps, info_all);
}

// ---- pre-shape ------------------------------------------------------------------------------------
// Both clouds of a registration in one call: two launches (sum + centroid, radius + publication), no stream
// synchronisation -- the host spins on the {value, sequence number} slots the second launch writes.

int kss_preshape_stats_pair_dev(kss_ctx* c, const void* d_src, int64_t ns, const void* d_tgt, int64_t nt, int dtype,
                                double c_src[3], double* r_src, double c_tgt[3], double* r_tgt) {
    if (!c || !d_src || !c_src || !r_src) return set_err(c, KSS_ERR_ARG, "preshape: null argument");
    if (d_tgt && (!c_tgt || !r_tgt)) return set_err(c, KSS_ERR_ARG, "preshape: null argument");
    if (ns <= 0 || (d_tgt && nt <= 0)) return set_err(c, KSS_ERR_ARG, "preshape: empty cloud");
    if (dtype != KSS_F32 && dtype != KSS_F64) return set_err(c, KSS_ERR_ARG, "preshape: bad dtype");
    HIPCHK(c, hipSetDevice(c->device));
    const void* xyz[2] = {d_src, d_tgt};
    const int64_t n[2] = {ns, d_tgt ? nt : 0};
    const int nb = preshape_blocks(ns) + (d_tgt ? preshape_blocks(nt) : 0);
    KCHK(ensure_zeroed(c, c->pre_partials, (size_t)nb * 4 * sizeof(Granule)));   // (zeroed when (re)allocated: no granule of an earlier owner)
    KCHK(ensure_zeroed(c, c->pre_state, 8 * sizeof(double)));   // the two centroids, each with the number of the launch that stored it
    KCHK(ensure_pub_slots(c));
    {
        ProfScope ps(c, KSS_K_PRESHAPE);
        const unsigned long long seq_sum = ++c->seq;   // (each launch hands its rows over under a number of its own)
        const unsigned long long seq = ++c->seq;
        launch_preshape_pair(c->stream, xyz, n, dtype, (Granule*)c->pre_partials.p, (double*)c->pre_state.p, c->h_seq_dev, seq_sum, seq);
    }
    HIPCHK(c, hipGetLastError());
    double h[8];
    KCHK(wait_slots(c, d_tgt ? 8 : 4, h));
    c_src[0] = h[0]; c_src[1] = h[1]; c_src[2] = h[2];
    *r_src = h[3] / (double)ns;
    if (d_tgt) {
        c_tgt[0] = h[4]; c_tgt[1] = h[5]; c_tgt[2] = h[6];
        *r_tgt = h[7] / (double)nt;
    }
    return KSS_OK;
}

int kss_preshape_stats_dev(kss_ctx* c, const void* d_xyz, int dtype, int64_t n, double centroid[3], double* mean_radius) {
    if (!c || !d_xyz || !centroid || !mean_radius) return set_err(c, KSS_ERR_ARG, "preshape: null argument");
    return kss_preshape_stats_pair_dev(c, d_xyz, n, nullptr, 0, dtype, centroid, mean_radius, nullptr, nullptr);
}

int kss_preshape_stats(kss_ctx* c, const void* xyz, int dtype, int64_t n, double centroid[3], double* mean_radius) {
    if (!c || !xyz) return set_err(c, KSS_ERR_ARG, "preshape: null argument");
    if (n <= 0) return set_err(c, KSS_ERR_ARG, "preshape: empty cloud");
    if (dtype != KSS_F32 && dtype != KSS_F64) return set_err(c, KSS_ERR_ARG, "preshape: bad dtype");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t esz = dtype == KSS_F64 ? 8 : 4;
    KCHK(upload(c, c->stage_src, xyz, (size_t)n * 3 * esz));
    return kss_preshape_stats_dev(c, c->stage_src.p, dtype, n, centroid, mean_radius);
}

// ---- pose / transform application -------------------------------------------------------------------
int kss_pose_apply_dev(kss_ctx* c, const double* d_in, int64_t n, const kss_pose* pose, double* d_out) {
    if (!c || !d_in || !d_out || !pose) return set_err(c, KSS_ERR_ARG, "pose_apply: null argument");
    if (n < 0) return set_err(c, KSS_ERR_ARG, "pose_apply: negative size");
    if (n == 0) return KSS_OK;
    HIPCHK(c, hipSetDevice(c->device));
    // cos/sin evaluated on the host so that they are the caller's libm values (reference: cos(angle) per point)
    const double cs[6] = {std::cos(pose->angle[0]), std::sin(pose->angle[0]), std::cos(pose->angle[1]),
                          std::sin(pose->angle[1]), std::cos(pose->angle[2]), std::sin(pose->angle[2])};
    {
        ProfScope ps(c, KSS_K_POSE_APPLY);
        launch_pose_apply(c->stream, d_in, n, *pose, cs, d_out);
    }
    HIPCHK(c, hipGetLastError());
    return KSS_OK;
}

int kss_pose_apply(kss_ctx* c, const double* in, int64_t n, const kss_pose* pose, double* out) {
    if (!c || !in || !out || !pose) return set_err(c, KSS_ERR_ARG, "pose_apply: null argument");
    if (n < 0) return set_err(c, KSS_ERR_ARG, "pose_apply: negative size");
    if (n == 0) return KSS_OK;
    HIPCHK(c, hipSetDevice(c->device));
    KCHK(upload(c, c->stage_src, in, (size_t)n * 3 * sizeof(double)));
    KCHK(ensure(c, c->stage_out, (size_t)n * 3 * sizeof(double)));
    KCHK(kss_pose_apply_dev(c, (const double*)c->stage_src.p, n, pose, (double*)c->stage_out.p));
    HIPCHK(c, hipMemcpyAsync(out, c->stage_out.p, (size_t)n * 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return KSS_OK;
}

int kss_transform_apply_dev(kss_ctx* c, const float T[16], const double* d_in, int64_t n, double* d_out) {
    if (!c || !T || !d_in || !d_out) return set_err(c, KSS_ERR_ARG, "transform_apply: null argument");
    if (n < 0) return set_err(c, KSS_ERR_ARG, "transform_apply: negative size");
    if (n == 0) return KSS_OK;
    HIPCHK(c, hipSetDevice(c->device));
    {
        ProfScope ps(c, KSS_K_POSE_APPLY);
        launch_transform_apply_f64(c->stream, T, d_in, n, d_out);
    }
    HIPCHK(c, hipGetLastError());
    return KSS_OK;
}

int kss_transform_apply(kss_ctx* c, const float T[16], const double* in, int64_t n, double* out) {
    if (!c || !T || !in || !out) return set_err(c, KSS_ERR_ARG, "transform_apply: null argument");
    if (n < 0) return set_err(c, KSS_ERR_ARG, "transform_apply: negative size");
    if (n == 0) return KSS_OK;
    HIPCHK(c, hipSetDevice(c->device));
    KCHK(upload(c, c->stage_src, in, (size_t)n * 3 * sizeof(double)));
    KCHK(ensure(c, c->stage_out, (size_t)n * 3 * sizeof(double)));
    KCHK(kss_transform_apply_dev(c, T, (const double*)c->stage_src.p, n, (double*)c->stage_out.p));
    HIPCHK(c, hipMemcpyAsync(out, c->stage_out.p, (size_t)n * 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return KSS_OK;
}

int kss_transform_apply_f32(kss_ctx* c, const float T[16], const float* in, int64_t n, float* out) {
    if (!c || !T || !in || !out) return set_err(c, KSS_ERR_ARG, "transform_apply_f32: null argument");
    if (n < 0) return set_err(c, KSS_ERR_ARG, "transform_apply_f32: negative size");
    if (n == 0) return KSS_OK;
    HIPCHK(c, hipSetDevice(c->device));
    KCHK(upload(c, c->stage_src, in, (size_t)n * 3 * sizeof(float)));
    KCHK(ensure(c, c->stage_out, (size_t)n * 3 * sizeof(float)));
    {
        ProfScope ps(c, KSS_K_POSE_APPLY);
        launch_transform_apply_f32(c->stream, T, (const float*)c->stage_src.p, n, (float*)c->stage_out.p);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out, c->stage_out.p, (size_t)n * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return KSS_OK;
}

int kss_downsample_fps(kss_ctx* c, const double* xyz, int64_t n, int64_t m, double* out, int32_t* out_idx) {
    if (!c || !xyz || !out) return set_err(c, KSS_ERR_ARG, "downsample_fps: null argument");
    if (n <= 0 || m <= 0 || m > n || n > 0x7fff0000ll) return set_err(c, KSS_ERR_ARG, "downsample_fps: need 0 < m <= n");
    HIPCHK(c, hipSetDevice(c->device));
    KCHK(upload(c, c->scratch_a, xyz, (size_t)n * 3 * sizeof(double)));
    KCHK(ensure(c, c->scratch_b, (size_t)n * sizeof(double)));
    KCHK(ensure(c, c->stage_idx, (size_t)m * sizeof(int32_t)));
    KCHK(ensure(c, c->stage_out, (size_t)m * 3 * sizeof(double)));
    launch_fps(c->stream, (const double*)c->scratch_a.p, (int)n, (int)m, (double*)c->scratch_b.p, (int32_t*)c->stage_idx.p, (double*)c->stage_out.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out, c->stage_out.p, (size_t)m * 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (out_idx) HIPCHK(c, hipMemcpyAsync(out_idx, c->stage_idx.p, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return KSS_OK;
}

int kss_downsample_aivs(kss_ctx* c, const double* xyz, int64_t n, int64_t point_num, double* out, int64_t capacity,
                        int64_t* n_out, int32_t* out_idx) {
    if (!c || !xyz || !out || !n_out) return set_err(c, KSS_ERR_ARG, "downsample_aivs: null argument");
    if (n <= 0 || point_num <= 0 || n > 0x7fff0000ll) return set_err(c, KSS_ERR_ARG, "downsample_aivs: bad sizes");
    HIPCHK(c, hipSetDevice(c->device));
    KCHK(upload(c, c->scratch_a, xyz, (size_t)n * 3 * sizeof(double)));
    std::vector<int32_t> sel;
    std::string err;
    auto scratch = [c](size_t bytes) -> void* { return ensure(c, c->scratch_b, bytes) == KSS_OK ? c->scratch_b.p : nullptr; };
    const int rc = aivs_device(c->stream, (const double*)c->scratch_a.p, (int)n, (int)std::min<int64_t>(point_num, 0x7fffffff), sel, err, scratch);
    if (rc != KSS_OK) return set_err(c, rc, err.c_str());
    *n_out = (int64_t)sel.size();
    if ((int64_t)sel.size() > capacity) return set_err(c, KSS_ERR_CAPACITY, "downsample_aivs: output buffer too small");
    for (size_t i = 0; i < sel.size(); ++i) {
        const int32_t s = sel[i];
        out[3 * i] = xyz[3 * (size_t)s]; out[3 * i + 1] = xyz[3 * (size_t)s + 1]; out[3 * i + 2] = xyz[3 * (size_t)s + 2];
        if (out_idx) out_idx[i] = s;
    }
    return KSS_OK;
}

int kss_downsample_aivs_pair(kss_ctx* c, const double* xyz0, int64_t n0, int64_t point_num0, double* out0, int64_t capacity0, int64_t* n_out0,
                             int32_t* out_idx0, const double* xyz1, int64_t n1, int64_t point_num1, double* out1, int64_t capacity1,
                             int64_t* n_out1, int32_t* out_idx1, int rc[2]) {
    if (!c || !rc) return set_err(c, KSS_ERR_ARG, "downsample_aivs_pair: null argument");
    HIPCHK(c, hipSetDevice(c->device));
    if (c->workers.empty()) {   // (worker contexts live as long as the parent: kss_register_batch shares them)
        kss_ctx* w = nullptr;
        const int wrc = kss_ctx_create(c->device, &w);
        if (wrc != KSS_OK) return set_err(c, wrc, "downsample_aivs_pair: cannot create a worker context");
        w->nn_mode = c->nn_mode;
        c->workers.push_back(w);
    }
    kss_ctx* w = c->workers[0];
    rc[0] = rc[1] = KSS_OK;
    // (a thread of its own: ~50 us per call; the context's pool -- woken through a condition variable -- was measured at 1.9 ms per pair of clouds against 0.65)
    std::thread other([&] { hipSetDevice(w->device); rc[1] = kss_downsample_aivs(w, xyz1, n1, point_num1, out1, capacity1, n_out1, out_idx1); });
    rc[0] = kss_downsample_aivs(c, xyz0, n0, point_num0, out0, capacity0, n_out0, out_idx0);
    other.join();
    if (rc[1] != KSS_OK && rc[0] == KSS_OK) c->err = w->err;   // (kss_last_error(ctx) then speaks of the cloud that failed)
    return KSS_OK;
}

// ---- octree down-sampler (Method_Octree.hpp:77-165) ----------------------------------------------------
int kss_downsample_octree(kss_ctx* c, const double* xyz, int64_t n, int32_t* out_idx, int64_t capacity, int64_t* n_out,
                          double* resolution_out) {
    if (!c || !xyz || !out_idx || !n_out) return set_err(c, KSS_ERR_ARG, "downsample_octree: null argument");
    if (n < 1000 || n > 0x7fff0000ll) return set_err(c, KSS_ERR_ARG, "downsample_octree: needs 1000 <= n < 2^31 points (the reference reads the first 1000 unconditionally)");
    HIPCHK(c, hipSetDevice(c->device));
    // the float cloud (cloud_i.x = pData[i][0]) on the host (box replay) and on the device
    std::vector<float> pf((size_t)n * 3);
    for (size_t i = 0; i < pf.size(); ++i) pf[i] = (float)xyz[i];
    KCHK(upload(c, c->oct_pts, pf.data(), pf.size() * sizeof(float)));
    // PCL_Octree_Resolution (:151-165) -> PCL_Octree_Estimate_Radius (:110-149): first 1000 points, kn-th neighbour
    int kn;
    if (n < 80000) kn = 2;
    else { const int md = (int)(n / 80000); kn = md >= 5 ? 35 : 7 * md; }
    KCHK(ensure(c, c->stage_idx, (size_t)1000 * kn * sizeof(int32_t)));
    KCHK(ensure(c, c->stage_d2, (size_t)1000 * kn * sizeof(float)));
    KCHK(knn_generic_dev(c, c->oct_pts.p, 1000, c->oct_pts.p, n, KSS_F32, kn, (int32_t*)c->stage_idx.p, (float*)c->stage_d2.p));
    std::vector<float> kd((size_t)1000 * kn);
    HIPCHK(c, hipMemcpyAsync(kd.data(), c->stage_d2.p, kd.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    double radiusSum = 0;
    for (int i = 0; i < 1000; ++i) radiusSum = radiusSum + (double)sqrtf(kd[(size_t)i * kn + kn - 1]);   // :141 float sqrt, widened
    radiusSum = radiusSum / 1000;
    const float resolution = (float)radiusSum;
    if (resolution_out) *resolution_out = (double)resolution;
    if (!(resolution > 0.f)) return set_err(c, KSS_ERR_ARG, "downsample_octree: zero resolution (coincident points)");
    // addPointsFromInputCloud: PCL's bounding cube, grown in insertion order
    OctBox box;
    std::memset(&box, 0, sizeof box);
    box.res = (double)resolution;
    oct_first_point(box, pf.data());
    for (int64_t i = 0; i < n; ++i)
        if (!oct_adopt(box, pf.data() + 3 * i)) return set_err(c, KSS_ERR_ARG, "downsample_octree: octree deeper than 21 levels");
    // occupied voxels in depth-first order -> centres
    KCHK(ensure(c, c->oct_cen, (size_t)n * 3 * sizeof(float)));
    std::string err;
    DevBuf* bufs[4] = {&c->oct_a, &c->oct_b, &c->scratch_c, &c->oct_tmp};
    auto scratch = [c, &bufs](int which, size_t bytes) -> void* { return ensure(c, *bufs[which], bytes) == KSS_OK ? bufs[which]->p : nullptr; };
    int m = 0;
    const int rc = octree_voxels_device(c->stream, (const float*)c->oct_pts.p, (int)n, box, (float*)c->oct_cen.p, &m, err, scratch);
    if (rc != KSS_OK) return set_err(c, rc, err.c_str());
    *n_out = m;
    if (m > capacity) return set_err(c, KSS_ERR_CAPACITY, "downsample_octree: output buffer too small");
    // octree.nearestKSearch(centre, 1): the exact NN engine (ties -> lowest index)
    KCHK(ensure(c, c->stage_idx, (size_t)m * sizeof(int32_t)));
    KCHK(ensure(c, c->stage_d2, (size_t)m * sizeof(float)));
    KCHK(kss_nn_dev(c, (const float*)c->oct_cen.p, m, (const float*)c->oct_pts.p, n, (int32_t*)c->stage_idx.p, (float*)c->stage_d2.p));
    HIPCHK(c, hipMemcpyAsync(out_idx, c->stage_idx.p, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return KSS_OK;
}

// ---- rotation search --------------------------------------------------------------------------------
int kss_grid_angles(double step, double* angles, int capacity) {
    if (!angles || capacity <= 0 || !(step > 0)) return KSS_ERR_ARG;
    const int g = grid_angles(step, angles, capacity);
    return g < 0 ? KSS_ERR_CAPACITY : g;
}

int kss_rotation_candidates(const double* err, int g, double step, double best_angle[3], double* angle_list,
                            int list_capacity, int* n_list) {
    if (!err || g <= 0 || !best_angle || !n_list || !(step > 0)) return KSS_ERR_ARG;
    std::vector<double> ang(g);
    if (grid_angles(step, ang.data(), g) != g) return KSS_ERR_ARG;
    // global arg-min, strict '<' against errorT = 9999 in i, j, k loop order (:239, :258-265)
    double errorT = 9999;
    double bi = 0, bj = 0, bk = 0;
    for (int i = 0; i < g; ++i)
        for (int j = 0; j < g; ++j)
            for (int k = 0; k < g; ++k) {
                const double e = err[((int64_t)i * g + j) * g + k];
                if (e < errorT) { errorT = e; bi = ang[i]; bj = ang[j]; bk = ang[k]; }
            }
    best_angle[0] = bi; best_angle[1] = bj; best_angle[2] = bk;
    int nl = 0;
    for (int i = 0; i < g; ++i)
        for (int j = 0; j < g; ++j)
            for (int k = 0; k < g; ++k)
                if (is_local_min(err, g, i, j, k, 2)) {
                    if (angle_list) {
                        if (nl >= list_capacity) return KSS_ERR_CAPACITY;
                        angle_list[3 * nl + 0] = (double)i * 6.3 / step;   // :282-284
                        angle_list[3 * nl + 1] = (double)j * 6.3 / step;
                        angle_list[3 * nl + 2] = (double)k * 6.3 / step;
                    }
                    ++nl;
                }
    *n_list = nl;
    return KSS_OK;
}

int kss_rotation_search_dev(kss_ctx* c, const double* d_src, int64_t ns, const double* d_tgt, int64_t nt, double step,
                            double* err, int64_t err_capacity, int* g_out) {
    if (!c || !d_src || !d_tgt || !err || !g_out) return set_err(c, KSS_ERR_ARG, "rotation_search: null argument");
    if (ns <= 0 || nt <= 0 || !(step > 0)) return set_err(c, KSS_ERR_ARG, "rotation_search: empty cloud or bad step");
    if (ns > 0x7fff0000ll || nt > 0x7fff0000ll) return set_err(c, KSS_ERR_ARG, "rotation_search: cloud too large");
    HIPCHK(c, hipSetDevice(c->device));
    double ang[64];
    const int g = grid_angles(step, ang, 40);
    if (g <= 0) return set_err(c, KSS_ERR_ARG, "rotation_search: grid larger than 40 per axis");
    const int64_t ncand = (int64_t)g * g * g;
    if (err_capacity < ncand) return set_err(c, KSS_ERR_CAPACITY, "rotation_search: err buffer too small");
    std::vector<double> cs(2 * g);
    for (int a = 0; a < g; ++a) { cs[2 * a] = std::cos(ang[a]); cs[2 * a + 1] = std::sin(ang[a]); }
    const int64_t nt_pad = (nt + NN_TILE - 1) / NN_TILE * NN_TILE;
    const int nth = rot_search_grain(ns, nt, g);
    const int nsb = (int)((ns + nth - 1) / nth);
    const int64_t nt_sweep = (nt + nth - 1) / nth * nth;   // what the search sweeps (<= nt_pad: the rest of the padding is never read)
    KCHK(ensure(c, c->tgt4, (size_t)nt_pad * sizeof(float4)));
    KCHK(ensure(c, c->cs, cs.size() * sizeof(double)));
    KCHK(ensure(c, c->partials, (size_t)ncand * nsb * sizeof(double)));
    KCHK(ensure(c, c->scratch_c, (size_t)ncand * sizeof(double)));
    HIPCHK(c, hipMemcpyAsync(c->cs.p, cs.data(), cs.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    launch_pack_f64_to_f4(c->stream, d_tgt, nt, (float4*)c->tgt4.p, nt_pad, true);   // :232-234 narrowing to PointXYZ
    {
        ProfScope ps(c, KSS_K_ROT_SEARCH);
        launch_rot_search(c->stream, d_src, ns, (const float4*)c->tgt4.p, nt_sweep, (const double*)c->cs.p, g,
                          (double*)c->partials.p, nsb, nth);
        launch_row_sums(c->stream, (const double*)c->partials.p, (int)ncand, nsb, 1.0, (double*)c->scratch_c.p);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(err, c->scratch_c.p, (size_t)ncand * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int64_t i = 0; i < ncand; ++i) err[i] = err[i] / (double)ns;   // :448 distanceSum / size
    *g_out = g;
    return KSS_OK;
}

int kss_rotation_search(kss_ctx* c, const double* src, int64_t ns, const double* tgt, int64_t nt, double step,
                        double* err, int64_t err_capacity, int* g_out) {
    if (!c || !src || !tgt) return set_err(c, KSS_ERR_ARG, "rotation_search: null argument");
    if (ns <= 0 || nt <= 0) return set_err(c, KSS_ERR_ARG, "rotation_search: empty cloud");
    HIPCHK(c, hipSetDevice(c->device));
    KCHK(upload(c, c->scratch_a, src, (size_t)ns * 3 * sizeof(double)));
    KCHK(upload(c, c->scratch_b, tgt, (size_t)nt * 3 * sizeof(double)));
    return kss_rotation_search_dev(c, (const double*)c->scratch_a.p, ns, (const double*)c->scratch_b.p, nt, step, err, err_capacity, g_out);
}

// ---- PCR_QM -------------------------------------------------------------------------------------------
int kss_pcr_qm(kss_ctx* c, const double* aligned, int64_t na, const double* tmpl, int64_t nt, double out[3]) {
    if (!c || !aligned || !tmpl || !out) return set_err(c, KSS_ERR_ARG, "pcr_qm: null argument");
    if (na <= 0 || nt <= 0) return set_err(c, KSS_ERR_ARG, "pcr_qm: empty cloud");
    HIPCHK(c, hipSetDevice(c->device));
    KCHK(upload(c, c->scratch_a, aligned, (size_t)na * 3 * sizeof(double)));
    KCHK(upload(c, c->scratch_b, tmpl, (size_t)nt * 3 * sizeof(double)));
    double sums[NSUMS];
    KCHK(nn_generic_dev(c, c->scratch_a.p, na, c->scratch_b.p, nt, KSS_F64, nullptr, nullptr, sums));
    const double mse = sums[17] / (double)na;      // registrationMeasure.hpp:85
    out[0] = mse;
    out[1] = std::sqrt(mse);                        // :87
    out[2] = sums[18] / (double)na;                 // :86
    return KSS_OK;
}

// ---- KSSICP_Registration on down-sampled clouds ----------------------------------------------------------
int kss_register(kss_ctx* c, const double* src_sub, int64_t nss, const double* tgt_sub, int64_t nts,
                 const double* src_full, int64_t nsf, double accurate, int iter, double* point_align,
                 kss_register_result* res) {
    if (!c || !src_sub || !tgt_sub || !res) return set_err(c, KSS_ERR_ARG, "register: null argument");
    if (nss <= 0 || nts <= 0 || nsf < 0 || (nsf > 0 && !src_full)) return set_err(c, KSS_ERR_ARG, "register: bad sizes");
    HIPCHK(c, hipSetDevice(c->device));
    std::memset(res, 0, sizeof *res);
    const bool reg_timing = getenv("KSS_TIMING") != nullptr;   // phase report on stderr (wall clock; the phases that enqueue only are charged to the next one that waits)
    auto t_prev = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {
        if (!reg_timing) return;
        const auto now = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[kss] register: %-34s %8.1f us\n", what, std::chrono::duration<double, std::micro>(now - t_prev).count());
        t_prev = now;
    };
    // resident copies of S', T' (f64) in the context's grow-only workspace (no hipMalloc / hipFree per registration:
    // each costs tens of microseconds and hipFree synchronises the device)
    DevBuf &dS = c->reg_s, &dT = c->reg_t, &dP = c->reg_p, &dAll = c->reg_all;
#define RCHK(expr) do { int rc_ = (expr); if (rc_ != KSS_OK) return rc_; } while (0)
    RCHK(upload(c, dS, src_sub, (size_t)nss * 3 * sizeof(double)));
    RCHK(upload(c, dT, tgt_sub, (size_t)nts * 3 * sizeof(double)));
    RCHK(ensure(c, dP, (size_t)nss * 3 * sizeof(double)));
    lap("uploads");
    // (a2) pre-shape
    double cS[3], cT[3], rS, rT;
    RCHK(kss_preshape_stats_pair_dev(c, dS.p, nss, dT.p, nts, KSS_F64, cS, &rS, cT, &rT));
    kss_pose pose;
    for (int k = 0; k < 3; ++k) { pose.shift[k] = cT[k] - cS[k]; pose.center[k] = cT[k]; pose.angle[k] = 0.0; }
    pose.scale = rT / rS;
    res->scale = pose.scale;
    for (int k = 0; k < 3; ++k) { res->c_src[k] = cS[k]; res->c_tgt[k] = cT[k]; }
    RCHK(kss_pose_apply_dev(c, (const double*)dS.p, nss, &pose, (double*)dP.p));   // S' (angle 0 -> exact identity rotation)
    lap("pre-shape statistics + pose");
    // (a4) rotation search
    std::vector<double> err(40 * 40 * 40);
    int g = 0;
    RCHK(kss_rotation_search_dev(c, (const double*)dP.p, nss, (const double*)dT.p, nts, accurate, err.data(), (int64_t)err.size(), &g));
    res->grid = g;
    lap("rotation search");
    std::vector<double> alist((size_t)3 * g * g * g);
    double best[3];
    int nl = 0;
    RCHK(kss_rotation_candidates(err.data(), g, accurate, best, alist.data(), g * g * g, &nl));
    res->n_angle_list = nl;
    lap("candidate list (host)");

    kss_icp_params ip;
    kss_icp_default_params(&ip);
    ip.max_iterations = iter;
    const int64_t to[2] = {0, nts};
    double chosen[3] = {best[0], best[1], best[2]};
    kss_icp_result r0, rfinal;
    std::vector<kss_icp_result> rr;
    bool have_judge = false, have_cands = false;
    // The judge ICP (from the best grid pose, KSS_ICP.hpp:92-93) and the candidate ICPs of the angle list (:102-118) do not
    // depend on each other -- only whether the candidates' results are USED depends on the judge's fitness (:99).  They run as
    // ONE batch sharing the target, the judge as its last pair; when the judge ends at or below the threshold the candidates
    // are told to stop where they are (the reference would not have run them; nothing of theirs is used).  Each pair is an
    // independent registration: the results equal those of the sequential calls.  KSS_REGISTER_SPEC=0, or an engine that
    // cannot cancel (no large BAR, a batch that does not fit the device at once): the sequential route below.
    static const bool want_spec = getenv("KSS_REGISTER_SPEC") == nullptr || atoi(getenv("KSS_REGISTER_SPEC")) != 0;
    auto fill_poses = [&](int n_list, bool with_judge) -> int {   // every candidate pose of S (and the judge's) in one launch
        const int count = n_list + (with_judge ? 1 : 0);
        RCHK(ensure(c, dAll, (size_t)count * nss * 3 * sizeof(double)));
        std::vector<double> cs((size_t)count * 6);
        for (int i = 0; i < count; ++i) {
            const double* ang = i < n_list ? &alist[3 * i] : best;
            // cos/sin evaluated on the host so that they are the caller's libm values (as kss_pose_apply_dev)
            for (int k = 0; k < 3; ++k) { cs[6 * i + 2 * k] = std::cos(ang[k]); cs[6 * i + 2 * k + 1] = std::sin(ang[k]); }
        }
        {
            ProfScope ps(c, KSS_K_POSE_APPLY);
            launch_pose_apply_many(c->stream, (const double*)dS.p, nss, pose, reinterpret_cast<const double (*)[6]>(cs.data()), count, (double*)dAll.p);
        }
        HIPCHK(c, hipGetLastError());
        return KSS_OK;
    };
    if (want_spec && nl > 0) {
        RCHK(fill_poses(nl, true));
        lap("candidate poses (enqueue)");
        std::vector<int64_t> so(nl + 2);
        for (int i = 0; i <= nl + 1; ++i) so[i] = (int64_t)i * nss;
        rr.resize(nl + 1);
        c->spec_judge = nl; c->spec_threshold = 0.0005; c->spec_ran = false; c->spec_cancelled = false;
        const int rc = icp_run_dev(c, dAll.p, so.data(), dT.p, to, nl + 1, true, KSS_F64, &ip, rr.data());
        c->spec_judge = -1;
        if (rc != KSS_OK) return rc;
        if (c->spec_ran) {
            r0 = rr[nl];
            have_judge = true;
            have_cands = !c->spec_cancelled;
        }
    }
    if (!have_judge) {
        // (a14) judge: ICP from the best grid pose (KSS_ICP.hpp:92-93)
        for (int k = 0; k < 3; ++k) pose.angle[k] = best[k];
        RCHK(kss_pose_apply_dev(c, (const double*)dS.p, nss, &pose, (double*)dP.p));
        const int64_t so[2] = {0, nss};
        RCHK(icp_run_dev(c, dP.p, so, dT.p, to, 1, false, KSS_F64, &ip, &r0));
    }
    res->E_d_init = r0.fitness;
    rfinal = r0;
    // the judge ICP *is* the final ICP when the threshold branch is not taken (same inputs, :93 vs :130)
    if (res->E_d_init > 0.0005 && nl > 0) {   // :99
        // (a14) all candidate ICPs as ONE batch sharing the target (:102-118)
        if (!have_cands) {
            RCHK(fill_poses(nl, false));
            std::vector<int64_t> so(nl + 1);
            for (int i = 0; i <= nl; ++i) so[i] = (int64_t)i * nss;
            rr.resize(nl);
            RCHK(icp_run_dev(c, dAll.p, so.data(), dT.p, to, nl, true, KSS_F64, &ip, rr.data()));
        }
        if (getenv("KSS_DEBUG_CANDS")) {   // every candidate's record (a diagnostic of run-to-run differences)
            char head[64]; std::snprintf(head, sizeof head, "[kss] ctx %p candidates:", (void*)c);
            std::string line = head;
            char buf[96];
            for (int i = 0; i < nl; ++i) { std::snprintf(buf, sizeof buf, " %d:(%d,%d,%.17g)", i, rr[i].iterations, rr[i].state, rr[i].fitness); line += buf; }
            std::fprintf(stderr, "%s | judge (%d,%d,%.17g) spec %d\n", line.c_str(), r0.iterations, r0.state, r0.fitness, have_cands ? 1 : 0);
        }
        double Q = 9999; int angleIndex = 0;
        for (int i = 0; i < nl; ++i) {
            const double ri = rr[i].fitness;
            if (ri < Q && ri >= 0) { Q = ri; angleIndex = i; }   // :113-116
        }
        res->used_angle_list = 1; res->angle_index = angleIndex;
        for (int k = 0; k < 3; ++k) chosen[k] = alist[3 * angleIndex + k];
        rfinal = rr[angleIndex];   // identical inputs => identical to re-running :130
    } else if (res->E_d_init > 0.0005) {
        res->used_angle_list = 1;  // empty angle list: the reference would index out of range; keep the best grid pose
    }
    lap("judge + candidate ICPs");
    for (int k = 0; k < 3; ++k) res->angle[k] = chosen[k];
    res->final_fitness = rfinal.fitness;
    res->icp_iterations = rfinal.iterations;
    res->icp_converged = rfinal.converged;
    std::memcpy(res->T_icp, rfinal.T, sizeof rfinal.T);
    // composite similarity: R = R_icp R0, t = R (c_T - s c_S) + t_icp
    double R0[9];
    euler_matrix(chosen, R0);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            res->R[3 * i + j] = (double)rfinal.T[4 * i] * R0[j] + (double)rfinal.T[4 * i + 1] * R0[3 + j] + (double)rfinal.T[4 * i + 2] * R0[6 + j];
    double v[3];
    for (int k = 0; k < 3; ++k) v[k] = cT[k] - pose.scale * cS[k];
    for (int i = 0; i < 3; ++i)
        res->t[i] = res->R[3 * i] * v[0] + res->R[3 * i + 1] * v[1] + res->R[3 * i + 2] * v[2] + (double)rfinal.T[4 * i + 3];
    // (a13) pointAlign = M * Rotation_Angle(pointSource) (:120/:124, :224-230)
    if (point_align && nsf > 0) {
        DevBuf &dF = c->reg_f, &dG = c->reg_g;
        int rc = upload(c, dF, src_full, (size_t)nsf * 3 * sizeof(double));
        if (rc == KSS_OK) rc = ensure(c, dG, (size_t)nsf * 3 * sizeof(double));
        for (int k = 0; k < 3; ++k) pose.angle[k] = chosen[k];
        if (rc == KSS_OK) rc = kss_pose_apply_dev(c, (const double*)dF.p, nsf, &pose, (double*)dG.p);
        if (rc == KSS_OK) rc = kss_transform_apply_dev(c, rfinal.T, (const double*)dG.p, nsf, (double*)dF.p);
        if (rc == KSS_OK && hipMemcpyAsync(point_align, dF.p, (size_t)nsf * 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream) != hipSuccess) rc = KSS_ERR_HIP;
        if (rc == KSS_OK && hipStreamSynchronize(c->stream) != hipSuccess) rc = KSS_ERR_HIP;
        if (rc != KSS_OK) return rc;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    lap("transform of the full cloud + copy");
#undef RCHK
    return KSS_OK;
}

// ---- many full registrations, concurrently ----------------------------------------------------------------------
static int downsample_for_register(kss_ctx* w, const double* xyz, int64_t n, int64_t m, std::vector<double>& out) {
    out.resize((size_t)n * 3);
    if (m <= 0 || m >= n) { std::memcpy(out.data(), xyz, (size_t)n * 3 * sizeof(double)); return KSS_OK; }
    int64_t k = 0;
    int rc = kss_downsample_aivs(w, xyz, n, m, out.data(), n, &k, nullptr);
    if (rc == KSS_ERR_ARG) {   // degenerate extent (the reference would divide by zero): exact farthest-point sampling
        rc = kss_downsample_fps(w, xyz, n, m, out.data(), nullptr);
        k = m;
    }
    if (rc != KSS_OK) return rc;
    out.resize((size_t)k * 3);
    return KSS_OK;
}

int kss_register_batch(kss_ctx* c, const double* src_all, const int64_t* src_off, const double* tgt_all, const int64_t* tgt_off,
                       int npairs, int64_t sample_cap, double accurate, int iter, int workers, double* point_align_all,
                       kss_register_result* results) {
    if (!c || !src_all || !src_off || !tgt_all || !tgt_off || !results || npairs <= 0) return set_err(c, KSS_ERR_ARG, "register_batch: bad argument");
    for (int i = 0; i < npairs; ++i)
        if (src_off[i + 1] <= src_off[i] || tgt_off[i + 1] <= tgt_off[i]) return set_err(c, KSS_ERR_ARG, "register_batch: empty cloud");
    HIPCHK(c, hipSetDevice(c->device));
    int nw = workers > 0 ? workers : 8;
    nw = std::min(std::min(nw, npairs), 32);
    while ((int)c->workers.size() < nw) {   // worker contexts live as long as the parent
        kss_ctx* w = nullptr;
        const int rc = kss_ctx_create(c->device, &w);
        if (rc != KSS_OK) return set_err(c, rc, "register_batch: cannot create a worker context");
        w->nn_mode = c->nn_mode;
        c->workers.push_back(w);
    }
    std::atomic<int> next{0}, failed{KSS_OK};
    std::string first_error;
    std::mutex err_mutex;
    auto run = [&](kss_ctx* w) {
        hipSetDevice(w->device);
        std::vector<double> ssub, tsub;
        for (;;) {
            const int i = next.fetch_add(1);
            if (i >= npairs || failed.load() != KSS_OK) return;
            const double* S = src_all + 3 * src_off[i];
            const double* T = tgt_all + 3 * tgt_off[i];
            const int64_t ns = src_off[i + 1] - src_off[i], nt = tgt_off[i + 1] - tgt_off[i];
            int64_t pNumber = std::min(ns, nt) / 2;                      // KSS_ICP.hpp:57-63
            if (sample_cap > 0 && pNumber > sample_cap) pNumber = sample_cap;
            int rc = downsample_for_register(w, T, nt, pNumber, tsub);    // :71-75 (target first, as the reference)
            if (rc == KSS_OK) rc = downsample_for_register(w, S, ns, pNumber, ssub);
            if (rc == KSS_OK)
                rc = kss_register(w, ssub.data(), (int64_t)ssub.size() / 3, tsub.data(), (int64_t)tsub.size() / 3, S, ns, accurate, iter,
                                  point_align_all ? point_align_all + 3 * src_off[i] : nullptr, &results[i]);
            if (rc != KSS_OK) {
                std::lock_guard<std::mutex> lk(err_mutex);
                if (failed.load() == KSS_OK) { failed.store(rc); first_error = "register_batch: pair " + std::to_string(i) + ": " + w->err; }
                return;
            }
        }
    };
    std::vector<std::thread> threads;
    for (int k = 1; k < nw; ++k) threads.emplace_back(run, c->workers[(size_t)k]);
    run(c->workers[0]);
    for (std::thread& t : threads) t.join();
    if (failed.load() != KSS_OK) return set_err(c, failed.load(), first_error.c_str());
    return KSS_OK;
}

// ---- RCCL gather of result records ------------------------------------------------------------------------
// ncclAllGather is resolved at run time from librccl.so so that libkssicp.so has no link-time RCCL
// dependency (single-GPU users never load it).
int kss_rccl_allreduce_sum(void* user, double* values, int n) {
    kss_rccl_link* L = (kss_rccl_link*)user;
    if (!L || !L->ctx || !L->rccl_comm || !values || n <= 0) return KSS_ERR_ARG;
    kss_ctx* c = L->ctx;
    HIPCHK(c, hipSetDevice(c->device));
    typedef int (*allreduce_fn)(const void*, void*, size_t, int, int, void*, hipStream_t);
    static allreduce_fn fn = nullptr;
    if (!fn) {
        void* h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!h) return set_err(c, KSS_ERR_RCCL, "cannot dlopen librccl.so");
        fn = (allreduce_fn)dlsym(h, "ncclAllReduce");
        if (!fn) return set_err(c, KSS_ERR_RCCL, "ncclAllReduce not found in librccl.so");
    }
    const size_t bytes = (size_t)n * sizeof(double);
    KCHK(ensure(c, c->sums, std::max<size_t>(bytes, NSUMS * sizeof(double))));
    HIPCHK(c, hipMemcpyAsync(c->sums.p, values, bytes, hipMemcpyHostToDevice, c->stream));
    const int rc = fn(c->sums.p, c->sums.p, (size_t)n, /*ncclFloat64*/ 8, /*ncclSum*/ 0, L->rccl_comm, c->stream);
    if (rc != 0) return set_err(c, KSS_ERR_RCCL, "ncclAllReduce failed");
    HIPCHK(c, hipMemcpyAsync(values, c->sums.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return KSS_OK;
}

int kss_gather_results(kss_ctx* c, void* rccl_comm, int world_size, const kss_icp_result* local, int n_local,
                       kss_icp_result* all) {
    if (!c || !rccl_comm || !local || !all || n_local <= 0 || world_size <= 0) return set_err(c, KSS_ERR_ARG, "gather: bad argument");
    HIPCHK(c, hipSetDevice(c->device));
    typedef int (*allgather_fn)(const void*, void*, size_t, int, void*, hipStream_t);
    static allgather_fn fn = nullptr;
    if (!fn) {
        void* h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!h) return set_err(c, KSS_ERR_RCCL, "cannot dlopen librccl.so");
        fn = (allgather_fn)dlsym(h, "ncclAllGather");
        if (!fn) return set_err(c, KSS_ERR_RCCL, "ncclAllGather not found in librccl.so");
    }
    const size_t bytes = (size_t)n_local * sizeof(kss_icp_result);
    KCHK(ensure(c, c->scratch_a, bytes));
    KCHK(ensure(c, c->scratch_b, bytes * (size_t)world_size));
    HIPCHK(c, hipMemcpyAsync(c->scratch_a.p, local, bytes, hipMemcpyHostToDevice, c->stream));
    const int rc = fn(c->scratch_a.p, c->scratch_b.p, bytes, /*ncclInt8*/ 0, rccl_comm, c->stream);
    if (rc != 0) return set_err(c, KSS_ERR_RCCL, "ncclAllGather failed");
    HIPCHK(c, hipMemcpyAsync(all, c->scratch_b.p, bytes * (size_t)world_size, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return KSS_OK;
}

}  // extern "C"
