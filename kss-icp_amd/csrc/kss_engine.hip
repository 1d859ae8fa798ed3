// kss_engine.hip -- the registration engine behind kss_icp* / kss_nn* / kss_pcr_qm / kss_register: how pairs, source
// blocks and target splits map onto workgroups (IcpPlan), staging of the packed clouds, the cell-list setups, one NN
// pass (fused cell-list launch, batched cell lists, or sweep + reduce + finalize) and the ICP loop around it.
// Host code only orchestrates: per iteration it launches the pass, takes 20 doubles per pair back, solves the 3x3 SVD
// (kss_host_math.hpp) and evaluates the PCL convergence criteria.  There is no CPU compute fallback in this file.
// The pair metrics (point-to-plane, trimmed, robust, generalized, symmetric, similarity, one-to-one) run pairs_loop, one pair or many in
// lockstep; what a pass launches for a mode is said once per kernel family: pair_pass_launch (kss_pair.hip), pairb_pass_launch (kss_pairb.hip).
#pragma clang fp contract(off)

#include <emmintrin.h>
#include <limits>

#include "kss_ctx.hpp"
#include "kss_pair_device.hpp"

namespace kss {

static int restore_zero_at_rest(kss_ctx* c);

// Workgroups of ONE launch that are certainly on the chip at the same time: one per compute unit of THIS device (the fused
// single-pair kernels need at most one CU's registers and LDS each).  Chained launches and the batches whose reducers wait
// in-launch rely on it; on a partitioned or smaller part the limit shrinks with the CU count instead of stalling every
// chain until its polls run out.
static int resident_rows_limit(kss_ctx* c) {
    if (c->cu_count <= 0) {
        hipDeviceProp_t prop;
        c->cu_count = hipGetDeviceProperties(&prop, c->device) == hipSuccess && prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 1;
        (void)hipGetLastError();
    }
    return c->cu_count;
}

constexpr int PUB_PAIRS = 32;   // brute-force batches up to this many pairs are awaited by spinning on the published sums
static int ensure_pub(kss_ctx* c, int npairs = PUB_PAIRS);   // host-mapped result slots (defined with wait_seq)

struct PairGeom {
    int64_t ns, nt;
    int32_t src_base;      // first source in the float4 source arrays
    int32_t tgt_base;      // first (padded) target in tgt4
    int32_t tgt_pad;       // padded target count = n_split * chunk
    int32_t n_split, chunk;
    int32_t key_base;
    int32_t n_src_blocks;
};

struct IcpPlan {
    int npairs = 0, S = 4;
    std::vector<PairGeom> g;
    mutable std::vector<NNWork> nn;   // (single pair on the cell list: filled only if the search ever needs the list pass)
    int per_block = 0;
    size_t nn_count = 0;
    std::vector<RedWork> red;
    std::vector<PairRed> pred;
    int64_t total_src = 0, total_tgt_pad = 0, total_keys = 0;
    bool shared_target = false;
    bool grid = false;      // exact cell-list search (single pair) with brute-force list fallback
    bool gridb = false;     // batched cell lists, one per pair (in-wave brute-force fallback after rcap shells)
    bool src_in_cell_order = false;   // sources were re-ordered by a cell-list setup: .w carries the original index
    GridParams gp;
    int total_cells = 0;
    // fused cell-list pass: one row (= workgroup = chunk of PASS_BS sorted sources) table, pair by pair
    std::vector<GridPairDev> gpairs;
    std::vector<int32_t> row_pair;
    int total_rows = 0;
};
constexpr int PASS_CHUNK = 512;   // == PASS_BS of kss_device.hpp (device-only header)

// sweep work items of pair p: (block of sources) x (target split)
static void fill_nn_table(const IcpPlan& pl, int p) {
    const PairGeom& g = pl.g[p];
    const int per_block = pl.per_block;
    for (int b = 0; b < g.n_src_blocks; ++b)
        for (int s = 0; s < g.n_split; ++s) {
            NNWork w;
            w.pair = p;
            w.src_begin = g.src_base + b * per_block;
            w.src_count = (int32_t)std::min<int64_t>(per_block, g.ns - (int64_t)b * per_block);
            w.tgt_begin = g.tgt_base + s * g.chunk;
            w.tgt_count = g.chunk;
            w.tgt_pair_base = g.tgt_base;
            w.key_begin = g.key_base + (int32_t)((int64_t)s * g.ns) + b * per_block;
            w.write_src = s == 0;
            if (pl.grid) {   // LIST semantics (kss_kernels.hip): offsets into the unresolved list, key row 0
                w.src_begin = b * per_block;
                w.key_begin = g.key_base;
                w.write_src = g.src_base;
            }
            pl.nn.push_back(w);
        }
}

static int build_plan(kss_ctx* c, const int64_t* ns, const int64_t* nt, int npairs, bool shared_target,
               int S_req, int split_req, int nn_mode, IcpPlan& pl) {
    pl.npairs = npairs;
    pl.shared_target = shared_target;
    if (nn_mode == KSS_NN_AUTO) nn_mode = c->nn_mode;
    // AUTO: the fused cell-list pass (one launch + a spin per iteration) beats sweep + reduce + finalize (three launches)
    // down to a few hundred points (1.4k x 1.4k: 22 vs 36 us per iteration); below that the build (~0.1 ms) is not paid
    // back.
    constexpr int64_t min_nt = 512, min_ns = 512;
    pl.grid = nn_mode == KSS_NN_GRID || (nn_mode == KSS_NN_AUTO && npairs == 1 && nt[0] >= min_nt && ns[0] >= min_ns);
    if (npairs != 1) pl.grid = false;
    // (Pairs sharing ONE target -- the candidate batch of kss_register -- stay on the brute-force engine: measured
    // on the fused batch kernel too, 14 candidates x 1406 points: the candidates start from local minima of the rotation
    // search, a few percent of their sources need the in-wave fallback EVERY pass, 123 us per pass against 25 us: 14.3 vs 4.5 ms.
    // On the pair-resident engine, 1406 searches per pass on ONE compute unit: kss_register 24.3 ms against 4.5 ms.)
    if (npairs > 1 && !shared_target) {
        // batch: one cell list per pair.  Measured against the brute-force batch (tools/batch_small.py): brute force wins
        // at 16 pairs x 600 points, they tie at 4 x 1500, the cell lists win from 16 x 1500 and 8 x 4000 up; badly posed
        // batches move back to brute force after one pass (icp_loop).
        int64_t least_nt = nt[0], tot_ns = 0;
        for (int p = 0; p < npairs; ++p) { least_nt = std::min(least_nt, nt[p]); tot_ns += ns[p]; }
        pl.gridb = nn_mode == KSS_NN_GRID || (nn_mode == KSS_NN_AUTO && least_nt >= 2 * min_nt && tot_ns >= 32 * min_ns);
    }
    const bool any_grid = pl.grid || pl.gridb;
    pl.src_in_cell_order = any_grid;
    int64_t tot = 0;
    for (int p = 0; p < npairs; ++p) {
        if (ns[p] <= 0 || nt[p] <= 0) return set_err(c, KSS_ERR_ARG, "empty cloud in ICP pair");
        if (ns[p] > 0x7fff0000ll || nt[p] > 0x7fff0000ll) return set_err(c, KSS_ERR_ARG, "problem too large for 32-bit indexing");
        tot += ns[p];
    }
    int S = S_req;
    int64_t max_tiles = 1;
    for (int p = 0; p < npairs; ++p) max_tiles = std::max<int64_t>(max_tiles, (nt[p] + NN_TILE - 1) / NN_TILE);
    auto blocks_for = [&](int s) { int64_t b = 0; for (int p = 0; p < npairs; ++p) b += (ns[p] + (int64_t)NN_THREADS * s - 1) / ((int64_t)NN_THREADS * s); return b; };
    bool small = false;
    if (S != 1 && S != 2 && S != 4 && S != 8) {
        S = tot >= 32768 ? 4 : (tot >= 8192 ? 2 : 1);
        // small problems (a few 1-2k-point pairs: the candidate batch of kss_register) cannot fill the chip even with one
        // target tile per workgroup: fewer sources per lane and single-tile splits give 4x the workgroups (measured: the
        // sweep of 14 pairs x 1.4k points 38 -> 10 us)
        while (S > 1 && blocks_for(S) * max_tiles < 2048) S /= 2;
        small = blocks_for(S) * max_tiles < 2048;
    }
    pl.S = S;
    const int per_block = NN_THREADS * S;
    const int64_t src_blocks_total = blocks_for(S);
    // enough workgroups to keep 256 CUs x 8 resident workgroups busy with >= 2 rounds
    int64_t want_split = 1;
    if (src_blocks_total < 2048) want_split = (4096 + src_blocks_total - 1) / src_blocks_total;
    if (split_req > 0) want_split = split_req;

    pl.g.resize(npairs);
    int64_t sb = 0, tb = 0, kb = 0;
    for (int p = 0; p < npairs; ++p) {
        PairGeom& g = pl.g[p];
        g.ns = ns[p]; g.nt = nt[p];
        const int64_t tiles = (nt[p] + NN_TILE - 1) / NN_TILE;
        int64_t split = std::min<int64_t>(want_split, std::max<int64_t>(1, small ? tiles : tiles / 2));
        int64_t chunk_tiles = (tiles + split - 1) / split;
        split = (tiles + chunk_tiles - 1) / chunk_tiles;
        g.n_split = (int32_t)split;
        g.chunk = (int32_t)(chunk_tiles * NN_TILE);
        g.tgt_pad = g.n_split * g.chunk;
        g.src_base = (int32_t)sb;
        g.key_base = (int32_t)kb;
        g.n_src_blocks = (int32_t)((ns[p] + per_block - 1) / per_block);
        if (shared_target && p > 0) {
            g.tgt_base = pl.g[0].tgt_base;
        } else {
            g.tgt_base = (int32_t)tb;
            tb += g.tgt_pad;
        }
        sb += ns[p];
        kb += any_grid ? ns[p] : (int64_t)g.n_split * ns[p];
        if (sb > 0x7fff0000ll || tb > 0x7fff0000ll || kb > 0x7fff0000ll)
            return set_err(c, KSS_ERR_ARG, "problem too large for 32-bit indexing");
    }
    pl.total_src = sb; pl.total_tgt_pad = tb; pl.total_keys = kb;
    pl.gpairs.clear(); pl.row_pair.clear(); pl.total_rows = 0;
    if (any_grid) {
        pl.gpairs.resize(npairs);
        for (int p = 0; p < npairs; ++p) {
            GridPairDev& gd = pl.gpairs[p];
            std::memset(&gd, 0, sizeof gd);
            gd.tgt_base = pl.g[p].tgt_base; gd.tgt_n = (int32_t)pl.g[p].nt; gd.tgt_pad = pl.g[p].tgt_pad;
            gd.src_base = pl.g[p].src_base; gd.src_n = (int32_t)pl.g[p].ns;
            gd.row_base = pl.total_rows;
            gd.n_rows = (int32_t)((pl.g[p].ns + PASS_CHUNK - 1) / PASS_CHUNK);
            for (int r = 0; r < gd.n_rows; ++r) pl.row_pair.push_back(p);
            pl.total_rows += gd.n_rows;
        }
    }

    pl.nn.clear(); pl.red.clear(); pl.pred.resize(npairs);
    pl.per_block = per_block;
    pl.nn_count = 0;
    int32_t prow = 0;
    for (int p = 0; p < npairs; ++p) {
        const PairGeom& g = pl.g[p];
        if (!pl.gridb) pl.nn_count += (size_t)g.n_src_blocks * g.n_split;
        if (!pl.gridb && !pl.grid) fill_nn_table(pl, p);   // (cell-list single pair: ~4000 entries nobody reads unless a source falls back; built then)
        pl.pred[p].first = prow;
        // reduce workgroups own 256*R consecutive sources (R = 1 up to 131k sources: the reduce is latency bound,
        // it wants many workgroups; the 240-lane final reduction handles hundreds of rows in a few microseconds)
        int64_t R = (g.ns + 256 * 512 - 1) / (256 * 512);   // <= ~512 partial rows per pair
        R = std::max<int64_t>(1, std::min<int64_t>(R, 64));
        const int64_t rchunk = 256 * R;
        const int nrb = (pl.gridb || pl.grid) ? 0 : (int)((g.ns + rchunk - 1) / rchunk);   // (the cell-list engines reduce inside the fused pass)
        for (int b = 0; b < nrb; ++b) {
            RedWork r;
            r.pair = p;
            r.src_begin = g.src_base + (int32_t)(b * rchunk);
            r.src_count = (int32_t)std::min<int64_t>(rchunk, g.ns - (int64_t)b * rchunk);
            r.key_begin = g.key_base + (int32_t)(b * rchunk);
            r.key_stride = (int32_t)g.ns;
            r.n_split = any_grid ? 1 : g.n_split;
            r.tgt_pair_base = g.tgt_base;
            r.partial_index = prow++;
            pl.red.push_back(r);
        }
        pl.pred[p].count = nrb;
    }
    return KSS_OK;
}

// Work tables of the sweep / reduce kernels (uploaded lazily on the fused cell-list path).
static int stage_tables(kss_ctx* c, const IcpPlan& pl) {
    if (c->tables_staged) return KSS_OK;
    if (pl.grid && pl.nn.empty())
        for (int p = 0; p < pl.npairs; ++p) fill_nn_table(pl, p);
    HIPCHK(c, hipMemcpyAsync(c->nn_work.p, pl.nn.data(), pl.nn.size() * sizeof(NNWork), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->red_work.p, pl.red.data(), pl.red.size() * sizeof(RedWork), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->pair_red.p, pl.pred.data(), pl.pred.size() * sizeof(PairRed), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));   // pageable sources: do not outlive this call unsynchronised
    c->tables_staged = true;
    return KSS_OK;
}

// Upload plan tables and size the workspace.
static int stage_plan(kss_ctx* c, const IcpPlan& pl) {
    KCHK(ensure(c, c->tgt4, (size_t)pl.total_tgt_pad * sizeof(float4)));
    KCHK(ensure(c, c->src0, (size_t)pl.total_src * sizeof(float4)));
    KCHK(ensure(c, c->cur[0], (size_t)pl.total_src * sizeof(float4)));
    KCHK(ensure(c, c->cur[1], (size_t)pl.total_src * sizeof(float4)));
    KCHK(ensure(c, c->keys, (size_t)pl.total_keys * sizeof(unsigned long long)));
    KCHK(ensure_zeroed(c, c->partials, std::max<size_t>(pl.red.size(), (size_t)pl.total_rows) * NSUMS * sizeof(Granule)));   // (rows as 16-byte granules; zeroed when (re)allocated: no stale {bits, number} granule of an earlier owner of the block)
    KCHK(ensure(c, c->sums, (size_t)pl.npairs * NSUMS * sizeof(double)));
    KCHK(ensure(c, c->nn_work, pl.nn_count * sizeof(NNWork)));
    KCHK(ensure(c, c->red_work, pl.red.size() * sizeof(RedWork)));
    KCHK(ensure(c, c->pair_red, pl.pred.size() * sizeof(PairRed)));
    KCHK(ensure(c, c->state, (size_t)pl.npairs * sizeof(PairState)));
    KCHK(ensure_pinned(c, c->h_sums, c->h_sums_cap, (size_t)pl.npairs * NSUMS * sizeof(double)));
    KCHK(ensure_pinned(c, c->h_state, c->h_state_cap, (size_t)pl.npairs * sizeof(PairState)));
    KCHK(ensure_pub(c, pl.npairs));
    c->tables_staged = false;
    // (the fused cell-list path needs the tables only if a query falls back, the candidate kernels not at all: nn_pass stages
    // them the first time its sweep + reduce form runs)
    if (!pl.grid && !pl.shared_target) KCHK(stage_tables(c, pl));
    return KSS_OK;
}

// Pack the clouds of every pair into the float4 workspace (targets sentinel padded).
// dtype: KSS_F32 / KSS_F64 packed triples on the DEVICE; src_off/tgt_off in points.
static int pack_clouds(kss_ctx* c, const IcpPlan& pl, const void* d_src, const int64_t* src_off, const void* d_tgt,
                const int64_t* tgt_off, int dtype) {
    const size_t esz = dtype == KSS_F64 ? sizeof(double) : sizeof(float);
    if (pl.grid) {   // single pair on the cell list: both clouds and the target's bbox partials in one launch
        const PairGeom& g = pl.g[0];
        const int nbb = pack_pair_bbox_rows(g.tgt_pad);
        KCHK(ensure(c, c->g_bbox, (size_t)nbb * 6 * sizeof(float)));
        // up to 8192 partials (2M targets, 256 KB over PCIe) also go straight to host memory as checked granules (grid_setup)
        static const bool box_host = !(getenv("KSS_BBOX_HOST") && atoi(getenv("KSS_BBOX_HOST")) == 0);
        c->box_tag = 0; c->box_rows = 0;
        if (box_host && nbb <= 8192) {
            const size_t want = (size_t)nbb * 32;
            if (want > c->h_box_bytes) {
                if (c->h_box) { HIPCHK(c, hipStreamSynchronize(c->stream)); HIPCHK(c, hipHostFree(c->h_box)); c->h_box = nullptr; c->h_box_dev = nullptr; c->h_box_bytes = 0; }
                void* hp = nullptr; void* dp = nullptr;
                const size_t bytes = want + want / 2;
                if (hipHostMalloc(&hp, bytes, hipHostMallocMapped) == hipSuccess && hipHostGetDevicePointer(&dp, hp, 0) == hipSuccess) {
                    std::memset(hp, 0, bytes);
                    c->h_box = (unsigned int*)hp; c->h_box_dev = (unsigned int*)dp; c->h_box_bytes = bytes;
                } else { if (hp) hipHostFree(hp); (void)hipGetLastError(); }
            }
            if (c->h_box) {
                c->box_tag = (unsigned)(++c->seq);
                if (c->box_tag == 0) c->box_tag = (unsigned)(++c->seq);
                c->box_rows = nbb;
            }
        }
        launch_pack_pair(c->stream, dtype, (const char*)d_tgt + (size_t)tgt_off[0] * 3 * esz, g.nt, (float4*)c->tgt4.p + g.tgt_base, g.tgt_pad,
                         (float*)c->g_bbox.p, (const char*)d_src + (size_t)src_off[0] * 3 * esz, g.ns, (float4*)c->src0.p + g.src_base,
                         c->box_tag ? c->h_box_dev : nullptr, c->box_tag);
        HIPCHK(c, hipGetLastError());
        return KSS_OK;
    }
    // sources are contiguous in both layouts
    {
        const char* base = (const char*)d_src + (size_t)src_off[0] * 3 * esz;
        if (dtype == KSS_F64) launch_pack_f64_to_f4(c->stream, (const double*)base, pl.total_src, (float4*)c->src0.p, pl.total_src, false);
        else launch_pack_f3_to_f4(c->stream, (const float*)base, pl.total_src, (float4*)c->src0.p, pl.total_src, false);
    }
    const int ntp = pl.shared_target ? 1 : pl.npairs;
    if (ntp > 8) {   // many pairs: one launch over a per-pair segment table (segments are laid out back to back in tgt4)
        std::vector<PackSeg> seg((size_t)ntp);
        for (int p = 0; p < ntp; ++p) { seg[p].in_off = tgt_off[p]; seg[p].out_base = pl.g[p].tgt_base; seg[p].n = pl.g[p].nt; }
        KCHK(ensure(c, c->pack_seg, seg.size() * sizeof(PackSeg)));
        HIPCHK(c, hipMemcpyAsync(c->pack_seg.p, seg.data(), seg.size() * sizeof(PackSeg), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));   // `seg` is pageable and about to go out of scope
        launch_pack_batch(c->stream, d_tgt, dtype, (const PackSeg*)c->pack_seg.p, ntp, pl.total_tgt_pad, (float4*)c->tgt4.p);
        HIPCHK(c, hipGetLastError());
        return KSS_OK;
    }
    for (int p = 0; p < ntp; ++p) {
        const PairGeom& g = pl.g[p];
        const char* base = (const char*)d_tgt + (size_t)tgt_off[p] * 3 * esz;
        float4* out = (float4*)c->tgt4.p + g.tgt_base;
        if (dtype == KSS_F64) launch_pack_f64_to_f4(c->stream, (const double*)base, g.nt, out, g.tgt_pad, true);
        else launch_pack_f3_to_f4(c->stream, (const float*)base, g.nt, out, g.tgt_pad, true);
    }
    HIPCHK(c, hipGetLastError());
    return KSS_OK;
}

static void choose_cells(const float mn[3], const float mx[3], int64_t nt, GridParams& gp) {
    const float ext[3] = {mx[0] - mn[0], mx[1] - mn[1], mx[2] - mn[2]};
    const float emax = std::max(ext[0], std::max(ext[1], ext[2]));
    // cell edge: a handful of points per occupied cell if the target is a surface (area ~ emax^2 * few)
    float hscale = 2.0f;
    if (const char* e = getenv("KSS_GRID_HSCALE")) { const float v = (float)atof(e); if (v > 0.05f && v < 50.f) hscale = v; }   // tuning hook
    float h = emax * hscale * std::sqrt(3.0f / (float)nt);
    h = std::max(h, emax / 255.5f);
    if (!(h > 0.f)) h = 1.f;   // all targets coincide
    gp.ox = mn[0]; gp.oy = mn[1]; gp.oz = mn[2];
    gp.h = h; gp.inv_h = 1.0f / h;
    gp.gx = std::max(1, std::min(256, (int)std::floor(ext[0] / h) + 1));
    gp.gy = std::max(1, std::min(256, (int)std::floor(ext[1] / h) + 1));
    gp.gz = std::max(1, std::min(256, (int)std::floor(ext[2] / h) + 1));
    const float mag = std::max(std::max(std::fabs(mn[0]), std::fabs(mx[0])), std::max(std::max(std::fabs(mn[1]), std::fabs(mx[1])), std::max(std::fabs(mn[2]), std::fabs(mx[2]))));
    gp.eps = 2e-6f * (mag + emax) + 1e-30f;
    gp.rcap = 4;   // shells before a query goes to the brute-force list (measured on badly initialised pairs: tools/hard_case.py)
}

// Build the uniform cell list over the (single) target: bbox -> cell size -> counting sort.
static int grid_setup(kss_ctx* c, IcpPlan& pl) {
    if (!pl.grid) return KSS_OK;
    const PairGeom& g = pl.g[0];
    const int nt = (int)g.nt, ns = (int)g.ns;
    const int nbb = pack_pair_bbox_rows(g.tgt_pad);   // one partial per 256 target slots, left by pack_clouds
    const float4* tgt = (const float4*)c->tgt4.p + g.tgt_base;
    ProfScope ps(c, KSS_K_GRID_BUILD);
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    bool have_box = false;
    if (c->box_tag != 0 && c->box_rows == nbb) {
        // the pack kernel's partials as checked granules in host memory: {three floats, tag + check word}, one for the minimum
        // and one for the maximum of every 256 target slots; a granule that is not there yet (or seen torn) is read again
        const unsigned long long* hq = (const unsigned long long*)c->h_box;
        const auto t0 = std::chrono::steady_clock::now();
        int g = 0;
        for (long spin = 0; g < 2 * nbb; ++spin) {
            const unsigned long long w0 = __atomic_load_n(&hq[2 * g], __ATOMIC_ACQUIRE), w1 = __atomic_load_n(&hq[2 * g + 1], __ATOMIC_ACQUIRE);
            const unsigned x = (unsigned)w0, y = (unsigned)(w0 >> 32), z = (unsigned)w1, tag = (unsigned)(w1 >> 32);
            if (tag - kss_mix3(x, y, z) == c->box_tag) {
                float f[3];
                std::memcpy(&f[0], &x, 4); std::memcpy(&f[1], &y, 4); std::memcpy(&f[2], &z, 4);
                for (int k = 0; k < 3; ++k) { if (g & 1) mx[k] = std::max(mx[k], f[k]); else mn[k] = std::min(mn[k], f[k]); }
                ++g;
                continue;
            }
            __builtin_ia32_pause();
            if ((spin & 4095) == 4095 && std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() > 20.0) break;   // (a faulted launch: the copy below reports it)
        }
        have_box = g == 2 * nbb;
        if (!have_box) { for (int k = 0; k < 3; ++k) { mn[k] = INFINITY; mx[k] = -INFINITY; } }
    }
    if (!have_box) {
        std::vector<float>& hb = c->h_bbox;
        hb.resize((size_t)nbb * 6);
        HIPCHK(c, hipMemcpyAsync(hb.data(), c->g_bbox.p, hb.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (int b = 0; b < nbb; ++b)
            for (int k = 0; k < 3; ++k) { mn[k] = std::min(mn[k], hb[(size_t)b * 6 + k]); mx[k] = std::max(mx[k], hb[(size_t)b * 6 + 3 + k]); }
    }
    if (!(std::isfinite(mn[0]) && std::isfinite(mn[1]) && std::isfinite(mn[2]) && std::isfinite(mx[0]) && std::isfinite(mx[1]) && std::isfinite(mx[2])))
        return set_err(c, KSS_ERR_ARG, "non-finite target coordinates");
    GridParams gp;
    choose_cells(mn, mx, nt, gp);
    pl.gp = gp;
    const size_t ncells = (size_t)gp.gx * gp.gy * gp.gz;
    KCHK(ensure_zeroed(c, c->g_counts, 2 * ncells * sizeof(int32_t)));   // target cells, then source cells; zero at rest (kss_ctx.hpp)
    KCHK(ensure(c, c->g_slot, ((size_t)nt + (size_t)ns) * sizeof(int32_t)));   // every point's slot inside its cell, from the count to the scatter
    KCHK(ensure(c, c->g_start, (2 * ncells + 8) * sizeof(int32_t)));   // [0] pad, target starts at [1 .. ncells + 1], source starts (+ nt) behind
    KCHK(ensure(c, c->g_bsums, scan_scratch_bytes((int)(2 * ncells))));
    KCHK(ensure(c, c->g_sorted, (size_t)nt * sizeof(float4)));
    KCHK(ensure(c, c->g_list, (size_t)ns * sizeof(int32_t)));
    KCHK(ensure(c, c->g_pos, (size_t)ns * sizeof(float4)));   // last winner of every source (written by the first pass before any pass reads it)
    c->nn_have = false;
    KCHK(ensure(c, c->g_nnst, (size_t)ns * sizeof(float2)));   // ... and its skip state (written by the first pass before any pass reads it)
    KCHK(ensure_zeroed(c, c->g_count, 64));   // [0] unresolved-list length: zero at rest
    if (getenv("KSS_COUNTS_CHECK")) {   // diagnostic: the zero-at-rest invariant of the cell counters, checked on the host
        HIPCHK(c, hipStreamSynchronize(c->stream));
        std::vector<int32_t> h(2 * ncells);
        HIPCHK(c, hipMemcpy(h.data(), c->g_counts.p, h.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        size_t bad = 0, first = 0;
        for (size_t k = 0; k < h.size(); ++k)
            if (h[k] != 0) { if (!bad) first = k; ++bad; }
        if (bad) {
            std::fprintf(stderr, "[kss] counts check: %zu cells x 2 (%d x %d x %d), buffer %zu bytes, %zu non-zero counters, first at %zu = %d\n", ncells,
                         gp.gx, gp.gy, gp.gz, c->g_counts.cap, bad, first, h[first]);
            return set_err(c, KSS_ERR_HIP, "cell counters not zero at rest");
        }
    }
    pl.gpairs[0].gp = gp;
    pl.gpairs[0].cell_base = 0;
    // both cell lists by shared launches; the sources end up in src0 in the target's cell order (original index in .w);
    // cur[0] is the scatter's scratch
    launch_grid_build_pair(c->stream, tgt, nt, (float4*)c->src0.p + g.src_base, ns, gp, (int32_t*)c->g_counts.p, (int32_t*)c->g_slot.p,
                           (int32_t*)c->g_start.p + 1, (int32_t*)c->g_bsums.p, (float4*)c->g_sorted.p, (float4*)c->cur[0].p);
    HIPCHK(c, hipGetLastError());
    c->grid_stats[0] = gp.h; c->grid_stats[1] = gp.gx; c->grid_stats[2] = gp.gy; c->grid_stats[3] = gp.gz;
    if (c->stats_ns != ns || c->stats_nt != nt) { c->grid_stats[4] = 0; c->grid_stats[5] = 0; }
    c->grid_stats[6] = ns; c->grid_stats[7] = nt;
    if (c->prof && (c->stats_ns != ns || c->stats_nt != nt)) {   // one extra small kernel, once per problem size while profiling
        c->stats_ns = ns; c->stats_nt = nt;
        KCHK(ensure(c, c->scratch_c, 64));
        HIPCHK(c, hipMemsetAsync(c->scratch_c.p, 0, 16, c->stream));
        launch_grid_stats(c->stream, (const float4*)c->src0.p + g.src_base, ns, gp, (const int32_t*)c->g_start.p + 1, (unsigned long long*)c->scratch_c.p);
        unsigned long long hst[2] = {0, 0};
        HIPCHK(c, hipMemcpyAsync(hst, c->scratch_c.p, 16, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->grid_stats[5] = (double)hst[0];
        c->grid_stats[4] = (double)hst[1];
    }
    return KSS_OK;
}

// Batched cell lists: one per pair, all built by the same launches.
static int grid_setup_batch(kss_ctx* c, IcpPlan& pl) {
    if (!pl.gridb) return KSS_OK;
    const int np = pl.npairs;
    std::vector<GridPairDev>& hp = pl.gpairs;   // segments and rows filled by build_plan; cell lists chosen below
    int64_t sum_nt = 0;
    for (int p = 0; p < np; ++p) sum_nt += pl.g[p].nt;
    ProfScope ps(c, KSS_K_GRID_BUILD);
    KCHK(ensure(c, c->g_pairs, (size_t)np * sizeof(GridPairDev)));
    KCHK(ensure(c, c->g_bbox, (size_t)np * 6 * sizeof(float)));
    HIPCHK(c, hipMemcpyAsync(c->g_pairs.p, hp.data(), (size_t)np * sizeof(GridPairDev), hipMemcpyHostToDevice, c->stream));
    launch_gridb_bbox(c->stream, (const float4*)c->tgt4.p, (const GridPairDev*)c->g_pairs.p, np, (float*)c->g_bbox.p);
    std::vector<float> hb((size_t)np * 6);
    HIPCHK(c, hipMemcpyAsync(hb.data(), c->g_bbox.p, hb.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int64_t cells = 0, sorted_base = 0;
    int most_cells = 0;
    for (int p = 0; p < np; ++p) {
        const float* b = &hb[(size_t)p * 6];
        for (int k = 0; k < 6; ++k)
            if (!std::isfinite(b[k])) return set_err(c, KSS_ERR_ARG, "non-finite target coordinates");
        choose_cells(b, b + 3, pl.g[p].nt, hp[p].gp);
        hp[p].cell_base = (int32_t)cells;
        hp[p].sorted_base = (int32_t)sorted_base;
        const int64_t nc = (int64_t)hp[p].gp.gx * hp[p].gp.gy * hp[p].gp.gz;
        most_cells = (int)std::max<int64_t>(most_cells, nc);
        cells += nc;
        sorted_base += pl.g[p].nt;
        if (cells > 0x7fff0000ll) return set_err(c, KSS_ERR_ARG, "batch cell lists exceed 32-bit indexing");
    }
    pl.total_cells = (int)cells;
    HIPCHK(c, hipMemcpyAsync(c->g_pairs.p, hp.data(), (size_t)np * sizeof(GridPairDev), hipMemcpyHostToDevice, c->stream));
    KCHK(ensure(c, c->g_start, ((size_t)cells + 8) * sizeof(int32_t)));   // [0] pad, starts at [1 ..], pads behind
    KCHK(ensure(c, c->g_sorted, (size_t)sum_nt * sizeof(float4)));
    KCHK(ensure(c, c->g_pos, (size_t)pl.total_src * sizeof(float4)));   // last winners (no initialisation: the first pass does not read them)
    c->nn_have = false;
    KCHK(ensure(c, c->g_nnst, (size_t)pl.total_src * sizeof(float2)));
    KCHK(ensure(c, c->g_rowpair, pl.row_pair.size() * sizeof(int32_t)));
    HIPCHK(c, hipMemcpyAsync(c->g_rowpair.p, pl.row_pair.data(), pl.row_pair.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    bool half = true;   // 16-bit counters: counts and in-pair positions of every pair fit
    for (int p = 0; p < np; ++p) half = half && pl.g[p].nt < 65536 && pl.g[p].ns < 65536;
    // every pair's counters fit a CU's LDS: one workgroup per pair builds both of its lists (kss_grid.hip)
    const bool built_in_lds = most_cells <= gridb_lds_max_cells(half) &&
        launch_gridb_build_lds(c->stream, (const float4*)c->tgt4.p, (float4*)c->src0.p, (float4*)c->cur[0].p, (const GridPairDev*)c->g_pairs.p, np,
                               (int32_t*)c->g_start.p + 1, (float4*)c->g_sorted.p, (int)most_cells, half);
    if (!built_in_lds) {
        // (zero at rest, as the single-pair build expects of this buffer: a plain ensure() here once left the slack behind
        // `cells` uninitialised, and a later single pair with more cells scanned garbage counts -- see DESIGN.md, incidents)
        KCHK(ensure_zeroed(c, c->g_counts, (size_t)cells * sizeof(int32_t)));
        KCHK(ensure(c, c->g_start2, ((size_t)cells + 1) * sizeof(int32_t)));
        KCHK(ensure(c, c->g_bsums, scan_scratch_bytes((int)cells)));
        if ((cells + 4095) / 4096 > 1024 * 16) return set_err(c, KSS_ERR_ARG, "batch cell lists too large for the scan");
        launch_gridb_build_targets(c->stream, (const float4*)c->tgt4.p, (int)pl.total_tgt_pad, (const GridPairDev*)c->g_pairs.p, np,
                                   (int)cells, (int32_t*)c->g_counts.p, (int32_t*)c->g_start.p + 1,
                                   (int32_t*)c->g_bsums.p, (float4*)c->g_sorted.p);
        launch_gridb_sort_sources(c->stream, (const float4*)c->src0.p, (int)pl.total_src, (const GridPairDev*)c->g_pairs.p, np, (int)cells,
                                  (int32_t*)c->g_counts.p, (int32_t*)c->g_start2.p, (int32_t*)c->g_bsums.p,
                                  (float4*)c->cur[0].p, (float4*)c->src0.p);   // (scatter: src0 -> cur[0]; rank fix: cur[0] -> src0)
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));   // hb is about to go out of scope (pageable)
    return KSS_OK;
}

// Host-mapped result slots: PUB_PAIRS x NSUMS x {bits(sum), sequence number}.  The kernel that ends an ICP iteration
// (fused grid_nn_kernel, or finalize_sums_kernel for small batches) stores every sum TOGETHER with the launch's
// sequence number as one aligned 16-byte write: a slot whose sequence number matches holds this launch's value, so
// there is no separate completion flag and no write-acknowledge round trip between "sums stored" and "flag stored"
// on the device.
static int ensure_pub(kss_ctx* c, int npairs) {
    const size_t want = (size_t)std::max(npairs, PUB_PAIRS) * (NSUMS + 1) * 16;   // (+1: the resident engines' exit flag of the pair, behind the launch's slots)
    if (c->h_seq && want <= c->h_seq_bytes) return KSS_OK;
    if (c->h_seq) {   // grow: nothing may still be writing the old slots
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipHostFree(c->h_seq));
        c->h_seq = nullptr; c->h_seq_dev = nullptr; c->h_seq_bytes = 0;
    }
    void* p = nullptr;
    const size_t bytes = want + want / 4;
    if (hipHostMalloc(&p, bytes, hipHostMallocMapped) != hipSuccess) return set_err(c, KSS_ERR_NOMEM, "hipHostMalloc(result slots)");
    c->h_seq = (unsigned long long*)p;
    c->h_seq_bytes = bytes;
    std::memset(p, 0, bytes);
    void* d = nullptr;
    HIPCHK(c, hipHostGetDevicePointer(&d, p, 0));
    c->h_seq_dev = (unsigned long long*)d;
    return KSS_OK;
}

// Wait for the first `npairs * NSUMS` slots to carry sequence number c->seq and copy the sums to h_sums, where the rest
// of the loop expects them.  The host spins (a stream sync costs a 5-10 us wake-up per ICP iteration); after ~2 ms
// without progress it falls back to the stream sync, which also surfaces a faulted kernel instead of spinning forever.
static void gated_cancel(kss_ctx* c);

// the 20 sums of pair p of launch `want`, if they have all landed (the slots' format and their reader: kss_handover.hpp)
static inline bool collect_pair(kss_ctx* c, int p, unsigned long long want) {
    const unsigned long long* sl = c->h_seq + (size_t)2 * NSUMS * p;
    double* out = (double*)c->h_sums + (size_t)NSUMS * p;
    if (!slots_collect(sl + 2 * (NSUMS - 1), 1, want, out + NSUMS - 1)) return false;   // the highest slot is usually the last to land
    return slots_collect(sl, NSUMS, want, out);
}

// wait for pair p's sums (spin; after ~2 ms without them: open any gate, synchronize the stream, look once more)
static int wait_pair(kss_ctx* c, int p, unsigned long long want) {
    for (long spin = 0; spin < 2000000; ++spin) {
        if (collect_pair(c, p, want)) return KSS_OK;
        __builtin_ia32_pause();
    }
    return KSS_ERR_HIP;   // the caller synchronizes (only one thread may) and retries
}

// not_published (optional): set when the stream drained without error and the slots still do not carry `want` -- the caller
// may know how to go on (a gated launch that gave up waiting for a stalled host thread has not touched anything)
static int wait_seq(kss_ctx* c, int npairs = 1, unsigned long long want = 0, const int* active = nullptr, bool* not_published = nullptr) {
    if (!want) want = c->seq;
    bool slow = false;
    for (int p = npairs - 1; p >= 0; --p) {
        if (active && !active[p]) continue;
        if (!slow && wait_pair(c, p, want) == KSS_OK) continue;
        if (!slow) {
            gated_cancel(c);   // a pre-enqueued launch behind a closed gate would make the synchronize below wait forever
            HIPCHK(c, hipStreamSynchronize(c->stream));
            slow = true;
        }
        if (!collect_pair(c, p, want)) {
            if (not_published) *not_published = true;
            return set_err(c, KSS_ERR_HIP, "kernel finished without publishing its result");
        }
    }
    return KSS_OK;
}

// the first `nslots` result slots of the launch with sequence number c->seq, as doubles (pre-shape statistics)
int ensure_pub_slots(kss_ctx* c) { return ensure_pub(c); }
int wait_slots(kss_ctx* c, int nslots, double* out) {
    const unsigned long long want = c->seq;
    for (long spin = 0; spin < 2000000; ++spin) {
        if (slots_collect(c->h_seq, nslots, want, out)) return KSS_OK;
        __builtin_ia32_pause();
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));   // surfaces a faulted kernel instead of spinning forever
    if (!slots_collect(c->h_seq, nslots, want, out)) return set_err(c, KSS_ERR_HIP, "kernel finished without publishing its result");
    return KSS_OK;
}

// ---- gated launches of the fused single-pair pass -------------------------------------------------------------
// Per ICP iteration the host has to see the sums, solve, and only then does the next transform exist: hipLaunchKernel
// (~3 us on the host), the dispatch after it and the new workgroups' first loads all sat on the critical path.  With
// gating the NEXT iteration's kernel is enqueued while the current one runs; it starts as soon as the current one ends,
// fetches its sources and previous winners, and polls a host-mapped 64-byte record for its transform (kss_grid.hip,
// grid_pass_kernel).  When the sums are in, the host solves, writes the transform into the record and stamps it with the
// launch's number (one release store): the kernel goes on from there -- no stream operation, no second PCIe round trip
// for the transform.  (Round 1 parked the kernel behind a hipStreamWaitValue64 and let it fetch the transform afterwards:
// wait-kernel -> dispatch -> fetch were three dependent steps where this has one.)  A pre-enqueued kernel the loop does not
// need (convergence, the brute-force fallback, an error) is CANCELLED: stamped with pad[0] = 1, it leaves at once.
// Nothing ever waits on a cancelled kernel, no path returns with a kernel unanswered (GatedGuard), and the kernel's poll
// is bounded, so neither side can wait forever.  A polling kernel keeps its workgroups resident (200 of ~770 slots at
// C2): other streams still run.  Exclusions: only on a stream the context owns and only while it is the only context
// of the process (several loops polling at once could crowd each other's real work out of the CUs), never with an
// all-reduce callback (its collective would queue up on this stream BEHIND the polling kernel, whose transform depends
// on it).  KSS_GATED=0 turns it off.
static bool gated_available(kss_ctx* c) {
    static const bool want = getenv("KSS_GATED") == nullptr || atoi(getenv("KSS_GATED")) != 0;   // KSS_GATED=0 switches it off
    if (!want || !c->own_stream || kss_live_contexts().load() != 1) return false;
    if (c->gated.supported < 0) {
        c->gated.supported = 0;
        // the device-side granules: on a large-BAR system in FINE-GRAINED device memory, which the host can store into directly
        // (tools/bar_probe.hip: same 2.1 us host -> kernel -> host round trip as a kernel polling host memory, but every
        // workgroup can poll it: no asking workgroup, no re-publication hop).  KSS_GATE_BAR=0: always the re-publishing form.
        if (bar_ensure(c, c->gate_bar, 256)) {   // two records, 128 bytes apart
            c->gated.supported = 1;
            return true;
        }
        void *x = nullptr, *xd = nullptr;
        if (ensure(c, c->g_gate, 256) == KSS_OK && hipMemsetAsync(c->g_gate.p, 0, 256, c->stream) == hipSuccess &&
            hipHostMalloc(&x, 2 * sizeof(PairState), hipHostMallocMapped) == hipSuccess && hipHostGetDevicePointer(&xd, x, 0) == hipSuccess) {
            std::memset(x, 0, 2 * sizeof(PairState));
            c->h_xf = (PairState*)x; c->h_xf_dev = (PairState*)xd;
            c->gated.supported = 1;
        } else {
            (void)hipGetLastError();
            if (x) hipHostFree(x);
        }
    }
    return c->gated.supported == 1;
}

static void gated_release(kss_ctx* c, const PairState& st, int skip) {   // transform (or the cancel mark), stamped
    if (c->gate_bar.p) {
        // the record straight into device memory through the BAR (kss_handover.hpp)
        unsigned words[16];
        std::memcpy(words, &st, sizeof st);
        words[14] = (unsigned)skip;             // pad[0]
        // (test hook: the n-th record of the process first arrives torn)
        static const long torn_at = getenv("KSS_TEST_TORN_GATE") ? atol(getenv("KSS_TEST_TORN_GATE")) : -1;
        static long released = 0;
        gate_record_store((unsigned*)c->gate_bar.p + 32 * c->gated.slot, words, (unsigned)c->gated.stamp, ++released == torn_at);   // two records, 128 bytes apart
    } else {
        PairState* rec = &c->h_xf[c->gated.slot];
        for (int k = 0; k < 12; ++k) rec->m[k] = st.m[k];
        rec->active = st.active; rec->apply = st.apply; rec->pad[0] = skip;
        __atomic_store_n(&rec->pad[1], c->gated.stamp, __ATOMIC_RELEASE);   // the kernel accepts the record when it reads this stamp
    }
    kss_ctx::Gated& G = c->gated;
    if (!skip && --G.steps_left > 0) {
        // a chained launch: its next pass waits for the next stamp in the other record, publishes under the next sequence
        // number and reads what this pass writes
        G.slot ^= 1;
        G.stamp += 1;                       // (the launch made sure the chain's stamps do not wrap)
        G.seq += 1;
        const void* in = G.d_out; G.d_out = const_cast<void*>(G.d_in); G.d_in = in;
    } else {
        G.pending = false;
        G.steps_left = 0;
    }
}

static void gated_cancel(kss_ctx* c) {
    if (!c->gated.pending) return;
    PairState none;
    std::memset(&none, 0, sizeof none);
    gated_release(c, none, 1);
}

struct GatedGuard {   // no exit from the ICP loop leaves a gate closed
    kss_ctx* c;
    explicit GatedGuard(kss_ctx* c_) : c(c_) {}
    ~GatedGuard() { gated_cancel(c); c->gated.want_next = false; }
};

// settings two engines share, each read once (at its first use)
static float skin_setting() {   // KSS_SKIN=-1: every source searches in every pass
    static const float skin = getenv("KSS_SKIN") ? (float)atof(getenv("KSS_SKIN")) : 0.25f;
    return skin;
}
static int gate_polls_setting() {   // bound of a waiting kernel's poll (~1 us each)
    static const int gate_polls = getenv("KSS_GATE_POLLS") ? atoi(getenv("KSS_GATE_POLLS")) : (1 << 22);
    return gate_polls;
}

// arguments of the fused cell-list pass for this plan (single pair or batch)
static PassArgs pass_args(kss_ctx* c, const IcpPlan& pl, const float4* d_in, float4* d_out, double max_d2,
                          int32_t* d_idx_out, float* d_d2_out) {
    PassArgs a;
    std::memset(&a, 0, sizeof a);
    a.src_in = d_in; a.src_out = d_out;
    a.cell_start = (const int32_t*)c->g_start.p + 1;
    a.sorted = (const float4*)c->g_sorted.p;
    a.tgt4 = (const float4*)c->tgt4.p;
    a.nn_win = (float4*)c->g_pos.p;
    a.nn_state = (float2*)c->g_nnst.p;
    a.skin = skin_setting();
    a.chain_len = 1;
    a.gate_polls = gate_polls_setting();
    a.chained = d_in != (const float4*)c->src0.p ? 1 : c->fit_last ? 2 : 0;   // (the first pass and the fitness pass read the original cloud)
    a.src_last0 = (const float4*)c->cur[0].p; a.src_last1 = (const float4*)c->cur[1].p;
    a.keys = (unsigned long long*)c->keys.p;
    a.list = (int32_t*)c->g_list.p; a.list_count = (int32_t*)c->g_count.p;
    a.total_rows = pl.total_rows;
    a.use_prev = c->nn_have ? 1 : 0;   // (nn_have: a search pass of this registration has written the per-source state)
    a.max_d2 = max_d2;
    a.rows = (Granule*)c->partials.p;
    a.pub = c->h_seq_dev;
    a.idx_out = d_idx_out; a.d2_out = d_d2_out;
    {   // test hook: the n-th fused launch stores one of its result slots torn first (kss_grid.hip)
        static const long torn_at = getenv("KSS_TEST_TORN_SLOT") ? atol(getenv("KSS_TEST_TORN_SLOT")) : -1;
        static long launches = 0;
        a.test_torn = torn_at > 0 && ++launches == torn_at ? 1 : 0;
    }
    if (pl.gridb) {
        a.pairs = (const GridPairDev*)c->g_pairs.p;
        a.row_pair = (const int32_t*)c->g_rowpair.p;
        // each pair's first workgroup adds the pair's rows up in the pass -- one waiter per pair, so at most one per compute
        // unit -- or, with more pairs than that, a finalize launch right after it does
        a.defer_pairs = pl.npairs > resident_rows_limit(c) ? pl.npairs : 0;
    } else {
        a.pair0 = pl.gpairs[0];   // (a single pair: its first workgroup is the one waiter, at any row count)
    }
    return a;
}

// ---- the fused single pair's pass (pl.grid): the gated chain as five steps, in this order ----
// what the steps hand on: the pass as nn_pass was asked for it, the plain launch's arguments, which launch is waited for
struct GridPass {
    const IcpPlan& pl;
    bool fma, full;
    const float4* d_in; float4* d_out;
    double max_d2;
    int32_t* d_idx_out; float* d_d2_out;
    PassArgs a;                               // the pass as a plain launch
    int nblk;
    unsigned long long* stamps2 = nullptr;    // KSS_GRID_STAMPS=2: two buffers that alternate with the launch's sequence number
    bool plain_args = false;                  // nothing a pre-enqueued launch could not have been given
    unsigned long long want_seq = 0;          // the launch whose sums this pass waits for
    bool via_gate = false;                    // ... was enqueued earlier and released by step 1
};

// search + correspondence sums + final reduction in ONE launch; sums land in host-mapped memory
static void grid_launch_plain(kss_ctx* c, GridPass& g) {
    ProfScope ps(c, KSS_K_GRID_NN);
    g.a.ps0 = ((const PairState*)c->h_state)[0];
    g.a.seq = ++c->seq;
    if (g.stamps2) g.a.stamps = g.stamps2 + (size_t)(g.a.seq & 1) * g.nblk * 16;
    launch_grid_pass(c->stream, g.fma, g.full, false, true, g.a);
    c->nn_have = true;
    g.want_seq = c->seq;
}

// step 1: release the pending launch if it is this pass, or launch plain
static void grid_release_or_launch(kss_ctx* c, GridPass& g) {
    kss_ctx::Gated& G = c->gated;
    if (G.pending && G.d_in == (const void*)g.d_in && G.d_out == (void*)g.d_out && G.fma == g.fma && G.full == g.full && G.max_d2 == g.max_d2 && g.plain_args) {
        // this pass was enqueued while the previous one ran: hand it its transform and open the gate
        g.want_seq = G.seq;
        c->seq = std::max(c->seq, G.seq);   // (sequence numbers of a chain are taken as its passes are released)
        if (G.chain && c->prof > 0) c->prof_n[KSS_K_GRID_CHAIN_PASS] += 1;
        g.via_gate = true;
        // (test hook: the n-th answer is never written -- a host thread that stalls for longer than the kernel's bounded
        // poll.  The waiting kernel gives up at the gate, having touched nothing, and the pass is launched again by step 3.)
        static const long drop_at = getenv("KSS_TEST_DROP_GATE") ? atol(getenv("KSS_TEST_DROP_GATE")) : -1;
        static long releases = 0;
        if (++releases == drop_at) { G.pending = false; G.steps_left = 0; }
        else gated_release(c, ((const PairState*)c->h_state)[0], 0);
    } else {
        gated_cancel(c);   // (a pre-enqueued kernel that does not fit this pass, e.g. before the fitness pass)
        grid_launch_plain(c, g);
    }
}

// step 2: decide how many iterations the next pre-enqueued launch may run, and enqueue it behind the gate while this pass runs
static void grid_enqueue_next(kss_ctx* c, const GridPass& g) {
    kss_ctx::Gated& G = c->gated;
    // HIP-event timing: a bracket behind the gate would also time the dispatch that follows the wait, so the launches
    // the profiler samples (every n-th) are plain launches; the others advance its tick here
    const bool next_sampled = c->prof == 1 || (c->prof > 1 && c->prof_tick[KSS_K_GRID_NN] % (unsigned)c->prof == 0);
    // how many iterations a pre-enqueued launch may run: all that can still follow (KSS_CHAIN=0: one, the form of every
    // system without a large BAR).  A single gated launch stays out of the way of the launches the profiler samples; a
    // chain is bracketed as a whole instead.
    static const bool want_chain = getenv("KSS_CHAIN") == nullptr || atoi(getenv("KSS_CHAIN")) != 0;
    int len = 1;
    if (G.want_next && !G.pending && g.plain_args && gated_available(c) && want_chain && c->gate_bar.p &&
        (g.pl.total_rows <= resident_rows_limit(c) || g.pl.total_rows == 1))   // (every workgroup of a chain waits at its gates: resident at once)
        len = std::max(1, std::min(G.max_steps, 1 << 16));
    if (!(G.want_next && !G.pending && g.plain_args && gated_available(c) && (len > 1 || !next_sampled))) return;
    if (c->prof > 1 && len == 1) ++c->prof_tick[KSS_K_GRID_NN];
    // the NEXT iteration reads what this pass writes (d_out) and writes the other ping-pong buffer
    float4* nxt_out = g.d_out == (float4*)c->cur[0].p ? (float4*)c->cur[1].p : (float4*)c->cur[0].p;
    G.slot ^= 1;
    G.stamp = (G.stamp + 1) & 0x7fffffff;
    if (G.stamp == 0 || G.stamp > 0x7fffffff - len - 1) G.stamp = 1;   // (0 is what a fresh record holds; a chain's stamps do not wrap)
    PassArgs n = pass_args(c, g.pl, g.d_out, nxt_out, g.max_d2, nullptr, nullptr);
    n.ps0 = ((const PairState*)c->h_state)[0];
    n.gate_seq = G.stamp;
    if (c->gate_bar.p) {   // the host writes the granules itself
        n.state = nullptr;
        n.gate_dev = (unsigned int*)c->gate_bar.p;    // two records, 128 bytes apart: pass k of the launch polls record (slot + k) & 1
        n.gate_slot = G.slot;
        n.chain_len = len;
        n.src_alt = g.d_out;
    } else {             // workgroup 0 asks the host-mapped record and re-publishes
        n.state = c->h_xf_dev + G.slot;
        n.gate_dev = (unsigned int*)c->g_gate.p;
    }
    n.seq = c->seq + 1;          // (taken when the pass is released)
    if (g.stamps2) n.stamps = g.stamps2 + (size_t)(n.seq & 1) * g.nblk * 16;
    if (len > 1) {   // bracketed as a whole whenever profiling is on (KSS_K_GRID_CHAIN; per pass: KSS_K_GRID_CHAIN_PASS)
        ProfScope ps(c, KSS_K_GRID_CHAIN, true);
        launch_grid_pass(c->stream, g.fma, G.want_full, false, true, n);
    } else {
        launch_grid_pass(c->stream, g.fma, G.want_full, false, true, n);
    }
    G.chain = len > 1;
    G.pending = true; G.steps_left = len; G.seq = n.seq; G.d_in = g.d_out; G.d_out = nxt_out; G.fma = g.fma; G.full = G.want_full; G.max_d2 = g.max_d2;
    if (hipGetLastError() != hipSuccess) { gated_cancel(c); G.supported = 0; }   // (if it did get queued it is answered; gating is given up)
}

// step 3: wait for the pass's sums; a waiting kernel that left unanswered is launched again as a plain pass
static int grid_wait(kss_ctx* c, GridPass& g) {
    bool not_published = false;
    const int rcw = wait_seq(c, 1, g.want_seq, nullptr, &not_published);
    if (rcw == KSS_OK || !g.via_gate || !not_published) return rcw;
    // The waiting kernel left at its gate (bounded poll: this thread was stalled, or the answer never arrived) and
    // the stream has drained.  Nothing of this pass has been written: launch it as a plain pass.
    c->gated.pending = false; c->gated.steps_left = 0;
    c->err.clear();
    std::fprintf(stderr, "[kss] a waiting kernel was not answered in time and left; the pass is launched again\n");
    // With more rows than resident workgroups the launch may have left in part only: workgroups that started after
    // the answer finally arrived have run, written their sources and may have put sources on the fallback list.
    // The stream has drained (wait_seq synchronised): re-arm everything that is zero at rest before the plain launch.
    c->ws_dirty = true;
    KCHK(restore_zero_at_rest(c));
    grid_launch_plain(c, g);
    HIPCHK(c, hipGetLastError());
    return wait_seq(c, 1, g.want_seq);
}

// step 4, and its arming ahead of step 1: diagnostic builds of the timeline (tools/grid_stamps.py).  KSS_GRID_STAMPS=1: plain
// launches, buffer cleared and read back every pass.  =2: the gated chain as it runs in production; two buffers alternate with
// the launch sequence number (the launch pre-enqueued behind the last real one is cancelled but has stamped its start) and
// kss_debug_grid_stamps fetches the one of the last launch that was waited for.
static int grid_stamps_arm(kss_ctx* c, GridPass& g) {
    static const int stamps_mode = getenv("KSS_GRID_STAMPS") ? atoi(getenv("KSS_GRID_STAMPS")) : 0;
    if (stamps_mode == 1) {
        KCHK(ensure(c, c->g_stamps, (size_t)g.nblk * 16 * sizeof(unsigned long long)));
        HIPCHK(c, hipMemsetAsync(c->g_stamps.p, 0, (size_t)g.nblk * 16 * sizeof(unsigned long long), c->stream));
        g.a.stamps = (unsigned long long*)c->g_stamps.p;
    } else if (stamps_mode == 2) {
        KCHK(ensure(c, c->g_stamps, (size_t)g.nblk * 32 * sizeof(unsigned long long)));
        g.stamps2 = (unsigned long long*)c->g_stamps.p;
        c->stamps_nblk = g.nblk;
    }
    return KSS_OK;
}
static int grid_stamps_read(kss_ctx* c, const GridPass& g) {
    if (g.stamps2) { c->stamps_seq = g.want_seq; return KSS_OK; }
    if (!g.a.stamps) return KSS_OK;
    c->last_stamps.resize((size_t)g.nblk * 16);
    HIPCHK(c, hipMemcpy(c->last_stamps.data(), g.a.stamps, c->last_stamps.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (int b = 0; b < g.nblk; ++b) c->evals_sum += (double)c->last_stamps[(size_t)b * 16 + 10];
    c->evals_launches += 1.0;
    return KSS_OK;
}

// step 5: sources the cell search gave up on (far from the target): brute-force sweep over the list, then the sums
// again by a SEARCH = false launch of the fused pass -- same rows, same order, so the result does not depend
// on WHICH sources needed the list
static int grid_list_fallback(kss_ctx* c, const GridPass& g) {
    const IcpPlan& pl = g.pl;
    gated_cancel(c);              // the list pass must not queue up behind a closed gate
    c->gated.want_next = false;   // (clouds this far apart: plain launches until the loop says otherwise)
    KCHK(stage_tables(c, pl));
    {   // the list sweep reads the pair's device-side state (active, identity): uploaded here, on the rare path only
        PairState one;
        std::memset(&one, 0, sizeof one);
        one.active = 1;
        HIPCHK(c, hipMemcpy(c->state.p, &one, sizeof one, hipMemcpyHostToDevice));
    }
    if (getenv("KSS_LIST_CHECK")) {   // diagnostic: the list the search pass has left, checked on the host before it is used
        HIPCHK(c, hipStreamSynchronize(c->stream));
        int32_t cnt = -1;
        HIPCHK(c, hipMemcpy(&cnt, c->g_count.p, sizeof cnt, hipMemcpyDeviceToHost));
        const int64_t ns0 = pl.g[0].ns;
        std::vector<int32_t> l((size_t)std::max<int64_t>(0, std::min<int64_t>(cnt, ns0)));
        if (!l.empty()) HIPCHK(c, hipMemcpy(l.data(), c->g_list.p, l.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        int64_t bad = 0;
        for (int32_t v : l) bad += v < 0 || v >= ns0;
        std::fprintf(stderr, "[kss] list check: count %d of %lld sources (column 19 said %.0f), %lld entries out of range, nn table %zu items, S %d\n",
                     cnt, (long long)ns0, ((const double*)c->h_sums)[NSUMS - 1], (long long)bad, pl.nn.size(), pl.S);
        if (cnt < 0 || cnt > ns0 || bad) return set_err(c, KSS_ERR_HIP, "list check failed");
    }
    {
        ProfScope ps(c, KSS_K_NN_SWEEP);
        launch_nn_sweep_list(c->stream, pl.S, g.fma, (const NNWork*)c->nn_work.p, (int)pl.nn.size(), (const PairState*)c->state.p,
                             g.d_out, (const float4*)c->tgt4.p, (unsigned long long*)c->keys.p, (const int32_t*)c->g_list.p,
                             (const int32_t*)c->g_count.p);
    }
    HIPCHK(c, hipMemsetAsync(c->g_count.p, 0, sizeof(int32_t), c->stream));   // the list is consumed
    {
        ProfScope ps(c, KSS_K_CORR_REDUCE);
        PassArgs r = pass_args(c, pl, g.d_in, g.d_out, g.max_d2, g.d_idx_out, g.d_d2_out);
        r.ps0 = ((const PairState*)c->h_state)[0];
        r.seq = ++c->seq;
        launch_grid_pass(c->stream, g.fma, true, false, false, r);
    }
    HIPCHK(c, hipGetLastError());
    return wait_seq(c, 1, c->seq);
}

// single pair on its cell list: the transform rides in the kernel arguments
static int nn_pass_grid(kss_ctx* c, const IcpPlan& pl, bool fma, const float4* d_in, float4* d_out, double max_d2,
                        int32_t* d_idx_out, float* d_d2_out, bool full) {
    GridPass g = {pl, fma, full, d_in, d_out, max_d2, d_idx_out, d_d2_out, pass_args(c, pl, d_in, d_out, max_d2, d_idx_out, d_d2_out),
                  grid_pass_blocks(pl.total_rows)};
    KCHK(grid_stamps_arm(c, g));
    g.plain_args = !g.a.stamps && !d_idx_out && !d_d2_out;
    const auto tl0 = c->timing ? std::chrono::steady_clock::now() : std::chrono::steady_clock::time_point();
    grid_release_or_launch(c, g);
    HIPCHK(c, hipGetLastError());
    grid_enqueue_next(c, g);
    const auto tl1 = c->timing ? std::chrono::steady_clock::now() : std::chrono::steady_clock::time_point();
    KCHK(grid_wait(c, g));
    if (c->timing) {
        const auto tl2 = std::chrono::steady_clock::now();
        c->t_launch_us += std::chrono::duration<double, std::micro>(tl1 - tl0).count();
        c->t_wait_us += std::chrono::duration<double, std::micro>(tl2 - tl1).count();
    }
    KCHK(grid_stamps_read(c, g));
    if (((const double*)c->h_sums)[NSUMS - 1] > 0.0) KCHK(grid_list_fallback(c, g));
    ((double*)c->h_sums)[NSUMS - 1] = 0.0;
    return KSS_OK;
}

// batched cell lists
static int nn_pass_gridb(kss_ctx* c, const IcpPlan& pl, bool fma, const float4* d_in, float4* d_out, double max_d2,
                         int32_t* d_idx_out, float* d_d2_out, bool full, const int* active) {
    PairState* hs = (PairState*)c->h_state;
    // batch: one launch searches every active pair; each pair's sums are published as soon as its rows are added up --
    // inside the launch by the pair's first workgroup, or, with more pairs than compute units, by the finalize launch
    // right after it (then every pair lands only once the whole pass is done).
    // The per-pair states (transform to apply, active flag) are read by every workgroup: a small batch reads them
    // straight from the pinned host-mapped table (no copy operation on the stream), a large one (thousands of
    // workgroups) gets the table copied to device memory once per pass.
    PassArgs a = pass_args(c, pl, d_in, d_out, max_d2, d_idx_out, d_d2_out);
    a.state = (const PairState*)c->state.p;
    if (c->bar_state.p && c->bar_state.cap >= (size_t)pl.npairs * sizeof(PairState)) {   // the host has stored the states there itself (mirror_state)
        _mm_sfence();
        a.state = (const PairState*)c->bar_state.p;
    }
    constexpr int host_state_rows = 32768;   // (measured at C3, 20480 workgroups: 9.71 ms from host memory vs 9.85 ms with the copy)
    if (a.state != (const PairState*)c->bar_state.p && pl.total_rows <= host_state_rows) {
        void* dev = nullptr;
        if (hipHostGetDevicePointer(&dev, c->h_state, 0) == hipSuccess && dev) a.state = (const PairState*)dev;
    }
    if (a.state == (const PairState*)c->state.p)
        HIPCHK(c, hipMemcpyAsync(c->state.p, hs, (size_t)pl.npairs * sizeof(PairState), hipMemcpyHostToDevice, c->stream));
    c->last_state_dev = a.state;
    const int nblk = grid_pass_blocks(pl.total_rows);
    if (getenv("KSS_GRID_STAMPS")) {   // diagnostic build of the timeline (tools/batch_stamps.py)
        KCHK(ensure(c, c->g_stamps, (size_t)nblk * 16 * sizeof(unsigned long long)));
        HIPCHK(c, hipMemsetAsync(c->g_stamps.p, 0, (size_t)nblk * 16 * sizeof(unsigned long long), c->stream));
        a.stamps = (unsigned long long*)c->g_stamps.p;
    }
    {
        ProfScope ps(c, KSS_K_GRID_NN);
        a.seq = ++c->seq;
        launch_grid_pass(c->stream, fma, full, true, true, a);
        c->nn_have = true;
    }
    HIPCHK(c, hipGetLastError());
    if (a.stamps) {
        HIPCHK(c, hipStreamSynchronize(c->stream));   // (the stream does not synchronise with the null stream)
        c->last_stamps.resize((size_t)nblk * 16);
        HIPCHK(c, hipMemcpy(c->last_stamps.data(), a.stamps, c->last_stamps.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    }
    if (!c->defer_wait) KCHK(wait_seq(c, pl.npairs, c->seq, active));
    return KSS_OK;
}

// brute-force engine.  Per-pair states as above.
static int nn_pass_brute(kss_ctx* c, const IcpPlan& pl, bool fma, const float4* d_in, float4* d_out, double max_d2,
                         int32_t* d_idx_out, float* d_d2_out, const int* active) {
    PairState* hs = (PairState*)c->h_state;
    const PairState* d_state = (const PairState*)c->state.p;
    if (pl.npairs <= PUB_PAIRS) {
        void* dev = nullptr;
        if (hipHostGetDevicePointer(&dev, c->h_state, 0) == hipSuccess && dev) d_state = (const PairState*)dev;
    }
    if (d_state == (const PairState*)c->state.p)
        HIPCHK(c, hipMemcpyAsync(c->state.p, hs, (size_t)pl.npairs * sizeof(PairState), hipMemcpyHostToDevice, c->stream));
    c->last_state_dev = d_state;
    // The candidate batch of a registration (pairs sharing ONE small target, all of one size): sweep + sums + publication in a
    // single launch per pass (kss_kernels.hip: cand_pass_kernel).  KSS_CAND_FUSED=0: sweep + reduce as before (A/B; the two
    // forms agree on every correspondence, their sums differ in the order of additions).
    static const bool cand_fused = getenv("KSS_CAND_FUSED") == nullptr || atoi(getenv("KSS_CAND_FUSED")) != 0;
    if (cand_fused && pl.shared_target && pl.npairs > 1 && !pl.src_in_cell_order && pl.g[0].tgt_pad <= 8192) {
        bool same = true;
        for (int p = 1; p < pl.npairs; ++p) same = same && pl.g[p].ns == pl.g[0].ns && pl.g[p].src_base == (int64_t)p * pl.g[0].ns;
        const int bpp = cand_pass_blocks_per_pair(pl.g[0].ns);
        if (same && ensure_zeroed(c, c->partials, (size_t)pl.npairs * bpp * NSUMS * sizeof(Granule)) == KSS_OK) {
            bool launched;
            {
                ProfScope ps(c, KSS_K_NN_SWEEP);
                launched = launch_cand_pass(c->stream, fma, pl.npairs, d_state, d_in, d_out, (const float4*)c->tgt4.p + pl.g[0].tgt_base, pl.g[0].tgt_pad,
                                            (int)pl.g[0].ns, max_d2, (Granule*)c->partials.p, c->h_seq_dev, c->seq + 1, d_idx_out, d_d2_out);
            }
            if (launched) {
                ++c->seq;
                HIPCHK(c, hipGetLastError());
                KCHK(wait_seq(c, pl.npairs, c->seq, active));
                return KSS_OK;
            }
        }
    }
    KCHK(stage_tables(c, pl));
    {
        ProfScope ps(c, KSS_K_NN_SWEEP);
        launch_nn_sweep(c->stream, pl.S, fma, (const NNWork*)c->nn_work.p, (int)pl.nn.size(), d_state,
                        d_in, d_out, (const float4*)c->tgt4.p, (unsigned long long*)c->keys.p);
    }
    const bool spin = pl.npairs <= PUB_PAIRS;
    {
        ProfScope ps(c, KSS_K_CORR_REDUCE);
        if (spin) {   // small batch: the reduce also adds each pair's rows up and publishes
            launch_corr_reduce_publish(c->stream, (const RedWork*)c->red_work.p, (int)pl.red.size(), d_state,
                                       d_out, (const float4*)c->tgt4.p, (const unsigned long long*)c->keys.p, max_d2,
                                       (Granule*)c->partials.p, d_idx_out, d_d2_out, pl.src_in_cell_order ? 1 : 0,
                                       (const PairRed*)c->pair_red.p, c->h_seq_dev, ++c->seq);
        } else {
            launch_corr_reduce(c->stream, (const RedWork*)c->red_work.p, (int)pl.red.size(), d_state,
                               d_out, (const float4*)c->tgt4.p, (const unsigned long long*)c->keys.p, max_d2,
                               (double*)c->partials.p, d_idx_out, d_d2_out, pl.src_in_cell_order ? 1 : 0);
            launch_finalize_sums(c->stream, (const PairRed*)c->pair_red.p, pl.npairs, (const double*)c->partials.p, (double*)c->h_sums_dev);
        }
    }
    HIPCHK(c, hipGetLastError());
    if (c->defer_wait) return KSS_OK;   // (pairs_loop: its own launches follow on the stream, it synchronises once behind them)
    if (spin) KCHK(wait_seq(c, pl.npairs));
    else HIPCHK(c, hipStreamSynchronize(c->stream));
    return KSS_OK;
}

// One NN pass (search + correspondence sums) over every active pair.  h_sums receives npairs*NSUMS.
// full: all 20 sums (the fitness / PCR_QM pass, traced runs); otherwise slots 17 and 18 stay 0 (an ICP iteration never
// reads them: one f64 sqrt per source and two reduction columns less).  active: which pairs take part (null: all).
static int nn_pass(kss_ctx* c, const IcpPlan& pl, bool fma, const float4* d_in, float4* d_out, double max_d2,
            int32_t* d_idx_out, float* d_d2_out, bool full, const int* active = nullptr) {
    if (pl.grid) return nn_pass_grid(c, pl, fma, d_in, d_out, max_d2, d_idx_out, d_d2_out, full);
    if (pl.gridb) return nn_pass_gridb(c, pl, fma, d_in, d_out, max_d2, d_idx_out, d_d2_out, full, active);
    return nn_pass_brute(c, pl, fma, d_in, d_out, max_d2, d_idx_out, d_d2_out, active);
}

static void set_state(PairState& s, const float T[16], int active, int apply) {
    for (int k = 0; k < 12; ++k) s.m[k] = T[k];
    s.active = active; s.apply = apply; s.pad[0] = s.pad[1] = 0;
}
// ... and its mirror in fine-grained device memory (large-BAR systems, batched cell lists): the workgroups of the next pass
// read their pair's state from device memory, the host having stored it there directly -- no copy operation, no PCIe read
// per workgroup.  Write-only on the host side (a host READ through the BAR costs microseconds).
static inline void mirror_state(PairState* bar, int p, const PairState& s) {
    if (!bar) return;
    const __m128i* v = reinterpret_cast<const __m128i*>(&s);
    __m128i* d = reinterpret_cast<__m128i*>(bar + p);
    for (int k = 0; k < 4; ++k) _mm_store_si128(d + k, _mm_loadu_si128(v + k));
}

// ---- what every ICP loop below shares ----
static inline Convergence convergence_of(const kss_icp_params& P) {   // PCL's criteria as kss_icp_params states them
    Convergence cv;
    cv.max_iterations = P.max_iterations;
    cv.rotation_threshold = 1.0 - P.transformation_epsilon;
    cv.translation_threshold = P.transformation_epsilon;
    cv.mse_rel = P.euclidean_fitness_epsilon;
    cv.mse_abs = P.abs_mse_epsilon;
    cv.fixed_iterations = P.fixed_iterations != 0;
    return cv;
}
// one row of the caller's trace: the pass's sums (ncol of them), its T_k and, for a trimmed pass, its {m, k, tau, kept}
static inline void trace_row(const kss_icp_params& P, const double* s, int ncol, const float* tk, double* trace_info = nullptr,
                             const double* info = nullptr, int ninfo = KSS_TRIM_NINFO) {
    if (!P.trace_n || *P.trace_n >= P.trace_cap) return;
    if (P.trace_sums) std::memcpy(P.trace_sums + (size_t)(*P.trace_n) * ncol, s, (size_t)ncol * sizeof(double));
    if (P.trace_Tk) std::memcpy(P.trace_Tk + (size_t)(*P.trace_n) * 16, tk, 16 * sizeof(float));
    if (trace_info) std::memcpy(trace_info + (size_t)(*P.trace_n) * ninfo, info, (size_t)ninfo * sizeof(double));
    ++*P.trace_n;
}
static inline void fill_result(kss_icp_result& r, const float fin[16], int iterations, int converged, int state, double last_mse,
                               double fitness, int pair) {
    std::memcpy(r.T, fin, 16 * sizeof(float));
    r.iterations = iterations; r.converged = converged; r.state = state;
    r.last_mse = last_mse; r.fitness = fitness; r.pair_id = pair;
}
// What the host does for ONE pair after a pass, in every loop below (icp_loop, resident_loop, pairs_loop): the
// min_correspondences test, the solve by metric (a default PairMode: the plain point metric, info unused), final <- T_k * final,
// the MSE and PCL's criteria.  s: the pass's record, info: its {m, k, tau, kept} (trimmed).  True: the pair goes on, t.tk is what
// the next NN pass applies on load; false: it has ended (state / converged say how).  What the engine is told is the caller's.
// trace: the pair whose passes the caller's trace receives (pair 0).
struct PairTrack {
    Convergence cv;
    float fin[16], tk[16];
    int iters = 0, state = KSS_STATE_NOT_CONVERGED, converged = 0;
    double last_mse = 0.0;
    double s_acc = 1.0;   // similarity: the scale accumulated so far
    explicit PairTrack(const kss_icp_params& P) : cv(convergence_of(P)) { mat4_identity(fin); mat4_identity(tk); }
};
static int pair_ninfo(const PairMode& M) { return M.sim ? KSS_SIM_NINFO : M.mutual ? KSS_RECIP_NINFO : M.unique ? KSS_O2O_NINFO : KSS_TRIM_NINFO; }
static_assert(KSS_O2O_NINFO <= KSS_SIM_NINFO && KSS_RECIP_NINFO <= KSS_SIM_NINFO, "the loops' info arrays hold KSS_SIM_NINFO doubles");
static bool pair_host_step(const kss_icp_params& P, const PairMode& M, const double* s, double* info, PairTrack& t, bool trace) {
    if (M.sim) { info[4] = 0.0; info[5] = t.s_acc; }
    // PCL: "Not enough correspondences found" (robust: the count kept, [0] being the weight total)
    const double cnt = M.robust ? s[(M.plane ? P2L_NSUMS : NSUMS) - 1] : s[0];
    if ((int)cnt < P.min_correspondences) { t.state = KSS_STATE_NO_CORRESPONDENCES; return false; }
    float ck[16];                 // similarity: the step without its scale, what the criteria read
    const float* crit = t.tk;
    double scale_dev2 = 0.0;
    if (M.symm) {
        if (!rigid_from_symm_sums(s, t.tk)) { t.state = KSS_STATE_DEGENERATE; return false; }
    } else if (M.plane) {
        if (!rigid_from_p2l_sums(s, t.tk)) { t.state = KSS_STATE_DEGENERATE; return false; }
    } else if (M.sim) {
        double sk;
        if (!sim_from_sums(s, M.scale_min / t.s_acc, M.scale_max / t.s_acc, t.tk, &sk, ck)) { t.state = KSS_STATE_DEGENERATE; return false; }
        t.s_acc = std::fmin(std::fmax(t.s_acc * sk, M.scale_min), M.scale_max);
        info[4] = sk; info[5] = t.s_acc;
        scale_dev2 = (sk - 1.0) * (sk - 1.0);
        crit = ck;
    } else {
        rigid_from_sums(s, t.tk);
    }
    mat4_mul(t.tk, t.fin, t.fin);   // final = transformation_ * final
    ++t.iters;
    const double mse = (M.plane ? s[28] : s[16]) / s[0];   // point-to-point d2 of the kept correspondences, as PCL's criteria read it
    t.last_mse = mse;
    if (trace) trace_row(P, s, M.plane ? P2L_NSUMS : NSUMS, t.tk, M.trimmed || M.robust ? M.trace_info : nullptr, info, pair_ninfo(M));
    const bool done = t.cv.has_converged(t.iters, crit, mse, scale_dev2);
    t.state = t.cv.state;
    if (done) t.converged = 1;
    return !done;
}
// pair 0's correspondences of the fitness pass into the caller's arrays
static int fitness_corr_out(kss_ctx* c, const kss_icp_params& P, const int32_t* d_idx, const float* d_d2, size_t n0) {
    if (P.fitness_idx) HIPCHK(c, hipMemcpyAsync(P.fitness_idx, d_idx, n0 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (P.fitness_d2) HIPCHK(c, hipMemcpyAsync(P.fitness_d2, d_d2, n0 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return KSS_OK;
}
// getFitnessScore(): NN of final * ORIGINAL input, mean d2 over ALL source points of each pair, into results[p].fitness.
// tr: per pair, as the loop left it.  claim_last: the plan is the one every pass of the loop ran on.
// d_idx / d_d2 (pl.total_src each; null: not wanted): the pass's correspondences by original source index, pair 0's copied to
// P.fitness_idx / P.fitness_d2.
static int fitness_pass(kss_ctx* c, const IcpPlan& pl, const kss_icp_params& P, const PairTrack* tr, bool claim_last,
                        PairState* bar, int32_t* d_idx, float* d_d2, kss_icp_result* results) {
    const int np = pl.npairs;
    PairState* hs = (PairState*)c->h_state;
    // (pad[0]: which work buffer holds the positions of the pair's last pass -- pass k writes cur[k & 1] -- so that the
    // cell-list pass can measure how far each source is from where its skip state was last brought up to date)
    const bool claim = claim_last && (pl.grid || pl.gridb);
    for (int p = 0; p < np; ++p) {
        set_state(hs[p], tr[p].fin, 1, 1);
        // (a pair that ended without correspondences, or on a singular system, took part in one more pass than it counted: its
        // last position is in the other buffer -- no claim is made for it, its sources simply search)
        if (claim && tr[p].iters >= 1 && tr[p].state != KSS_STATE_NO_CORRESPONDENCES && tr[p].state != KSS_STATE_DEGENERATE)
            hs[p].pad[0] = 1 + ((tr[p].iters - 1) & 1);
        mirror_state(bar, p, hs[p]);
    }
    c->fit_last = claim;
    struct FitGuard { kss_ctx* c; ~FitGuard() { c->fit_last = false; } } fit_guard{c};
    c->gated.want_next = false;
    KCHK(nn_pass(c, pl, P.nn_fma != 0, (const float4*)c->src0.p, (float4*)c->cur[0].p, P.max_corr_dist * P.max_corr_dist, d_idx, d_d2, true));
    const double* hsum = (const double*)c->h_sums;
    if (P.allreduce) {   // mean over ALL source rows of the job
        double v[2] = {hsum[17], (double)pl.g[0].ns};
        if (P.allreduce(P.allreduce_user, v, 2) != 0) return set_err(c, KSS_ERR_RCCL, "icp: the allreduce callback failed");
        results[0].fitness = v[0] / v[1];
    } else {
        for (int p = 0; p < np; ++p) results[p].fitness = hsum[(size_t)p * NSUMS + 17] / (double)pl.g[p].ns;
    }
    if (d_idx) KCHK(fitness_corr_out(c, P, d_idx, d_d2, (size_t)pl.g[0].ns));
    return KSS_OK;
}

// ---- the pair-resident engine (kss_resident.hip), host side ------------------------------------------------------------
// One launch runs every registration of the batch, one workgroup per pair; the host's part of an ICP iteration -- 20 sums in,
// 3x3 SVD, convergence tests, transform out -- is served per PAIR as its sums land, by a few threads that each own an
// interleaved share of the pairs (workgroups start roughly in pair order, so the pairs in flight spread over all threads).
// Every pair is solved by exactly one thread with the code of the launch-per-pass loop: same results.
// Gate records live in fine-grained device memory the host stores into through the BAR (large-BAR systems only; otherwise
// the launch-per-pass engine runs).  KSS_RESIDENT=0 switches the engine off (A/B; the engines agree bit for bit).
static bool resident_capacities(const IcpPlan& pl, int* ntc_out, int* tabc_out) {
    int64_t max_nt = 0;
    for (int p = 0; p < pl.npairs; ++p) {
        if (pl.g[p].ns > (int64_t)RES_SMAX * RES_THREADS || pl.g[p].nt > 65534) return false;   // (positions are 16 bits, 0xffff: none)
        max_nt = std::max(max_nt, pl.g[p].nt);
    }
    const int ntc = (int)((max_nt + 3 + 63) / 64 * 64);   // (+3: an evaluation step reads four points)
    const int64_t avail = ((int64_t)RES_LDS_MAX - (int64_t)resident_lds_bytes(ntc, 0)) / 2 / 8 * 8;   // table entries that still fit
    if (avail < 16) return false;
    int64_t want = 16;
    for (int p = 0; p < pl.npairs; ++p) {
        const GridParams& gp = pl.gpairs[p].gp;
        const int64_t rows = (int64_t)gp.gy * gp.gz;
        int xs = 0;
        while (xs <= 8 && rows * (((gp.gx + (1 << xs) - 1) >> xs) + 1) > avail) ++xs;   // x resolution of the table halves until it fits
        if (xs > 8) return false;
        want = std::max(want, rows * (((gp.gx + (1 << xs) - 1) >> xs) + 1));
    }
    *ntc_out = ntc;
    *tabc_out = (int)((want + 7) / 8 * 8);
    return true;
}

// workgroups of candidate-resident launches in flight, per device, over all contexts of the process
static std::atomic<int> g_cand_in_flight[64];
struct CandReservation {
    int dev = -1, n = 0;
    bool take(int device, int want, int cap) {
        if (device < 0 || device >= 64 || n != 0) return false;
        const int before = g_cand_in_flight[device].fetch_add(want);
        if (before + want > cap) { g_cand_in_flight[device].fetch_sub(want); return false; }
        dev = device; n = want;
        return true;
    }
    ~CandReservation() { if (n > 0) g_cand_in_flight[dev].fetch_sub(n); }
};

// ---- the two launches of the resident engines.  Each fills what the serving loop needs to know about the launch, whichever
// kernel it is; launched == false with KSS_OK: declined (the plan does not qualify, or the launch failed): nothing touched ----
struct ResLaunch {
    bool launched = false;
    unsigned long long seq0 = 0; unsigned stamp0 = 0;
    int32_t* idx_out = nullptr; float* d2_out = nullptr;
    unsigned long long* stamps = nullptr;   // diagnostic timeline (KSS_GRID_STAMPS: tools/resident_stamps.py, tools/cand_stamps.py)
    unsigned int* gate = nullptr;
};
// the launch's numbers, the correspondence buffers if the caller wants them, the stamp buffer: once nothing can decline any more
static int resident_launch_prepare(kss_ctx* c, const IcpPlan& pl, const kss_icp_params& P, int max_passes, ResLaunch& a) {
    a.seq0 = c->seq + 1;
    c->seq += (unsigned long long)max_passes + 1;
    c->res_launches = c->res_launches % 500000u + 1u;
    a.stamp0 = c->res_launches * 4096u;          // every launch has its own 4096 stamps: a record of an earlier launch never matches
    if (P.compute_fitness && (P.fitness_idx || P.fitness_d2)) {
        KCHK(ensure(c, c->stage_idx, (size_t)pl.total_src * sizeof(int32_t)));
        KCHK(ensure(c, c->stage_d2, (size_t)pl.total_src * sizeof(float)));
        a.idx_out = (int32_t*)c->stage_idx.p; a.d2_out = (float*)c->stage_d2.p;
    }
    static const bool stamps_on = getenv("KSS_GRID_STAMPS") != nullptr;
    if (stamps_on) {
        KCHK(ensure(c, c->g_stamps, (size_t)pl.npairs * 16 * sizeof(unsigned long long)));
        HIPCHK(c, hipMemsetAsync(c->g_stamps.p, 0, (size_t)pl.npairs * 16 * sizeof(unsigned long long), c->stream));
        a.stamps = (unsigned long long*)c->g_stamps.p;
    }
    return KSS_OK;
}

// batched cell lists: one workgroup per pair.  ra stays with the caller for the second launch of a split batch.
// A batch of more pairs than the device runs at once ends with a tail: 1024 uneven registrations on 256 compute units take
// 6.5 ms for 4.8 ms of work per unit (a tenth of C3's pairs keep hundreds of searches per pass going and run twice as long;
// whichever of them starts last is the kernel's end).  Such a batch runs as TWO launches: every pair's passes 0 .. split_at - 1
// (default: passes 0 and 1 -- the first, where every source searches, is the same work for every pair), then the rest with
// the pairs in the order of DECREASING cost as the first launch predicts it -- longest first, the classic rule for this
// scheduling problem.  The predictor: the searches the pair asked for in pass 1 (its exit flag carries the count): a pair
// that is still moving then keeps moving, and searching, for the passes to come.  (With pass 0 alone in the first launch the
// host orders by the mean squared distance of the first correspondences instead: on C3 as good -- 6.53 vs 6.59 ms -- but by
// accident: that distance saturates at the point spacing, the long pairs are those rotated by 2-4 degrees, one to two
// spacings, which creep for all twenty passes, and they merely end up in the middle of that order.  The size of the first
// ICP step predicts nothing: 7.4.)  Measured at C3 (ms per batch): one launch 7.39-7.45; split after pass 0: 6.51-6.64,
// after pass 1: 6.59-6.66, 2: 6.83, 3: 7.05, 5: 7.15, 7: 7.63.  Between the launches a pair's registers rest in memory (20 bytes per source).
// Same passes, same host protocol, same bits.  KSS_RESIDENT_SPLIT=0: one launch (A/B); =k: split after pass k - 1.
static int resident_launch_cells(kss_ctx* c, const IcpPlan& pl, const kss_icp_params& P, int max_passes, ResArgs& ra, int* split_at, ResLaunch& a) {
    const int np = pl.npairs;
    static const int split_env = getenv("KSS_RESIDENT_SPLIT") ? atoi(getenv("KSS_RESIDENT_SPLIT")) : 2;
    int ntc = 0, tabc = 0;
    if (!resident_capacities(pl, &ntc, &tabc)) return KSS_OK;
    a.gate = (unsigned int*)bar_ensure(c, c->res_gate, (size_t)np * 128);   // one 128-byte gate record per pair
    if (!a.gate) return KSS_OK;
    if (split_env > 0 && np >= 2 * resident_rows_limit(c) && P.max_iterations >= split_env + 4 &&
        ensure(c, c->res_pos, (size_t)pl.total_src * sizeof(float4)) == KSS_OK && ensure(c, c->res_wc, (size_t)pl.total_src * sizeof(unsigned)) == KSS_OK &&
        ensure(c, c->res_perm, (size_t)np * sizeof(int32_t)) == KSS_OK)
        *split_at = split_env;
    KCHK(resident_launch_prepare(c, pl, P, max_passes, a));
    ra.pairs = (const GridPairDev*)c->g_pairs.p;
    ra.cell_start = (const int32_t*)c->g_start.p + 1;
    ra.sorted = (const float4*)c->g_sorted.p;
    ra.src0 = (const float4*)c->src0.p;
    ra.gate = a.gate;
    ra.pub = c->h_seq_dev;
    ra.exit_flags = c->h_seq_dev + (size_t)2 * NSUMS * np;
    ra.max_passes = max_passes;
    ra.seq0 = a.seq0; ra.stamp0 = a.stamp0;
    ra.exit_tag = a.stamp0;
    ra.split_at = *split_at;
    ra.st_pos = (float4*)c->res_pos.p; ra.st_wc = (unsigned*)c->res_wc.p;
    ra.max_d2 = P.max_corr_dist * P.max_corr_dist;
    ra.skin = skin_setting();
    ra.gate_polls = gate_polls_setting();
    ra.full_always = P.trace_sums != nullptr ? 1 : 0;
    ra.ntc = ntc; ra.tabc = tabc;
    ra.idx_out = a.idx_out; ra.d2_out = a.d2_out;
    ra.stamps = a.stamps;
    ProfScope ps(c, KSS_K_RESIDENT, true);
    std::string lerr;
    if (launch_resident(c->stream, P.nn_fma != 0, np, ra, lerr) != KSS_OK) (void)hipGetLastError();   // (not launched: nothing touched, the other engine runs)
    else a.launched = true;
    return KSS_OK;
}

// candidates of one registration: equal sizes, packed one after the other, original order (what cand_pass_kernel asks
// for), and the whole launch resident at once -- up to CAND_TPW tiles of 32 sources per workgroup.  reserve: the caller's, given
// back only after the kernel has drained.
static int resident_launch_cands(kss_ctx* c, const IcpPlan& pl, const kss_icp_params& P, int max_passes, CandReservation& reserve, ResLaunch& a) {
    const int np = pl.npairs;
    for (int p = 0; p < np; ++p)
        if (pl.g[p].ns != pl.g[0].ns || pl.g[p].src_base != (int64_t)p * pl.g[0].ns) return KSS_OK;
    const int nt_pad = (int)pl.g[0].tgt_pad;
    const bool fma = P.nn_fma != 0;
    if (c->cand_cap_pad != nt_pad || c->cand_cap_fma != (fma ? 1 : 0)) {
        c->cand_cap = cand_resident_capacity(fma, nt_pad);
        c->cand_cap_pad = nt_pad; c->cand_cap_fma = fma ? 1 : 0;
    }
    // Every workgroup of the launch has to be on the chip at once, and so do those of the launches other contexts of this
    // process (the workers of kss_register_batch) have in flight on the same device: each launch RESERVES its workgroups
    // out of the device's capacity, takes more tiles per workgroup when little is left, and goes to the launch-per-pass
    // form when that is not enough.  (KSS_CAND_CAP: a smaller capacity, to exercise exactly that.)
    static const int cap_env = getenv("KSS_CAND_CAP") ? atoi(getenv("KSS_CAND_CAP")) : 0;
    const int cap = cap_env > 0 ? std::min(c->cand_cap, cap_env) : c->cand_cap;
    const int bpp = cand_pass_blocks_per_pair(pl.g[0].ns);
    if (cap <= 0 || bpp <= 0) return KSS_OK;
    int tpw = 0;
    for (int t = 1; t <= CAND_TPW && !tpw; ++t) {
        const int want_wg = np * ((bpp + t - 1) / t);
        if (want_wg > cap) continue;
        if (reserve.take(c->device, want_wg, cap)) tpw = t;
    }
    if (!tpw) return KSS_OK;
    a.gate = (unsigned int*)bar_ensure(c, c->res_gate, (size_t)np * 128);   // one 128-byte gate record per pair
    if (!a.gate) return KSS_OK;
    if (ensure_zeroed(c, c->partials, (size_t)np * bpp * NSUMS * sizeof(Granule)) != KSS_OK) return KSS_OK;
    KCHK(resident_launch_prepare(c, pl, P, max_passes, a));
    CandArgs ca;
    std::memset(&ca, 0, sizeof ca);
    ca.src0 = (const float4*)c->src0.p;
    ca.tgt = (const float4*)c->tgt4.p + pl.g[0].tgt_base;
    ca.nt_pad = nt_pad; ca.ns = (int)pl.g[0].ns;
    ca.bpp = bpp; ca.tpw = tpw; ca.wpp = (bpp + tpw - 1) / tpw;
    ca.max_d2 = P.max_corr_dist * P.max_corr_dist;
    ca.rows = (Granule*)c->partials.p;   // (zeroed when (re)allocated: no granule of the block's earlier owner; pass numbers start at 1)
    ca.gate = a.gate;
    ca.pub = c->h_seq_dev;
    ca.exit_flags = c->h_seq_dev + (size_t)2 * NSUMS * np;
    ca.seq0 = a.seq0; ca.stamp0 = a.stamp0;
    ca.gate_polls = gate_polls_setting(); ca.max_passes = max_passes;
    ca.idx_out = a.idx_out; ca.d2_out = a.d2_out;
    ca.stamps = a.stamps;
    ProfScope ps(c, KSS_K_RESIDENT, true);
    std::string lerr;
    if (launch_cand_resident(c->stream, fma, np, ca, lerr) != KSS_OK) (void)hipGetLastError();
    else a.launched = true;
    return KSS_OK;
}

// ---- serving a resident launch: the per-pair host state (icp_loop's record and what the serving protocol adds), the launch's
// description, what the serving threads share, and the steps in resident_loop's order ----
enum { PH_ITER = 0, PH_FIT = 1, PH_DONE = 2 };
struct PairHost {
    PairTrack t;
    int k = 0, phase = PH_ITER, cancelled = 0, parked = 0;
    double fitness = 0.0;
    explicit PairHost(const kss_icp_params& P) : t(P) {}
};
struct ResidentServe {
    kss_ctx* const c; const IcpPlan& pl; const kss_icp_params& P; const bool cand;
    const int np;
    const ResLaunch a;
    ResArgs ra;                     // cell lists: the first launch's arguments, changed into the second's
    const int split_at;
    int split_now;                  // > 0 while the first launch of a split batch is being served
    unsigned exit_tag_now;
    std::vector<PairHost> H;
    std::vector<char> in_launch;
    const PairMode plain{};         // the untrimmed, unweighted point metric
    const int judge; const double judge_threshold;
    const unsigned long long* const h_seq;
    const unsigned long long* const exit_flags;   // one per pair, behind the launch's slots
    std::atomic<int> failed{0}, kernel_done{0}, pairs_left, cancel_all{0}, query_said{0};
    std::atomic<long long> units{0};
    std::atomic<long> sent{0};
    std::chrono::steady_clock::time_point last_progress;   // (the calling thread's alone)
    const int nthreads;             // of the first launch
    const long torn_at, stall_at;   // test hooks (resident_loop)

    ResidentServe(kss_ctx* c_, const IcpPlan& pl_, const kss_icp_params& P_, bool cand_, const ResLaunch& a_, const ResArgs& ra_, int split_at_, long torn_at_, long stall_at_)
        : c(c_), pl(pl_), P(P_), cand(cand_), np(pl_.npairs), a(a_), ra(ra_), split_at(split_at_), split_now(split_at_), exit_tag_now(a_.stamp0),
          H((size_t)pl_.npairs, PairHost(P_)), in_launch((size_t)pl_.npairs, 1), judge(cand_ ? c_->spec_judge : -1), judge_threshold(c_->spec_threshold),
          h_seq(c_->h_seq), exit_flags(c_->h_seq + (size_t)2 * NSUMS * pl_.npairs), pairs_left(pl_.npairs), nthreads(threads_for(pl_.npairs)), torn_at(torn_at_), stall_at(stall_at_) {
        if (P.trace_n) *P.trace_n = 0;
    }

    int threads_for(int pairs) const {
        static const int res_threads = [] {
            int v = (int)std::thread::hardware_concurrency();
            v = std::max(1, std::min(v, 12));
            if (const char* e = getenv("KSS_HOST_THREADS")) { const int u = atoi(e); if (u >= 1 && u <= 64) v = u; }
            return v;
        }();
        // (eight pairs a thread: one, two, four and eight candidates per thread were measured alike on a registration's 15 -- an
        // answer is a microsecond of host work -- and several registrations at once, kss_register_batch, must not bring more
        // spinning threads than the machine has cores)
        static const int cand_div = getenv("KSS_CAND_PAIRS_PER_THREAD") ? std::max(1, atoi(getenv("KSS_CAND_PAIRS_PER_THREAD"))) : 8;
        return std::max(1, std::min(res_threads, cand ? (pairs + cand_div - 1) / cand_div : (pairs + 7) / 8));
    }
    void run(int threads) { c->pool.run_threads(threads, [this](int t, int nt) { serve(t, nt); }); }

    // the gate record of pair p's NEXT pass (number H[p].k + 1); inlined: serve's answers are on every resident batch's critical path
    __attribute__((always_inline)) void send(int p, const float* T, int apply, int mode, bool any_pass = false) {
        unsigned w[15];
        if (T) std::memcpy(w, T, 12 * sizeof(float)); else std::memset(w, 0, 12 * sizeof(float));
        w[12] = 1u; w[13] = (unsigned)apply; w[14] = (unsigned)mode;
        // (any_pass: an order to stop that may land while some workgroups still wait for an EARLIER record -- one record per pair)
        const unsigned stamp = a.stamp0 + (any_pass ? RES_STAMP_ANY : (unsigned)(H[p].k + 1));
        const long nth = sent.fetch_add(1) + 1;
        if (nth == stall_at) std::this_thread::sleep_for(std::chrono::milliseconds(300));
        gate_record_store(a.gate + (size_t)p * 32, w, stamp, nth == torn_at);
    }

    void serve(int t, int nt) {
        if (t == 0) last_progress = std::chrono::steady_clock::now();
        int remaining = 0;
        for (int p = t; p < np; p += nt)
            if (H[p].phase != PH_DONE && !H[p].parked) ++remaining;
        long idle = 0, grace = 0;
        double s[NSUMS];
        long long my_units = 0;
        // (the calling thread stays until EVERY pair is done: it is the one that asks HIP whether the kernel is still there)
        while ((remaining > 0 || (t == 0 && pairs_left.load(std::memory_order_relaxed) > 0)) && !failed.load(std::memory_order_relaxed)) {
            bool progress = false;
            const bool cancelling = judge >= 0 && cancel_all.load(std::memory_order_relaxed) != 0;
            for (int p = t; p < np; p += nt) {
                PairHost& h = H[p];
                if (h.phase == PH_DONE || h.parked) continue;
                if (cancelling && p != judge) {
                    // the judge was good enough: this candidate's result will not be looked at.  Its workgroups are told to stop at
                    // whatever gate they reach next (some may be inside a pass the others will never join: rows carry the number of
                    // their launch and pass, nothing is left to clear); a candidate already on its last pass leaves by itself.
                    if (h.phase == PH_ITER) send(p, nullptr, 0, 2, true);
                    h.phase = PH_DONE; h.cancelled = 1; --remaining; pairs_left.fetch_sub(1, std::memory_order_relaxed);
                    progress = true;
                    continue;
                }
                if (!slots_collect(h_seq + (size_t)2 * NSUMS * p, NSUMS, a.seq0 + (unsigned long long)h.k, s)) continue;
                progress = true;
                ++my_units;
                if (h.phase == PH_FIT) {   // getFitnessScore(): mean d2 over ALL source points
                    h.fitness = s[17] / (double)pl.g[p].ns;
                    h.phase = PH_DONE; --remaining; pairs_left.fetch_sub(1, std::memory_order_relaxed);
                    if (p == judge && h.fitness <= judge_threshold) cancel_all.store(1, std::memory_order_relaxed);
                    continue;
                }
                if (pair_host_step(P, plain, s, nullptr, h.t, p == 0)) {
                    send(p, h.t.tk, 1, 0);                 // the next pass applies T_k on load (transformCloud)
                    ++h.k;
                } else if (P.compute_fitness) {
                    send(p, h.t.fin, 1, 1);                // final * original input, all 20 sums
                    ++h.k;
                    h.phase = PH_FIT;
                } else {
                    send(p, nullptr, 0, 2);
                    h.phase = PH_DONE; --remaining; pairs_left.fetch_sub(1, std::memory_order_relaxed);
                }
                // the first launch of a split batch: the pair's workgroup left after pass split_now - 1; the record just written
                // is what the pair's workgroup of the SECOND launch finds at its first gate
                if (split_now > 0 && h.phase != PH_DONE && h.k == split_now) {
                    h.parked = 1; --remaining; pairs_left.fetch_sub(1, std::memory_order_relaxed);
                }
            }
            if (progress) { idle = 0; grace = 0; if (t == 0) last_progress = std::chrono::steady_clock::now(); continue; }
            __builtin_ia32_pause();
            if (idle > 16384 && (idle & 1023) == 1023) std::this_thread::yield();   // (nothing for ~a millisecond and maybe more spinning threads than cores: let the others run; sooner, the call costs a large batch's answers their latency: C3 7.5 -> 8.2 ms)
            if (++idle % 4096 == 0) {
                // nothing for a while: has the kernel gone?  (Only the calling thread talks to HIP.)  A workgroup that was not
                // answered within its bounded poll has left; its pair will never publish.  After the kernel has ended every
                // result is in host memory already: a thread that still finds nothing for ~10 ms of polling gives up.
                if (t == 0 && !kernel_done.load()) kernel_gone();
                if (kernel_done.load() && ++grace > 64) failed.store(1);
            }
        }
        units.fetch_add(my_units);
    }

    // has the kernel gone?  Every pair's workgroups have stored their exit flag (no HIP call here: one can wait on locks that
    // other threads of the process hold for as long as THEIR kernels run -- and this thread has pairs to answer); after two
    // seconds of nothing, HIP is asked all the same: a faulted kernel sets no flags
    void kernel_gone() {
        bool gone = true;
        for (int p = 0; p < np && gone; ++p)
            if (in_launch[p]) gone = exit_flag_read(exit_flags, p, exit_tag_now, nullptr);
        if (gone) kernel_done.store(1);
        else if (std::chrono::duration<double>(std::chrono::steady_clock::now() - last_progress).count() > 2.0) {
            const hipError_t q = hipStreamQuery(c->stream);
            if (q != hipErrorNotReady) { query_said.store((int)q); kernel_done.store(1); }
            last_progress = std::chrono::steady_clock::now();
        }
    }

    // the second launch of a split batch: the parked pairs, longest first
    int second_launch() {
        HIPCHK(c, hipStreamSynchronize(c->stream));   // every workgroup of the first launch has left (its registers are in memory)
        // cost predictor: the searches the pair asked for in passes 1 .. split_at - 1 (its exit flag carries the count); with
        // only pass 0 in the first launch, or with KSS_RESIDENT_SPLIT_KEY=mse, the mean squared distance of its first correspondences
        static const bool key_mse = getenv("KSS_RESIDENT_SPLIT_KEY") != nullptr && std::string(getenv("KSS_RESIDENT_SPLIT_KEY")) == "mse";
        std::vector<std::pair<double, int>> order;
        for (int p = 0; p < np; ++p) {
            in_launch[p] = 0;
            if (!H[p].parked) continue;
            unsigned searches = 0;   // (every parked pair's flag is there and fits: kernel_gone has seen it, the stream is drained)
            exit_flag_read(exit_flags, p, a.stamp0, &searches);
            order.emplace_back(key_mse || split_at < 2 ? H[p].t.last_mse : (double)searches, p);
        }
        std::stable_sort(order.begin(), order.end(), [](const std::pair<double, int>& x, const std::pair<double, int>& y) { return x.first > y.first; });
        const int np2 = (int)order.size();
        if (np2 == 0) return KSS_OK;
        std::vector<int32_t> perm((size_t)np2);
        for (int i = 0; i < np2; ++i) { perm[i] = order[i].second; in_launch[order[i].second] = 1; H[order[i].second].parked = 0; }
        HIPCHK(c, hipMemcpyAsync(c->res_perm.p, perm.data(), (size_t)np2 * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));   // (pageable source)
        ra.perm = (const int32_t*)c->res_perm.p;
        ra.first_pass = split_at; ra.split_at = 0;
        ra.exit_tag = a.stamp0 + 1u;
        if (a.stamps) HIPCHK(c, hipMemsetAsync(c->g_stamps.p, 0, (size_t)np * 16 * sizeof(unsigned long long), c->stream));   // (the timeline of the SECOND launch)
        split_now = 0; exit_tag_now = ra.exit_tag;
        kernel_done.store(0); pairs_left.store(np2);
        {
            ProfScope ps(c, KSS_K_RESIDENT, true);
            std::string lerr;
            if (launch_resident(c->stream, P.nn_fma != 0, np2, ra, lerr) != KSS_OK) return set_err(c, KSS_ERR_HIP, "resident: the second launch of a split batch failed");
        }
        run(threads_for(np2));
        return KSS_OK;
    }

    // let every workgroup that still waits (or has not started yet) leave, then report: the caller starts over on the
    // launch-per-pass engine (the resident kernel has written nothing but its result slots -- and, for candidates, rows
    // that carry this launch's numbers)
    int give_up() {
        for (int p = 0; p < np; ++p)
            if (H[p].phase != PH_DONE) send(p, nullptr, 0, 2, true);
        HIPCHK(c, hipStreamSynchronize(c->stream));
        constexpr int backoff_s = 30;
        c->res_backoff[cand ? 1 : 0] = std::chrono::steady_clock::now() + std::chrono::seconds(backoff_s);   // not again for a while: each failure costs the polls' bound (~1 s)
        int unfinished = 0, k_min = 1 << 30, k_max = 0;
        for (int p = 0; p < np; ++p)
            if (H[p].phase != PH_DONE) { ++unfinished; k_min = std::min(k_min, H[p].k); k_max = std::max(k_max, H[p].k); }
        std::fprintf(stderr, "[kss] the pair-resident kernel left before every pair was finished (a stalled host thread?); running the launch-per-pass engine"
                             " (and for the next %d s on this context)"
                             " [%s, %d of %d pairs unfinished, waiting for passes %d..%d, %d host threads, stream query: %s]\n",
                     backoff_s, cand ? "candidates" : "cell lists", unfinished, np, k_min, k_max, nthreads, hipGetErrorName((hipError_t)query_said.load()));
        if (getenv("KSS_DEBUG_RES")) {   // what each unfinished pair was waiting for, and what is there
            for (int p = 0; p < np; ++p) {
                if (H[p].phase == PH_DONE) continue;
                const unsigned long long want = a.seq0 + (unsigned long long)H[p].k;
                std::fprintf(stderr, "[kss]   pair %d: phase %d, waiting for the sums of pass %d (seq %llu); slots hold seq:", p, H[p].phase, H[p].k, want & 0xffffffffull);
                const unsigned long long* sl = h_seq + (size_t)2 * NSUMS * p;
                for (int k = 0; k < NSUMS; ++k) std::fprintf(stderr, " %llu", sl[2 * k + 1] & 0xffffffffull);
                std::fprintf(stderr, "\n");
            }
        }
        return KSS_OK;
    }

    // results, the fitness pass's correspondences, the diagnostic timeline
    int finish(kss_icp_result* results) {
        HIPCHK(c, hipStreamSynchronize(c->stream));   // every workgroup has left (its last act was the publication just consumed)
        if (c->prof > 0) { c->prof_n[KSS_K_RESIDENT_PASS] += units.load(); }
        for (int p = 0; p < np; ++p) {
            const PairHost& h = H[p];   // (a cancelled candidate: its result will not be looked at)
            fill_result(results[p], h.t.fin, h.t.iters, h.cancelled ? 0 : h.t.converged, h.cancelled ? KSS_STATE_NOT_CONVERGED : h.t.state, h.t.last_mse,
                        P.compute_fitness && !h.cancelled ? h.fitness : 0.0, p);
        }
        if (judge >= 0) { c->spec_ran = true; c->spec_cancelled = cancel_all.load() != 0; }
        if (a.idx_out) KCHK(fitness_corr_out(c, P, a.idx_out, a.d2_out, (size_t)pl.g[0].ns));
        if (a.stamps) {
            c->last_stamps.resize((size_t)np * 16);
            HIPCHK(c, hipMemcpy(c->last_stamps.data(), a.stamps, c->last_stamps.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        }
        return KSS_OK;
    }
};

// *handled = false with KSS_OK: the plan does not qualify (or the engine gave up before touching any result): the caller
// runs the launch-per-pass loop
static int resident_loop(kss_ctx* c, const IcpPlan& pl, const kss_icp_params& P, kss_icp_result* results, bool* handled, bool cand = false) {
    *handled = false;
    static const bool want = getenv("KSS_RESIDENT") == nullptr || atoi(getenv("KSS_RESIDENT")) != 0;
    static const bool want_cand = getenv("KSS_CAND_RESIDENT") == nullptr || atoi(getenv("KSS_CAND_RESIDENT")) != 0;
    if (!(cand ? want_cand : want) || P.allreduce || P.max_iterations < 1 || P.max_iterations > 4000) return KSS_OK;
    if (cand ? (pl.grid || pl.gridb || !pl.shared_target || pl.src_in_cell_order || pl.g[0].tgt_pad > 8192) : !pl.gridb) return KSS_OK;
    if (std::chrono::steady_clock::now() < c->res_backoff[cand ? 1 : 0]) return KSS_OK;   // given up recently: ResidentServe::give_up
    const int max_passes = P.max_iterations + 2;
    CandReservation cand_reserve;   // (given back when this function returns: the kernel has drained by then on every path)
    ResLaunch a;
    int split_at = 0;
    ResArgs ra{};
    KCHK(cand ? resident_launch_cands(c, pl, P, max_passes, cand_reserve, a) : resident_launch_cells(c, pl, P, max_passes, ra, &split_at, a));
    if (!a.launched) return KSS_OK;
    // test hooks: the n-th record of the call first arrives torn (kss_handover.hpp); the n-th answer is held back for 300 ms (a
    // stalled host thread: with a small KSS_GATE_POLLS the workgroup leaves, and the call starts over on the other engine)
    static const long torn_at = getenv("KSS_TEST_TORN_RES_GATE") ? atol(getenv("KSS_TEST_TORN_RES_GATE")) : -1;
    static const long stall_at = getenv("KSS_TEST_RES_STALL") ? atol(getenv("KSS_TEST_RES_STALL")) : -1;
    ResidentServe S(c, pl, P, cand, a, ra, split_at, torn_at, stall_at);
    S.run(S.nthreads);
    if (split_at > 0 && !S.failed.load()) KCHK(S.second_launch());
    if (S.failed.load()) return S.give_up();
    KCHK(S.finish(results));
    *handled = true;
    return KSS_OK;
}

// Batched cell lists: slot 19 of a pair's sums counts the lanes that ended in the in-wave brute-force fallback.  When more
// than 10 % of the sources of the pairs that were active in the pass did (badly posed or partly overlapping pairs), the rest of
// the call runs on the brute-force engine, whose tiled sweep is several times faster at that job; the engines agree bit for
// bit on every correspondence, so the switch only changes speed.  The packed clouds stay where they are.  plan: the batched
// cell-list plan the pass ran on, replaced by brute_plan (built and staged here) when the rule fires.
static int switch_engine_on_fallback(kss_ctx* c, const IcpPlan*& plan, IcpPlan& brute_plan, const kss_icp_params& P,
                                     const std::vector<int>& was_active) {
    const int np = plan->npairs;
    const double* hsum = (const double*)c->h_sums;
    double fallback = 0.0, act = 0.0;
    for (int p = 0; p < np; ++p)
        if (was_active[p]) { fallback += hsum[(size_t)p * NSUMS + NSUMS - 1]; act += (double)plan->g[p].ns; }
    if (!(fallback > 0.10 * act) || getenv("KSS_GRID_NOSWITCH")) return KSS_OK;
    std::vector<int64_t> ns(np), nt(np);
    for (int p = 0; p < np; ++p) { ns[p] = plan->g[p].ns; nt[p] = plan->g[p].nt; }
    KCHK(build_plan(c, ns.data(), nt.data(), np, false, P.nn_sources_per_thread, P.nn_target_splits, KSS_NN_BRUTE, brute_plan));
    brute_plan.src_in_cell_order = true;
    KCHK(stage_plan(c, brute_plan));
    plan = &brute_plan;
    return KSS_OK;
}

// The ICP loop over a packed workspace (src0/tgt4 already filled).
static int icp_loop(kss_ctx* c, const IcpPlan& pl_in, const kss_icp_params& P, kss_icp_result* results) {
    if (pl_in.gridb) {   // batches whose pairs fit a CU each: one launch, every pair resident for its whole registration
        bool handled = false;
        KCHK(resident_loop(c, pl_in, P, results, &handled));
        if (handled) return KSS_OK;
    }
    if (!pl_in.grid && !pl_in.gridb && pl_in.shared_target) {   // the candidate batch of a registration: one launch, every workgroup resident
        bool handled = false;
        KCHK(resident_loop(c, pl_in, P, results, &handled, true));
        if (handled) return KSS_OK;
    }
    if (c->spec_judge >= 0) return KSS_OK;   // a speculative batch (kss_register) runs on that engine only: spec_ran stays false, the caller takes the sequential route
    const IcpPlan* plan = &pl_in;   // may change to the brute-force plan below
    IcpPlan brute_plan;
    const int np = pl_in.npairs;
    std::vector<PairTrack> tr((size_t)np, PairTrack(P));
    std::vector<int> active(np, 1), solved(np, 0), was_active;
    const PairMode plain;   // the untrimmed, unweighted point metric
    const bool full = P.trace_sums != nullptr;   // traced runs report all 20 sums of every pass
    PairState* hs = (PairState*)c->h_state;
    PairState* bar = pl_in.gridb ? (PairState*)bar_ensure(c, c->bar_state, (size_t)np * sizeof(PairState)) : nullptr;   // (null without a large BAR)
    float I[16];
    mat4_identity(I);
    for (int p = 0; p < np; ++p) {
        set_state(hs[p], I, 1, 0);
        mirror_state(bar, p, hs[p]);
    }
    const double max_d2 = P.max_corr_dist * P.max_corr_dist;
    const double* hsum = (const double*)c->h_sums;
    if (P.trace_n) *P.trace_n = 0;
    int n_active = P.max_iterations > 0 ? np : 0;
    if (P.max_iterations <= 0)
        for (int p = 0; p < np; ++p) { active[p] = 0; }
    int it = 0;
    GatedGuard gated_guard(c);

    // ---- per-pair solve + convergence test of the pairs [p0, p1) after a pass: pairs are independent (a large batch is
    // split over a few host threads; each pair is handled by exactly one thread with the serial code, so the results do
    // not depend on the split).  poll: the pass published per pair (batched cell lists) and the pairs are picked up as
    // their sums land, in launch order, while the rest of the launch is still running.  Returns the pairs that finished.
    auto solve_pairs = [&](int p0, int p1, unsigned long long pass_seq, bool poll_first, int* n_finished) -> int {
        std::atomic<int> finished{0}, stuck{0};
        bool poll = poll_first;
        std::fill(solved.begin() + p0, solved.begin() + p1, 0);
        auto solve = [&](int pb, int pe) {
            int fin_here = 0;
            for (int p = pb; p < pe; ++p) {
                if (!active[p] || solved[p]) continue;
                if (poll && wait_pair(c, p, pass_seq) != KSS_OK) { stuck.fetch_add(1); continue; }   // (retried below after a stream sync)
                PairTrack& t = tr[p];
                const bool goes_on = pair_host_step(P, plain, hsum + (size_t)p * NSUMS, nullptr, t, p == 0);
                solved[p] = 1;
                if (goes_on) {
                    set_state(hs[p], t.tk, 1, 1);   // next sweep applies T_k on load (transformCloud)
                } else {
                    active[p] = 0; ++fin_here;
                    if (t.state == KSS_STATE_NO_CORRESPONDENCES) set_state(hs[p], I, 0, 0);
                    else set_state(hs[p], t.tk, 0, 1);
                }
                mirror_state(bar, p, hs[p]);
            }
            finished.fetch_add(fin_here, std::memory_order_relaxed);
        };
        const int n = p1 - p0;
        if (n >= 64) {
            std::atomic<int> next{0};
            constexpr int kBlock = 64;   // pairs claimed at a time, in launch order: the first threads start while the GPU is still on later pairs.  Measured at C3: blocks of 4 pairs 11.7 ms (threads share cache lines of the per-pair records), 16: 9.85, 64: 9.5
            c->pool.parallel_for(n, [&](int, int) {
                for (;;) {
                    const int pb = p0 + next.fetch_add(1) * kBlock;
                    if (pb >= p1) break;
                    solve(pb, std::min(p1, pb + kBlock));
                }
            });
        } else {
            solve(p0, p1);
        }
        if (stuck.load() > 0) {   // a pair did not publish in time: synchronize (surfaces a faulted kernel), then finish the stragglers
            HIPCHK(c, hipStreamSynchronize(c->stream));
            for (int p = p0; p < p1; ++p) {
                if (!active[p] || solved[p]) continue;
                if (!collect_pair(c, p, pass_seq)) return set_err(c, KSS_ERR_HIP, "kernel finished without publishing its result");
            }
            poll = false;        // their sums are in h_sums now
            solve(p0, p1);       // (pairs already solved in this pass are skipped)
        }
        *n_finished = finished.load(std::memory_order_relaxed);
        return KSS_OK;
    };

    while (n_active > 0) {
        const float4* d_in = it == 0 ? (const float4*)c->src0.p : (const float4*)c->cur[(it - 1) & 1].p;
        float4* d_out = (float4*)c->cur[it & 1].p;
        // (cancelled if this iteration converges; never with an all-reduce callback: its collective would queue up on
        // this stream BEHIND the polling kernel, whose transform depends on it)
        c->gated.want_next = plan->grid && !P.allreduce && it + 1 < P.max_iterations;
        c->gated.want_full = full;
        c->gated.max_steps = P.max_iterations - (it + 1);
        // batched cell lists: the solve loop picks each pair up as its sums land -- while the rest of the launch is still
        // running where the pairs' first workgroups add their rows up in the pass (at most one pair per compute unit)
        c->defer_wait = plan->gridb;
        const auto tb0 = c->timing ? std::chrono::steady_clock::now() : std::chrono::steady_clock::time_point();
        const int rc_pass = nn_pass(c, *plan, P.nn_fma != 0, d_in, d_out, max_d2, nullptr, nullptr, full, active.data());
        const bool deferred = c->defer_wait;
        c->defer_wait = false;
        const auto tb1 = c->timing ? std::chrono::steady_clock::now() : std::chrono::steady_clock::time_point();
        KCHK(rc_pass);
        const unsigned long long pass_seq = c->seq;
        // source rows split over ranks: the sums of all ranks, identical on every rank from here on
        if (P.allreduce && P.allreduce(P.allreduce_user, (double*)c->h_sums, NSUMS) != 0)
            return set_err(c, KSS_ERR_RCCL, "icp: the allreduce callback failed");
        if (plan->gridb) was_active = active;   // the fallback statistics of this pass need the pairs that were active when it ran
        int fin_now = 0;
        KCHK(solve_pairs(0, np, pass_seq, deferred, &fin_now));
        if (c->timing && deferred) {   // batch: time to enqueue the pass vs time until every pair was solved
            const auto tb2 = std::chrono::steady_clock::now();
            c->t_launch_us += std::chrono::duration<double, std::micro>(tb1 - tb0).count();
            c->t_wait_us += std::chrono::duration<double, std::micro>(tb2 - tb1).count();
        }
        if (plan->gridb) KCHK(switch_engine_on_fallback(c, plan, brute_plan, P, was_active));
        n_active -= fin_now;
        ++it;
    }
    for (int p = 0; p < np; ++p) fill_result(results[p], tr[p].fin, tr[p].iters, tr[p].converged, tr[p].state, tr[p].last_mse, 0.0, p);
    if (!P.compute_fitness) return KSS_OK;
    int32_t* d_idx = nullptr;
    float* d_d2 = nullptr;
    if (P.fitness_idx || P.fitness_d2) {   // per-source correspondences of the fitness pass
        KCHK(ensure(c, c->stage_idx, (size_t)plan->total_src * sizeof(int32_t)));
        KCHK(ensure(c, c->stage_d2, (size_t)plan->total_src * sizeof(float)));
        d_idx = (int32_t*)c->stage_idx.p; d_d2 = (float*)c->stage_d2.p;
    }
    return fitness_pass(c, *plan, P, tr.data(), plan == &pl_in, bar, d_idx, d_d2, results);
}

// zero-at-rest buffers (kss_ctx.hpp): cleared here when the previous call on this context did not finish
static int restore_zero_at_rest(kss_ctx* c) {
    if (!c->ws_dirty) return KSS_OK;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (DevBuf* b : {&c->g_count, &c->g_counts})
        if (b->p) HIPCHK(c, hipMemsetAsync(b->p, 0, b->cap, c->stream));
    c->ws_dirty = false;
    return KSS_OK;
}
struct DirtyGuard {   // a call that returns early leaves the zero-at-rest buffers in an unknown state
    kss_ctx* c; bool ok = false;
    explicit DirtyGuard(kss_ctx* c_) : c(c_) {}
    ~DirtyGuard() { if (!ok) c->ws_dirty = true; }
};

int icp_run_dev(kss_ctx* c, const void* d_src, const int64_t* src_off, const void* d_tgt, const int64_t* tgt_off,
                int npairs, bool shared_target, int dtype, const kss_icp_params* p, kss_icp_result* results) {
    if (!c || !d_src || !d_tgt || !src_off || !tgt_off || !p || !results || npairs <= 0) return set_err(c, KSS_ERR_ARG, "icp: bad argument");
    if (p->allreduce && npairs != 1) return set_err(c, KSS_ERR_ARG, "icp: the source-row split (allreduce) is for a single pair");
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<int64_t> ns(npairs), nt(npairs);
    for (int i = 0; i < npairs; ++i) {
        ns[i] = src_off[i + 1] - src_off[i];
        nt[i] = shared_target ? tgt_off[1] - tgt_off[0] : tgt_off[i + 1] - tgt_off[i];
    }
    IcpPlan pl;
    const auto t0 = std::chrono::steady_clock::now();
    KCHK(restore_zero_at_rest(c));
    DirtyGuard guard(c);
    c->timing = getenv("KSS_TIMING") != nullptr;
    auto lap = [&](const char* what, std::chrono::steady_clock::time_point& from) {   // KSS_TIMING: host time of each setup stage
        if (!c->timing) return;
        const auto now = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[kss]   %s %.1f us\n", what, std::chrono::duration<double, std::micro>(now - from).count());
        from = now;
    };
    auto ts = t0;
    KCHK(build_plan(c, ns.data(), nt.data(), npairs, shared_target, p->nn_sources_per_thread, p->nn_target_splits, p->nn_mode, pl));
    lap("plan", ts);
    KCHK(stage_plan(c, pl));
    lap("stage", ts);
    KCHK(pack_clouds(c, pl, d_src, src_off, d_tgt, tgt_off, dtype));
    lap("pack (enqueue)", ts);
    KCHK(grid_setup(c, pl));
    KCHK(grid_setup_batch(c, pl));
    lap("cell lists (bbox sync + enqueue)", ts);
    if (c->timing) HIPCHK(c, hipStreamSynchronize(c->stream));   // (only to split setup from loop in the KSS_TIMING report)
    lap("drain", ts);
    const auto t1 = std::chrono::steady_clock::now();
    c->t_launch_us = c->t_wait_us = 0;
    const int rc = icp_loop(c, pl, *p, results);
    guard.ok = rc == KSS_OK;
    const auto t2 = std::chrono::steady_clock::now();
    c->last_setup_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
    c->last_loop_ms = std::chrono::duration<double, std::milli>(t2 - t1).count();
    if (c->timing)
        std::fprintf(stderr, "[kss] setup %.3f ms, loop+fitness %.3f ms (fused launches: enqueue %.1f us, wait %.1f us, rest = host math)\n",
                     c->last_setup_ms, c->last_loop_ms, c->t_launch_us, c->t_wait_us);
    return rc;
}

// ---- one pair with a metric or a selection the chained point-to-point path does not have: kss_icp_p2l (plane, untrimmed),
// kss_icp_trimmed (point or plane, the closest `overlap` share of each pass's candidates kept) ----
// icp_loop's PCL align() for a single pair.  Per pass: the NN pass (plain launches; the pending T_k rides in as on the plain
// point-to-point path) writes idx / d2 by original source index; trimmed: the radix select over that d2 (four plain launches,
// tau / m / k stay on the device); the metric's rows + final launches reduce the sums into host-mapped memory (h_p2l: the sums
// in front, the selection's {m, k, tau, kept} behind KSS_P2L_NSUMS doubles); ONE stream synchronisation; then the solve and
// the PCL criteria on the host.  Untrimmed plane passes make no selection launches and keep a correspondence by
// !(d2 > max_d2).  The plan, the packed clouds and the cell list are built once per call.
// Robust (kss_icp_robust; stated in PairMode, never inferred): behind the NN pass, with the automatic scale, the
// plane metric's key launch and the same radix select at overlap 0.5 for the median key, then the weighted rows + final
// launches (the info slots hold {m, c2, sum of weights, cnt}); with a fixed scale only the latter two.  The host step reads cnt
// for the min_correspondences test and solves the weighted record as it is: [0] is the weight total.
// Generalized (kss_icp_gicp; M.gicp with M.plane): the gicp rows launch in place of the plane metric's, given the
// rotation of the transform accumulated so far for the source normals; the final launch, the record's layout, the host step and
// the criteria are the plane metric's.
// Symmetric (kss_icp_symm; M.symm with M.plane): the symmetric rows launch with the same rotation; the record's
// layout and the solve are the plane metric's, the step built from the solution is rigid_from_symm_sums' (two half rotations).
// Robust symmetric (kss_icp_symm_robust; M.symm with M.robust): the robust branch with the symmetric keys and rows
// launches and that rotation; the selection, the final launch, the info slots and the host step (cnt, rigid_from_symm_sums) are shared.
// Similarity (kss_icp_sim; M.sim with M.trimmed, point metric): the trimmed point metric's launches with SimMetric's
// rows and the final launch that keeps slot 17; the host step solves by sim_from_sums inside [scale_min, scale_max] / s_acc, keeps
// the pair's accumulated scale s_acc and reads PCL's criteria on the step without its scale; the info record grows to
// KSS_SIM_NINFO = {m, k, tau, kept, s_k, s_acc} (s_k = 0 where the pass made no step), the last two filled here on the host.
// One-to-one (kss_icp_o2o; M.unique with M.trimmed, either metric): three launches ahead of the selection (kss_o2o.hip:
// table reset, claim, resolve) filter the NN pass's idx / d2 into o2o_idx / o2o_d2, which the selection and the rows launch read in
// their place; the info record grows to KSS_O2O_NINFO = {u, k, tau, kept, m}, m published by the resolve launch behind the
// selection's four slots.  The NN pass's own arrays stay as written: the fitness pass and fitness_idx / fitness_d2 are unfiltered.
// Reciprocal (kss_icp_recip; M.mutual with M.trimmed, either metric): five launches ahead of the
// selection (kss_recip.hip: reset, claim + count, scan, scatter, resolve + check) filter the same arrays the same way, against the
// positions the NN pass wrote; the info record grows to KSS_RECIP_NINFO = {r, k, tau, kept, m, u}, m and u published by the resolve launch.
// One pair or many per call (kss_icp_recip_pairs), the same kernels: every pair on its own grid.
// the rotation block of a row-major 4 x 4 (the float bits of the accumulated Matrix4f)
static GicpRot rot_of(const float* F) { return GicpRot{{F[0], F[1], F[2], F[4], F[5], F[6], F[8], F[9], F[10]}}; }

// ---- what a pass launches behind its correspondences, by PairMode.  pair_pass_launch (kss_pair.hip's kernels,
// one pair) and pairb_pass_launch (kss_pairb.hip's, npairs >= 1) are the only places that turn a mode into launches: a new metric
// adds one line to each. ----
// the buffers pair_pass_launch uses for n sources; have_d2: its PairArgs will carry the NN pass's d2
static int pair_pass_ensure(kss_ctx* c, const PairMode& M, int64_t n, bool have_d2) {
    KCHK(ensure(c, c->p2l_rows, (size_t)p2l_rows_blocks(n) * P2L_NSUMS * sizeof(double)));
    if (M.trimmed || (M.robust && M.rs.autoscale)) {
        KCHK(ensure(c, c->trim_rows, trim_rows_bytes(n)));
        KCHK(ensure(c, c->trim_state, TRIM_NSTATE * sizeof(TrimState)));
    }
    if (M.robust && M.rs.autoscale && (M.plane || !have_d2)) KCHK(ensure(c, c->rob_keys, (size_t)n * sizeof(float)));
    return ensure_pinned(c, c->h_p2l, c->h_p2l_cap, (P2L_NSUMS + KSS_TRIM_NINFO + 2) * sizeof(double));   // (+ m, or m and u)
}

// a single pair as the filters' kernels see it: a batch of one descriptor
static PairbDesc lone_desc(int64_t ns, int64_t nt, double overlap) {
    PairbDesc d;
    d.src_base = 0; d.ns = ns; d.tgt_off = 0; d.nt = nt; d.overlap = overlap; d.row_base = 0; d.nrows = stream_blocks(ns);
    return d;
}

// reciprocal's reset and four launches for np pairs against s's positions, the reverse distances by dist2<nn_fma>: the NN pass's own
// p2l_idx / p2l_d2 filtered into o2o_idx / o2o_d2, {m, u} per pair into d_info_mu.  One pair: np = 1, total_rows = stream_blocks(n),
// total_tgt = nt, no tables: the pair's descriptor `lone` and its grid go inside the arguments.
static int recip_pass_launch(kss_ctx* c, const PairSrc& s, const float* tgt, const PairbDesc* desc, const int32_t* row_pair, const PairState* state,
                             int np, int total_rows, int64_t total_tgt, double* d_info_mu, bool nn_fma, const PairbDesc& lone = PairbDesc()) {
    RecipArgs ra = {s, tgt, desc, row_pair, state, (const RecipPairDev*)c->recip_grids.p, c->o2o_table.p, total_tgt, np,
                    (float4*)c->recip_sorted.p, (int32_t*)c->o2o_idx.p, (float*)c->o2o_d2.p, d_info_mu, lone, c->h_recip_grids[0]};
    ra.s.idx = (const int32_t*)c->p2l_idx.p; ra.s.d2 = (const float*)c->p2l_d2.p;
    if (launch_recip(c->stream, total_rows, c->recip_total_cells, ra, nn_fma) != 0) return set_err(c, KSS_ERR_HIP, "hipMemsetAsync(reciprocal workspace)");
    return KSS_OK;
}

// One pair: [one-to-one's three launches | reciprocal's five] [selection] [keys launch + the 0.5 selection] rows launch, final launch.  Rn: the
// rotation the source normals turn with (generalized, symmetric); d_rec: the record, d_info: the selection's or the weights' four
// slots, the one-to-one's m behind them (device or host-mapped).  One-to-one filters the context's p2l_idx / p2l_d2 (the NN
// pass's own) into o2o_idx / o2o_d2, which a.s.idx / a.s.d2 then are.  The automatic scale's median key: the plane metrics write
// their keys; a point-metric pass that carries d2 selects on it, one without d2 writes its keys first.  Reciprocal filters the same
// arrays against a.s's positions, the reverse distances by dist2<nn_fma>; m and u land behind the selection's record.
static int pair_pass_launch(kss_ctx* c, const PairArgs& a, const PairMode& M, const GicpRot& Rn, double* d_rec, double* d_info,
                            bool nn_fma = false) {
    ProfScope ps(c, KSS_K_CORR_REDUCE);
    const hipStream_t st = c->stream;
    const double max_d2 = a.s.max_d2;
    const int nb = stream_blocks(a.n);
    TrimState* d_state = (TrimState*)c->trim_state.p;
    if (M.unique) {   // table reset, claim, resolve: m lands behind the selection's record
        const O2oArgs oa = {(const int32_t*)c->p2l_idx.p, (const float*)c->p2l_d2.p, (const PairbDesc*)c->pb_desc.p, nullptr, nullptr, max_d2,
                            (unsigned long long*)c->o2o_table.p, (unsigned*)((unsigned long long*)c->o2o_table.p + a.nt),
                            (int32_t*)c->o2o_idx.p, (float*)c->o2o_d2.p, d_info + KSS_TRIM_NINFO};
        if (launch_o2o(st, nb, a.nt, 1, oa) != 0) return set_err(c, KSS_ERR_HIP, "hipMemsetAsync(claim table)");
    }
    if (M.mutual)   // reset, claim + count, scan, scatter, resolve + check
        KCHK(recip_pass_launch(c, a.s, a.tgt, nullptr, nullptr, nullptr, 1, nb, a.nt, d_info + KSS_TRIM_NINFO, nn_fma, lone_desc(a.n, a.nt, M.overlap)));
    if (M.trimmed) launch_trim_select(st, a.s.d2, a.n, max_d2, M.overlap, (unsigned*)c->trim_rows.p, d_state, d_info);
    const double* d_cut = M.trimmed ? &d_state[TRIM_NSTATE - 1].cut : nullptr;
    if (M.robust) {
        const TrimState* d_sel = nullptr;
        if (M.rs.autoscale) {   // (written keys carry the whole candidate test, a NaN is none: no bound; d2 takes the pass's)
            const float* d_keys = a.keys;
            if (M.symm) launch_pair_rows(st, a, SymmMetric<PAIR_KEY>(Rn, M.symm_align));
            else if (M.plane) launch_pair_rows(st, a, PlaneRobustMetric<PAIR_KEY>());
            else if (a.s.d2) d_keys = a.s.d2;
            else launch_pair_rows(st, a, PointRobustMetric<PAIR_KEY>());
            launch_trim_select(st, d_keys, a.n, M.plane ? std::numeric_limits<double>::infinity() : max_d2, 0.5, (unsigned*)c->trim_rows.p,
                               d_state, nullptr);
            d_sel = d_state + (TRIM_NSTATE - 1);
        }
        if (M.symm) launch_pair_rows(st, a, SymmMetric<PAIR_ROBUST>(Rn, M.symm_align, M.rs, d_sel));
        else if (M.plane) launch_pair_rows(st, a, PlaneRobustMetric<PAIR_ROBUST>(M.rs, d_sel));
        else launch_pair_rows(st, a, PointRobustMetric<PAIR_ROBUST>(M.rs, d_sel));
        if (M.plane) launch_robust_plane_final(st, a.rows, nb, M.rs, d_sel, d_rec, d_info);
        else launch_robust_point_final(st, a.rows, nb, M.rs, d_sel, d_rec, d_info);
    } else if (M.plane) {
        if (M.gicp) launch_pair_rows(st, a, GicpMetric(Rn, 1.0 - M.gicp_epsilon));
        else if (M.symm) launch_pair_rows(st, a, SymmMetric<PAIR_PLAIN>(Rn, M.symm_align));
        else if (M.trimmed) launch_pair_rows(st, a, PlaneMetric<true>(max_d2, d_cut));
        else launch_pair_rows(st, a, PlaneMetric<false>(max_d2, nullptr));
        launch_p2l_final(st, a.rows, nb, d_rec);
    } else if (M.sim) {
        launch_pair_rows(st, a, SimMetric(max_d2, d_cut));
        launch_sim_final(st, a.rows, nb, d_rec);
    } else {
        launch_pair_rows(st, a, PointTrimMetric(d_cut));
        launch_trim_point_final(st, a.rows, nb, d_rec);
    }
    return KSS_OK;
}

// npairs >= 1 pairs, the same order of launches over the per-pair tables of a: d_rec: np records of P2L_NSUMS doubles, d_info: np
// info records of four slots, the one-to-one's np m's behind them.  rob_select: some pair takes its scale from the pass's median
// key (the point metric's keys are the NN pass's d2).  A pass table on the device is first copied from the pinned one as the host
// steps left it: the last pass's synchronisation has ordered those writes behind its copy.  Reciprocal: the reset and four launches
// for the whole batch against a.s's positions, the reverse distances by dist2<nn_fma>; every pair's m and u land behind the np
// selection records, two slots per pair.
static int pairb_pass_launch(kss_ctx* c, const PairbArgs& a, const PairMode& M, int np, int total_rows, int64_t total_tgt, bool rob_select,
                             double* d_rec, double* d_info, bool nn_fma = false) {
    ProfScope ps(c, KSS_K_CORR_REDUCE);
    const hipStream_t st = c->stream;
    const double max_d2 = a.s.max_d2;
    if (a.pass && a.pass == (const PairPass*)c->pb_gicp.p)
        HIPCHK(c, hipMemcpyAsync(c->pb_gicp.p, c->h_gicp, (size_t)np * sizeof(PairPass), hipMemcpyHostToDevice, st));
    if (M.unique) {   // table reset, claim, resolve for the whole batch
        const O2oArgs oa = {(const int32_t*)c->p2l_idx.p, (const float*)c->p2l_d2.p, a.desc, a.row_pair, a.state, max_d2,
                            (unsigned long long*)c->o2o_table.p, (unsigned*)((unsigned long long*)c->o2o_table.p + total_tgt),
                            (int32_t*)c->o2o_idx.p, (float*)c->o2o_d2.p, d_info + (size_t)np * KSS_TRIM_NINFO};
        if (launch_o2o(st, total_rows, total_tgt, np, oa) != 0) return set_err(c, KSS_ERR_HIP, "hipMemsetAsync(claim table)");
    }
    if (M.mutual)   // reset, claim + count, scan, scatter, resolve + check for the whole batch
        KCHK(recip_pass_launch(c, a.s, a.tgt, a.desc, a.row_pair, a.state, np, total_rows, total_tgt, d_info + (size_t)np * KSS_TRIM_NINFO, nn_fma));
    if (M.trimmed) launch_pairb_select(st, a.s.d2, a.desc, np, a.state, max_d2, a.ts, d_info);
    if (M.robust) {
        if (rob_select) {   // (written keys carry the whole candidate test, a NaN is none: no bound)
            if (M.symm) launch_pairb_rows<SymmMetric<PAIR_KEY>>(st, total_rows, a);
            else if (M.plane) launch_pairb_rows<PlaneRobustMetric<PAIR_KEY>>(st, total_rows, a);
            launch_pairb_robust_select(st, np, a, M.plane ? a.keys : a.s.d2, M.plane ? std::numeric_limits<double>::infinity() : max_d2);
        }
        if (M.symm) launch_pairb_rows<SymmMetric<PAIR_ROBUST>>(st, total_rows, a);
        else if (M.plane) launch_pairb_rows<PlaneRobustMetric<PAIR_ROBUST>>(st, total_rows, a);
        else launch_pairb_rows<PointRobustMetric<PAIR_ROBUST>>(st, total_rows, a);
        launch_pairb_robust_final(st, M.plane, np, a, d_rec, d_info);
    } else {
        if (M.gicp) launch_pairb_rows<GicpMetric>(st, total_rows, a);
        else if (M.symm) launch_pairb_rows<SymmMetric<PAIR_PLAIN>>(st, total_rows, a);
        else if (M.sim) launch_pairb_rows<SimMetric>(st, total_rows, a);
        else if (!M.plane) launch_pairb_rows<PointTrimMetric>(st, total_rows, a);
        else if (M.trimmed) launch_pairb_rows<PlaneMetric<true>>(st, total_rows, a);
        else launch_pairb_rows<PlaneMetric<false>>(st, total_rows, a);
        launch_pairb_final(st, M.plane, np, a, d_rec, M.sim);
    }
    return KSS_OK;
}

// One pass over given correspondences (the *_sums_dev entry points, which check their arguments: kss_api.hip): the record of mode M
// for n packed float triples d_src with the targets d_idx, into sums (KSS_P2L_NSUMS or KSS_NSUMS doubles by metric) and, robust, its
// {m, c2, sum of weights, cnt} into info.  Rn: the row-major 3 x 3 the source normals turn with (null: identity).  No NN pass has
// run: the distances are recomputed, the point metric writes its keys.
int pair_record_dev(kss_ctx* c, const float* d_src, const float* d_tgt, const float* d_nrm, const int32_t* d_idx, int64_t n, int64_t nt,
                    double max_d2, const PairMode& M, const float* Rn, double* sums, double* info) {
    KCHK(pair_pass_ensure(c, M, n, false));
    const PairArgs a = {{d_src, nullptr, nullptr, d_idx, nullptr, M.d_src_nrm, max_d2}, d_tgt, d_nrm, n, nt, (double*)c->p2l_rows.p,
                        (float*)c->rob_keys.p};
    KCHK(pair_pass_launch(c, a, M, gicp_rot_of(Rn), (double*)c->h_p2l_dev, (double*)c->h_p2l_dev + P2L_NSUMS));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::memcpy(sums, c->h_p2l, (size_t)(M.plane ? P2L_NSUMS : NSUMS) * sizeof(double));
    if (M.robust) std::memcpy(info, (const double*)c->h_p2l + P2L_NSUMS, KSS_ROBUST_NINFO * sizeof(double));
    return KSS_OK;
}

// ---- the loop of every pair metric: kss_icp_p2l, kss_icp_trimmed, kss_icp_robust, kss_icp_gicp, kss_icp_symm,
// kss_icp_symm_robust, kss_icp_sim, kss_icp_o2o and their _batch forms ----
// npairs >= 1 pairs in lockstep.  Per pass: ONE NN pass over the pairs still active (idx / d2 by global source index), the
// launches of the call's kernel family (above), ONE stream synchronisation, then pair_host_step for every active pair (the host
// pool from 64 pairs up, each pair on exactly one thread).  A pair that ends goes inactive in the per-pair state table; the
// workgroups of the later passes' launches leave at once for it and its rows of the host-mapped tables are not written again: no
// ending touches another pair's record.  icp_loop's engine switch applies.
// single: the call is pair_run_dev's.  It decides how the NN pass is called (the single pair's waits for its own sums, gated /
// chained machinery and all; the batch's wait is deferred to the launches behind it) and which family's launches follow -- nothing
// else.  A batch of one runs the batched kernels; the host-mapped layouts of both families coincide at np == 1.
struct DeferWait {   // the NN pass does not wait for its sums: the launches behind it are waited for instead
    kss_ctx* c;
    explicit DeferWait(kss_ctx* c_) : c(c_) { c->defer_wait = true; }
    ~DeferWait() { c->defer_wait = false; }
};
// pair p's info record behind a pass, from the host-mapped tables h: np records, np selection records, np m's (one-to-one) or np
// {m, u} (reciprocal)
static void pair_info_read(const PairMode& M, const double* h, int np, int p, double* info) {
    if (!M.trimmed && !M.robust) return;
    const double* hinfo = h + (size_t)np * P2L_NSUMS;
    std::memcpy(info, hinfo + (size_t)p * KSS_TRIM_NINFO, KSS_TRIM_NINFO * sizeof(double));
    if (M.trimmed) info[3] = h[(size_t)p * P2L_NSUMS];   // the correspondences the step is computed from (plane: those of the cut with a finite normal)
    if (M.unique) info[4] = hinfo[(size_t)np * KSS_TRIM_NINFO + p];   // one-to-one: m, the candidates before the rejection ([0] is u)
    if (M.mutual) {   // reciprocal: m and u ([0] is r), two slots per pair behind the np selection records
        info[4] = hinfo[(size_t)np * KSS_TRIM_NINFO + 2 * (size_t)p];
        info[5] = hinfo[(size_t)np * KSS_TRIM_NINFO + 2 * (size_t)p + 1];
    }
}
static int pairs_loop(kss_ctx* c, const IcpPlan& pl_in, const kss_icp_params& P, const PairMode& M, const float* d_tgt, const float* d_nrm,
                      const int32_t* d_perm, bool single, bool rob_select, kss_icp_result* results, double* info_all) {
    const int np = pl_in.npairs;
    // generalized, symmetric: every pair's PairPass (pinned; staged by stage_pass_table) starts from the identity and follows the
    // pair's fin: the rotation the source normals turn with.  The single pair's launches take it from there by value; the batched
    // kernels read a device copy made per pass or, A/B switch, the pinned table across the bus
    PairPass* hpass = M.gicp || M.symm ? (PairPass*)c->h_gicp : nullptr;
    const char* env_mapped = hpass ? getenv("KSS_GICP_TABLE_MAPPED") : nullptr;
    const bool pass_mapped = env_mapped && atoi(env_mapped) != 0 && c->h_gicp_dev;
    const PairPass* d_pass = hpass ? (pass_mapped ? (const PairPass*)c->h_gicp_dev : (const PairPass*)c->pb_gicp.p) : nullptr;
    auto pass_rot = [hpass](int p, const float* F) {
        if (hpass) std::memcpy(hpass[p].r, rot_of(F).r, sizeof hpass[p].r);
    };
    const IcpPlan* plan = &pl_in;   // may change to the brute-force plan below
    IcpPlan brute_plan;
    std::vector<PairTrack> tr((size_t)np, PairTrack(P));
    std::vector<int> active(np, 1), was_active;
    PairState* hs = (PairState*)c->h_state;
    PairState* bar = pl_in.gridb ? (PairState*)bar_ensure(c, c->bar_state, (size_t)np * sizeof(PairState)) : nullptr;   // (null without a large BAR)
    float I[16];
    mat4_identity(I);
    for (int p = 0; p < np; ++p) {
        set_state(hs[p], I, 1, 0);
        mirror_state(bar, p, hs[p]);
        pass_rot(p, tr[p].fin);
    }
    const double max_d2 = P.max_corr_dist * P.max_corr_dist;
    int32_t* d_idx = (int32_t*)c->p2l_idx.p;
    float* d_d2 = (float*)c->p2l_d2.p;
    const double* hrec = (const double*)c->h_p2l;   // np records of P2L_NSUMS doubles, the info records behind them (pair_info_read)
    double* d_rec = (double*)c->h_p2l_dev;
    double* d_info = d_rec + (size_t)np * P2L_NSUMS;
    // one-to-one: the selection and the rows read the filtered copies; d_idx / d_d2 stay the NN pass's own
    const bool filtered = M.unique || M.mutual;   // (reciprocal, DESIGN.md 2.25: the same hand-over)
    const PairSrc src = {nullptr, nullptr, d_perm, filtered ? (const int32_t*)c->o2o_idx.p : d_idx, filtered ? (const float*)c->o2o_d2.p : d_d2,
                         M.d_src_nrm, max_d2};
    int64_t total_tgt = 0;
    int total_rows = 0;
    for (int p = 0; p < np; ++p) { total_tgt += pl_in.g[p].nt; total_rows += stream_blocks(pl_in.g[p].ns); }
    if (P.trace_n) *P.trace_n = 0;
    const int ninfo = pair_ninfo(M);
    if (info_all) std::fill(info_all, info_all + (size_t)np * ninfo, 0.0);
    int n_active = P.max_iterations > 0 ? np : 0;
    if (n_active == 0) std::fill(active.begin(), active.end(), 0);
    int it = 0;
    GatedGuard gated_guard(c);
    c->gated.want_next = false;
    while (n_active > 0) {
        const float4* d_in = it == 0 ? (const float4*)c->src0.p : (const float4*)c->cur[(it - 1) & 1].p;
        float4* d_out = (float4*)c->cur[it & 1].p;
        c->last_state_dev = nullptr;
        PairSrc s = src;
        s.src4 = d_out;
        unsigned long long pass_seq = 0;
        if (single) {
            KCHK(nn_pass(c, *plan, P.nn_fma != 0, d_in, d_out, max_d2, d_idx, d_d2, false));
            const PairArgs a = {s, d_tgt, d_nrm, plan->g[0].ns, plan->g[0].nt, (double*)c->p2l_rows.p, (float*)c->rob_keys.p};
            KCHK(pair_pass_launch(c, a, M, gicp_rot_of(hpass ? hpass[0].r : nullptr), d_rec, d_info, P.nn_fma != 0));
        } else {
            {
                DeferWait defer(c);
                KCHK(nn_pass(c, *plan, P.nn_fma != 0, d_in, d_out, max_d2, d_idx, d_d2, false, active.data()));
            }
            pass_seq = c->seq;
            // (state: the table the NN pass read; a single pair on its own cell list has none: it is active)
            const PairbArgs a = {s, d_tgt, d_nrm, (const PairbDesc*)c->pb_desc.p, (const int32_t*)c->pb_rowpair.p, c->last_state_dev,
                                 (const RobustScale*)c->pb_rscale.p, (TrimState*)c->trim_state.p, d_pass, (double*)c->p2l_rows.p,
                                 (float*)c->rob_keys.p};
            KCHK(pairb_pass_launch(c, a, M, np, total_rows, total_tgt, rob_select, d_rec, d_info, P.nn_fma != 0));
        }
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));
        ++it;
        if (plan->gridb) {   // the NN pass's own sums (slot 19: the fallback count) have landed with everything else
            for (int p = 0; p < np; ++p)
                if (active[p] && !collect_pair(c, p, pass_seq)) return set_err(c, KSS_ERR_HIP, "kernel finished without publishing its result");
            was_active = active;
        }
        std::atomic<int> finished{0};
        auto solve = [&](int pb, int pe) {
            int fin_here = 0;
            for (int p = pb; p < pe; ++p) {
                if (!active[p]) continue;
                double info[KSS_SIM_NINFO] = {};
                pair_info_read(M, hrec, np, p, info);
                const bool goes_on = pair_host_step(P, M, hrec + (size_t)p * P2L_NSUMS, info, tr[p], p == 0);   // (similarity: fills the scale slots of info)
                if ((M.trimmed || M.robust) && info_all) std::memcpy(info_all + (size_t)p * ninfo, info, (size_t)ninfo * sizeof(double));
                if (goes_on) {
                    set_state(hs[p], tr[p].tk, 1, 1);   // next NN pass applies T_k on load (transformCloud)
                } else {
                    active[p] = 0; ++fin_here;
                    set_state(hs[p], I, 0, 0);
                }
                pass_rot(p, tr[p].fin);   // the source normals turn with the transform accumulated so far
                mirror_state(bar, p, hs[p]);
            }
            finished.fetch_add(fin_here, std::memory_order_relaxed);
        };
        if (np >= 64) {
            std::atomic<int> next{0};
            constexpr int kBlock = 64;   // pairs claimed at a time (solve_pairs' grain)
            c->pool.parallel_for(np, [&](int, int) {
                for (;;) {
                    const int pb = next.fetch_add(1) * kBlock;
                    if (pb >= np) break;
                    solve(pb, std::min(np, pb + kBlock));
                }
            });
        } else {
            solve(0, np);
        }
        n_active -= finished.load(std::memory_order_relaxed);
        if (plan->gridb && n_active > 0) KCHK(switch_engine_on_fallback(c, plan, brute_plan, P, was_active));
    }
    for (int p = 0; p < np; ++p) fill_result(results[p], tr[p].fin, tr[p].iters, tr[p].converged, tr[p].state, tr[p].last_mse, 0.0, p);
    if (!P.compute_fitness) return KSS_OK;
    const bool corr = P.fitness_idx || P.fitness_d2;
    return fitness_pass(c, *plan, P, tr.data(), plan == &pl_in, bar, corr ? d_idx : nullptr, corr ? d_d2 : nullptr, results);
}

static int stage_pairb(kss_ctx* c, const std::vector<PairbDesc>& desc, bool rows);

// ---- what pair_run_dev and pairs_run_dev share around the loop ----
// the mode's consistency (the arguments are the entry points' to check: kss_api.hip); batch: with the per-pair tables its forms need
static int pair_mode_check(kss_ctx* c, const char* who, const PairMode& M, const float* d_nrm, bool batch = false,
                           const RobustScale* rscales = nullptr, const double* gicp_eps = nullptr, const int32_t* symm_aligns = nullptr) {
    const std::string w = std::string(who) + ": ";
    auto bad = [&](const char* what) { return set_err(c, KSS_ERR_ARG, (w + what).c_str()); };
    if (!M.plane && !M.trimmed && !M.robust) return bad("the untrimmed point metric is kss_icp's");
    if (M.trimmed && M.robust) return bad("trimmed and robust exclude each other");
    if (M.sim && (M.plane || !M.trimmed)) return bad("similarity ICP is the trimmed point metric's");
    if (M.gicp && (!M.plane || M.trimmed || M.robust || !M.d_src_nrm || !d_nrm))
        return bad("generalized ICP is the plane record with both clouds' normals, neither trimmed nor robust");
    if (M.symm && (!M.plane || M.trimmed || M.gicp || !M.d_src_nrm || !d_nrm))
        return bad("symmetric ICP is the plane record with both clouds' normals, neither trimmed nor generalized");
    if (M.unique && (!M.trimmed || M.robust || M.gicp || M.symm || M.sim))
        return bad("one-to-one rejection is the trimmed pass's, neither robust, generalized, symmetric nor similarity");
    if (M.mutual && (!M.trimmed || M.unique || M.robust || M.gicp || M.symm || M.sim))
        return bad("reciprocal rejection is the trimmed pass's, neither one-to-one, robust, generalized, symmetric nor similarity");
    if (!batch) return KSS_OK;
    if (M.robust && !rscales) return bad("robust needs the per-pair scales");
    if (M.gicp && !gicp_eps) return bad("generalized ICP needs the per-pair epsilons");
    if (M.symm && !symm_aligns) return bad("symmetric ICP needs the per-pair aligns");
    return KSS_OK;
}

// generalized, symmetric: the per-pair pass table, pinned and on the device: e = 1 - epsilon as pair_pass_launch forms it, align
// as it passes it; pairs_loop fills the rotations
static int stage_pass_table(kss_ctx* c, const PairMode& M, int npairs, const double* gicp_eps, const int32_t* symm_aligns) {
    KCHK(ensure(c, c->pb_gicp, (size_t)npairs * sizeof(PairPass)));
    KCHK(ensure_pinned(c, c->h_gicp, c->h_gicp_cap, (size_t)npairs * sizeof(PairPass)));
    HIPCHK(c, hipHostGetDevicePointer(&c->h_gicp_dev, c->h_gicp, 0));
    PairPass* hpass = (PairPass*)c->h_gicp;
    std::memset(hpass, 0, (size_t)npairs * sizeof(PairPass));
    for (int i = 0; i < npairs; ++i) {
        if (M.gicp) hpass[i].e = 1.0 - gicp_eps[i];
        else hpass[i].align = symm_aligns[i];
    }
    return KSS_OK;
}

// the end of both: where the cell-list setup put each source (it re-orders them, .w: the global original index), the loop, and
// the call's two timings from t0
static int pair_run_loop(kss_ctx* c, const IcpPlan& pl, std::chrono::steady_clock::time_point t0, DirtyGuard& guard, const kss_icp_params& P,
                         const PairMode& M, const float* d_tgt, const float* d_nrm, bool single, bool rob_select, kss_icp_result* results,
                         double* info_all) {
    const int32_t* d_perm = nullptr;
    if (pl.src_in_cell_order) {
        KCHK(ensure(c, c->p2l_perm, (size_t)pl.total_src * sizeof(int32_t)));
        launch_p2l_perm(c->stream, (const float4*)c->src0.p, pl.total_src, (int32_t*)c->p2l_perm.p);
        HIPCHK(c, hipGetLastError());
        d_perm = (const int32_t*)c->p2l_perm.p;
    }
    const auto t1 = std::chrono::steady_clock::now();
    const int rc = pairs_loop(c, pl, P, M, d_tgt, d_nrm, d_perm, single, rob_select, results, info_all);
    guard.ok = rc == KSS_OK;
    const auto t2 = std::chrono::steady_clock::now();
    c->last_setup_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
    c->last_loop_ms = std::chrono::duration<double, std::milli>(t2 - t1).count();
    return rc;
}

// reciprocal, once per call, behind stage_pairb: every pair's target box from ONE launch over the staged
// descriptors (`split` partials per pair, one copy back and ONE synchronisation whatever the pair count), every pair's grid --
// recip_grid_of(the box of ITS target, ITS source count) -- with its first cell, staged next to pb_desc; the workspace and the
// call's cell-ordered source array of total_src float4.  lone: the single-pair entries' desc[0], whose partials are cut finer and
// which stages nothing: descriptor and grid travel in the launches' arguments.
// How the partials are cut may move a bit of a grid (fminf / fmaxf may hand back either zero of a tie).  It cannot matter: "mutual"
// is an existence statement over ALL sources of the pair, the box walk is proven to hold every source that can hit on ANY grid of
// this form, and the escape scans the pair's whole slice.
static int recip_setup(kss_ctx* c, const float* d_tgt, const std::vector<PairbDesc>& desc, int64_t total_src, const char* who, bool lone = false) {
    const int np = (int)desc.size();
    int64_t total_tgt = 0, max_nt = 0;
    for (const PairbDesc& d : desc) { total_tgt += d.nt; max_nt = std::max(max_nt, d.nt); }
    const int split = lone ? (int)std::max<int64_t>(1, std::min<int64_t>(RECIP_BOX_BLOCKS, (max_nt + 1023) / 1024))
                           : (int)std::max<int64_t>(1, std::min<int64_t>(64, (max_nt + 4 * 1024 - 1) / (4 * 1024)));
    const std::string large = std::string(who) + ": batch too large for 32-bit indexing";
    if (total_tgt > PAIRB_INDEX_MAX || (int64_t)np * split > PAIRB_INDEX_MAX) return set_err(c, KSS_ERR_ARG, large.c_str());
    const size_t nbox = (size_t)np * split;
    KCHK(ensure(c, c->recip_box, nbox * 6 * sizeof(float)));
    launch_recip_bbox(c->stream, d_tgt, lone ? nullptr : (const PairbDesc*)c->pb_desc.p, desc[0], np, split, (float*)c->recip_box.p);
    HIPCHK(c, hipGetLastError());
    std::vector<float> hb(nbox * 6);
    HIPCHK(c, hipMemcpyAsync(hb.data(), c->recip_box.p, hb.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->recip_total_cells = recip_grids_of(hb.data(), split, desc, c->h_recip_grids);
    if (c->recip_total_cells < 0) return set_err(c, KSS_ERR_ARG, large.c_str());
    if (!lone) {   // (the source of this copy is the context's own vector: it outlives the copy, no synchronisation here)
        KCHK(ensure(c, c->recip_grids, (size_t)np * sizeof(RecipPairDev)));
        HIPCHK(c, hipMemcpyAsync(c->recip_grids.p, c->h_recip_grids.data(), (size_t)np * sizeof(RecipPairDev), hipMemcpyHostToDevice, c->stream));
    }
    KCHK(ensure(c, c->o2o_table, recip_work_bytes(total_tgt, np, c->recip_total_cells)));
    return ensure(c, c->recip_sorted, (size_t)total_src * sizeof(float4));
}

int pair_run_dev(kss_ctx* c, const float* d_src, int64_t ns, const float* d_tgt, int64_t nt, const float* d_nrm,
                 const kss_icp_params* p, const PairMode& M, kss_icp_result* res) {
    KCHK(pair_mode_check(c, "pair_run", M, d_nrm));
    HIPCHK(c, hipSetDevice(c->device));
    IcpPlan pl;
    const auto t0 = std::chrono::steady_clock::now();
    KCHK(restore_zero_at_rest(c));
    DirtyGuard guard(c);
    c->timing = false;
    KCHK(build_plan(c, &ns, &nt, 1, false, p->nn_sources_per_thread, p->nn_target_splits, p->nn_mode, pl));
    KCHK(stage_plan(c, pl));
    KCHK(ensure(c, c->p2l_idx, (size_t)ns * sizeof(int32_t)));
    KCHK(ensure(c, c->p2l_d2, (size_t)ns * sizeof(float)));
    KCHK(pair_pass_ensure(c, M, ns, true));
    if (M.gicp || M.symm) KCHK(stage_pass_table(c, M, 1, &M.gicp_epsilon, &M.symm_align));
    if (M.unique || M.mutual) {   // the filtered idx / d2 and the pair as the filters' kernels see it: a batch of one descriptor
        KCHK(ensure(c, c->o2o_idx, (size_t)ns * sizeof(int32_t)));
        KCHK(ensure(c, c->o2o_d2, (size_t)ns * sizeof(float)));
        const std::vector<PairbDesc> desc(1, lone_desc(ns, nt, M.overlap));
        if (M.unique) {   // staged, and the claim table
            KCHK(stage_pairb(c, desc, false));
            KCHK(ensure(c, c->o2o_table, o2o_table_bytes(nt, 1)));
        } else {          // in the launches' arguments: the cell grid over the target's box, the workspace and the cell-ordered sources
            KCHK(recip_setup(c, d_tgt, desc, ns, "pair_run", true));
        }
    }
    const int64_t so[2] = {0, ns}, to[2] = {0, nt};
    KCHK(pack_clouds(c, pl, d_src, so, d_tgt, to, KSS_F32));
    KCHK(grid_setup(c, pl));
    return pair_run_loop(c, pl, t0, guard, *p, M, d_tgt, d_nrm, true, false, res, M.last_info);
}

// ---- voxelized generalized ICP against a voxel map (kss_icp_vgicp) ----
// No plan, no packed clouds, no cell list, no NN pass: a pass is VgicpMetric's rows launch -- which moves the sources by the last
// step on the way in (pass k >= 1 reads the positions of pass k - 1, pass 1 the caller's cloud, and writes cur[k & 1]) -- and the plane
// record's final launch into h_p2l, ONE synchronisation, then pair_host_step as for kss_icp_gicp (M.plane with M.gicp: the
// Cholesky step, MSE = [28] / [0], the trace).  Nothing here touches a zero-at-rest buffer.
// KSS_VGICP_UNFUSED=1 (A/B, tools/vgicp_time.py): the move as a launch of its own in front of a rows launch that does not move.
static PairArgs vgicp_args(kss_ctx* c, const float* d_snrm, int64_t n, double max_d2) {
    return PairArgs{{nullptr, nullptr, nullptr, nullptr, nullptr, d_snrm, max_d2}, nullptr, nullptr, n, 0, (double*)c->p2l_rows.p, nullptr};
}
static int vgicp_ensure(kss_ctx* c, int64_t n) {
    KCHK(ensure(c, c->p2l_rows, (size_t)p2l_rows_blocks(n) * P2L_NSUMS * sizeof(double)));
    return ensure_pinned(c, c->h_p2l, c->h_p2l_cap, (P2L_NSUMS + KSS_TRIM_NINFO + 2) * sizeof(double));
}
// rows + final into h_p2l: T null: the positions d_in as they are; else moved by T (a row-major 4 x 4) into d_out first
static int vgicp_pass_launch(kss_ctx* c, const PairArgs& a, const kss_vmap* map, const float* T, const float* d_in, float* d_out,
                             const GicpRot& Rn, double epsilon, bool unfused) {
    ProfScope ps(c, KSS_K_CORR_REDUCE);
    VmapMove mv;
    if (T) std::memcpy(mv.m, T, sizeof mv.m);
    if (T && unfused) {
        launch_transform_apply_f32(c->stream, T, d_in, a.n, d_out);
        launch_vgicp_rows(c->stream, a, map->dev(), nullptr, d_out, nullptr, Rn, 1.0 - epsilon, map->nb);
    } else {
        launch_vgicp_rows(c->stream, a, map->dev(), T ? &mv : nullptr, d_in, d_out, Rn, 1.0 - epsilon, map->nb);
    }
    launch_p2l_final(c->stream, a.rows, stream_blocks(a.n), (double*)c->h_p2l_dev);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return KSS_OK;
}

int vgicp_record_dev(kss_ctx* c, const float* d_src, const float* d_snrm, int64_t n, const kss_vmap* map, double max_d2, const float* Rn,
                     double epsilon, double* sums) {
    HIPCHK(c, hipSetDevice(c->device));
    KCHK(vgicp_ensure(c, n));
    KCHK(vgicp_pass_launch(c, vgicp_args(c, d_snrm, n, max_d2), map, nullptr, d_src, nullptr, gicp_rot_of(Rn), epsilon, false));
    std::memcpy(sums, c->h_p2l, P2L_NSUMS * sizeof(double));
    return KSS_OK;
}

// T0 (kss_icp_vgicp_from): fin starts at T0, pass 0 moves the caller's cloud by T0 into cur[0] on the way in and pass
// k >= 1 reads cur[(k - 1) & 1]; null: the loop above, unchanged.
int vgicp_run_dev(kss_ctx* c, const float* d_src, int64_t ns, const float* d_snrm, const kss_vmap* map, const float* T0, const kss_icp_params* p,
                  double epsilon, kss_icp_result* res, double* info) {
    HIPCHK(c, hipSetDevice(c->device));
    const kss_icp_params& P = *p;
    const auto t0 = std::chrono::steady_clock::now();
    KCHK(vgicp_ensure(c, ns));
    for (DevBuf& b : c->cur) KCHK(ensure(c, b, (size_t)ns * 3 * sizeof(float)));
    static const bool unfused = getenv("KSS_VGICP_UNFUSED") != nullptr && atoi(getenv("KSS_VGICP_UNFUSED")) != 0;
    PairMode M;
    M.plane = true; M.gicp = true;
    const PairArgs a = vgicp_args(c, d_snrm, ns, P.max_corr_dist * P.max_corr_dist);
    float* d_cur[2] = {(float*)c->cur[0].p, (float*)c->cur[1].p};   // pass k >= 1 writes [k & 1] and reads what pass k - 1 wrote
    const double* hrec = (const double*)c->h_p2l;
    PairTrack t(P);
    if (T0) std::memcpy(t.fin, T0, sizeof t.fin);
    double last[KSS_VGICP_NINFO] = {0.0, (double)ns, 0.0, (double)map->b.nvox};
    if (P.trace_n) *P.trace_n = 0;
    const auto t1 = std::chrono::steady_clock::now();
    for (int it = 0; P.max_iterations > 0; ++it) {
        // pass it works on T_{it-1} ... T_0 * source: the last step is applied on the way in
        // (without a start pose pass 0 moves nothing, so pass 1 still reads the caller's cloud)
        KCHK(vgicp_pass_launch(c, a, map, it == 0 ? T0 : t.tk, it <= (T0 ? 0 : 1) ? d_src : d_cur[(it - 1) & 1], d_cur[it & 1], rot_of(t.fin), epsilon,
                               unfused));
        last[0] = hrec[0]; last[2] = hrec[30];
        double unused[KSS_SIM_NINFO] = {};
        if (!pair_host_step(P, M, hrec, unused, t, true)) break;
    }
    fill_result(*res, t.fin, t.iters, t.converged, t.state, t.last_mse, 0.0, 0);
    if (P.compute_fitness) {   // one more evaluation at fin * source: [28] / [0], over the sources that have a voxel (kept ones)
        KCHK(vgicp_pass_launch(c, a, map, t.fin, d_src, d_cur[0], rot_of(t.fin), epsilon, unfused));
        res->fitness = hrec[28] / hrec[0];
    }
    if (info) std::memcpy(info, last, sizeof last);
    const auto t2 = std::chrono::steady_clock::now();
    c->last_setup_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
    c->last_loop_ms = std::chrono::duration<double, std::milli>(t2 - t1).count();
    return KSS_OK;
}

// The ladder (kss_icp_vgicp_c2f): the staged scan and its normals serve every level; a level is vgicp_run_dev from
// the pose of the one before, whatever its state; the fitness evaluation and the caller's trace belong to the last level.
int vgicp_c2f_run_dev(kss_ctx* c, const float* d_src, int64_t ns, const float* d_snrm, const kss_vmap* const* maps, int nlevels, const float* T0,
                      const kss_icp_params* p, double epsilon, kss_icp_result* results, double* info) {
    kss_icp_params quiet = *p;   // the levels in front of the last: no fitness evaluation, no trace
    quiet.compute_fitness = 0;
    quiet.trace_sums = nullptr; quiet.trace_Tk = nullptr; quiet.trace_cap = 0; quiet.trace_n = nullptr;
    double setup_ms = 0.0, loop_ms = 0.0;
    for (int l = 0; l < nlevels; ++l) {
        KCHK(vgicp_run_dev(c, d_src, ns, d_snrm, maps[l], l == 0 ? T0 : results[l - 1].T, l == nlevels - 1 ? p : &quiet, epsilon, &results[l],
                           info ? info + (size_t)l * KSS_VGICP_NINFO : nullptr));
        results[l].pair_id = l;
        setup_ms += c->last_setup_ms; loop_ms += c->last_loop_ms;
    }
    c->last_setup_ms = setup_ms; c->last_loop_ms = loop_ms;
    return KSS_OK;
}

// ---- the same for many scans against one map (kss_icp_vgicp_batch) ----
// nscans >= 1 scans in lockstep, every scan on its own PairTrack.  Per pass: the per-scan table (step, rotation, e, active flag)
// rewritten in pinned memory and copied in one transfer, the batch's rows launch -- pass 0 on the caller's packed scans unmoved,
// pass k >= 1 moving every active scan by ITS last step on the way in, from the caller's scans (k = 1) or cur[(k - 1) & 1] into
// cur[k & 1] -- and its final launch into h_p2l, ONE synchronisation, then vgicp_run_dev's host step for every active scan (the
// host pool from 64 scans up, each scan on exactly one thread).  A scan that ends goes inactive in the table: the workgroups of
// the later passes leave at once for it and its record in h_p2l is not written again.  The fitness evaluation is one more pass
// with every scan active, moved by its own fin from the caller's scans.  src_off: from 0; epsilons: one per scan.
int vgicpb_run_dev(kss_ctx* c, const float* d_src, const int64_t* src_off, const float* d_snrm, int nscans, const kss_vmap* map,
                   const kss_icp_params* p, const double* epsilons, kss_icp_result* results, double* info_all) {
    HIPCHK(c, hipSetDevice(c->device));
    const kss_icp_params& P = *p;
    const auto t0 = std::chrono::steady_clock::now();
    const int np = nscans;
    std::vector<PairbDesc> desc((size_t)np);
    int64_t total_rows = 0;
    for (int i = 0; i < np; ++i) {
        PairbDesc& d = desc[i];
        d.src_base = src_off[i]; d.ns = src_off[i + 1] - src_off[i];
        d.tgt_off = 0; d.nt = 0; d.overlap = 1.0;
        d.row_base = (int32_t)total_rows; d.nrows = stream_blocks(d.ns);
        total_rows += d.nrows;
        if (total_rows > PAIRB_INDEX_MAX) return set_err(c, KSS_ERR_ARG, "icp_vgicp_batch: batch too large for 32-bit indexing");
    }
    const int64_t total_src = src_off[np];
    KCHK(stage_pairb(c, desc, true));
    KCHK(ensure(c, c->p2l_rows, (size_t)total_rows * P2L_NSUMS * sizeof(double)));
    for (DevBuf& b : c->cur) KCHK(ensure(c, b, (size_t)total_src * 3 * sizeof(float)));
    KCHK(ensure(c, c->pb_gicp, (size_t)np * sizeof(VgicpbPass)));
    KCHK(ensure_pinned(c, c->h_gicp, c->h_gicp_cap, (size_t)np * sizeof(VgicpbPass)));
    KCHK(ensure_pinned(c, c->h_p2l, c->h_p2l_cap, (size_t)np * P2L_NSUMS * sizeof(double)));
    PairMode M;
    M.plane = true; M.gicp = true;
    VgicpbPass* hpass = (VgicpbPass*)c->h_gicp;
    float* d_cur[2] = {(float*)c->cur[0].p, (float*)c->cur[1].p};
    const double* hrec = (const double*)c->h_p2l;   // np records of P2L_NSUMS doubles
    VgicpbArgs a = {map->dev(), nullptr, nullptr, d_snrm, P.max_corr_dist * P.max_corr_dist, (const PairbDesc*)c->pb_desc.p,
                    (const int32_t*)c->pb_rowpair.p, (const VgicpbPass*)c->pb_gicp.p, (double*)c->p2l_rows.p};
    a.nb = map->nb;
    std::vector<PairTrack> tr((size_t)np, PairTrack(P));
    std::vector<int> active((size_t)np, P.max_iterations > 0 ? 1 : 0);
    std::vector<double> last((size_t)np * KSS_VGICP_NINFO, 0.0);
    for (int i = 0; i < np; ++i) { last[(size_t)i * KSS_VGICP_NINFO + 1] = (double)desc[i].ns; last[(size_t)i * KSS_VGICP_NINFO + 3] = (double)map->b.nvox; }
    // the table as the next launch reads it (T: the row-major 4 x 4 whose upper three rows the scan's sources are moved by), one
    // copy, rows + final into h_p2l, one synchronisation
    auto pass = [&](bool fitness, const float* d_in, float* d_out, bool move) -> int {
        ProfScope ps(c, KSS_K_CORR_REDUCE);
        for (int i = 0; i < np; ++i) {
            VgicpbPass& e = hpass[i];
            std::memcpy(e.t, fitness ? tr[i].fin : tr[i].tk, sizeof e.t);
            std::memcpy(e.r, rot_of(tr[i].fin).r, sizeof e.r);
            e.active = fitness ? 1 : active[i];
            e.e = 1.0 - epsilons[i];
        }
        HIPCHK(c, hipMemcpyAsync(c->pb_gicp.p, hpass, (size_t)np * sizeof(VgicpbPass), hipMemcpyHostToDevice, c->stream));
        a.in = d_in; a.out = d_out;
        launch_vgicpb_rows(c->stream, (int)total_rows, move, a);
        launch_vgicpb_final(c->stream, np, a, (double*)c->h_p2l_dev);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return KSS_OK;
    };
    if (P.trace_n) *P.trace_n = 0;
    int n_active = P.max_iterations > 0 ? np : 0;
    const auto t1 = std::chrono::steady_clock::now();
    for (int it = 0; n_active > 0; ++it) {
        KCHK(pass(false, it <= 1 ? d_src : d_cur[(it - 1) & 1], it == 0 ? nullptr : d_cur[it & 1], it > 0));
        std::atomic<int> finished{0};
        auto solve = [&](int pb, int pe) {
            int fin_here = 0;
            for (int i = pb; i < pe; ++i) {
                if (!active[i]) continue;
                const double* s = hrec + (size_t)i * P2L_NSUMS;
                last[(size_t)i * KSS_VGICP_NINFO] = s[0]; last[(size_t)i * KSS_VGICP_NINFO + 2] = s[30];
                double unused[KSS_SIM_NINFO] = {};
                if (!pair_host_step(P, M, s, unused, tr[i], i == 0)) { active[i] = 0; ++fin_here; }
            }
            finished.fetch_add(fin_here, std::memory_order_relaxed);
        };
        if (np >= 64) {
            std::atomic<int> next{0};
            constexpr int kBlock = 64;   // scans claimed at a time (pairs_loop's grain)
            c->pool.parallel_for(np, [&](int, int) {
                for (;;) {
                    const int pb = next.fetch_add(1) * kBlock;
                    if (pb >= np) break;
                    solve(pb, std::min(np, pb + kBlock));
                }
            });
        } else {
            solve(0, np);
        }
        n_active -= finished.load(std::memory_order_relaxed);
    }
    for (int i = 0; i < np; ++i) fill_result(results[i], tr[i].fin, tr[i].iters, tr[i].converged, tr[i].state, tr[i].last_mse, 0.0, i);
    if (P.compute_fitness) {   // [28] / [0] of one more evaluation at fin_i * scan i, over the sources that have a voxel (kept ones)
        KCHK(pass(true, d_src, d_cur[0], true));
        for (int i = 0; i < np; ++i) results[i].fitness = hrec[(size_t)i * P2L_NSUMS + 28] / hrec[(size_t)i * P2L_NSUMS];
    }
    if (info_all) std::memcpy(info_all, last.data(), last.size() * sizeof(double));
    const auto t2 = std::chrono::steady_clock::now();
    c->last_setup_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
    c->last_loop_ms = std::chrono::duration<double, std::milli>(t2 - t1).count();
    return KSS_OK;
}


// tau / m / k / kept of n squared distances on the device (kss_trim_threshold_dev)
int trim_threshold_dev(kss_ctx* c, const float* d_d2, int64_t n, double max_d2, double overlap, double* info) {
    HIPCHK(c, hipSetDevice(c->device));
    KCHK(ensure(c, c->trim_rows, trim_rows_bytes(n)));
    KCHK(ensure(c, c->trim_state, TRIM_NSTATE * sizeof(TrimState)));
    KCHK(ensure_pinned(c, c->h_p2l, c->h_p2l_cap, (P2L_NSUMS + KSS_TRIM_NINFO) * sizeof(double)));
    launch_trim_select(c->stream, d_d2, n, max_d2, overlap, (unsigned*)c->trim_rows.p, (TrimState*)c->trim_state.p,
                       (double*)c->h_p2l_dev + P2L_NSUMS);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::memcpy(info, (const double*)c->h_p2l + P2L_NSUMS, KSS_TRIM_NINFO * sizeof(double));
    return KSS_OK;
}


// per-pair descriptors (and the row -> pair table) of the batched kernels, uploaded once per call
static int stage_pairb(kss_ctx* c, const std::vector<PairbDesc>& desc, bool rows) {
    std::vector<int32_t> row_pair;
    if (rows)
        for (size_t p = 0; p < desc.size(); ++p) row_pair.insert(row_pair.end(), (size_t)desc[p].nrows, (int32_t)p);
    KCHK(ensure(c, c->pb_desc, desc.size() * sizeof(PairbDesc)));
    HIPCHK(c, hipMemcpyAsync(c->pb_desc.p, desc.data(), desc.size() * sizeof(PairbDesc), hipMemcpyHostToDevice, c->stream));
    if (rows) {
        KCHK(ensure(c, c->pb_rowpair, row_pair.size() * sizeof(int32_t)));
        HIPCHK(c, hipMemcpyAsync(c->pb_rowpair.p, row_pair.data(), row_pair.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));   // pageable sources about to go out of scope
    return KSS_OK;
}

int pairs_run_dev(kss_ctx* c, const float* d_src, const int64_t* src_off, const float* d_tgt, const int64_t* tgt_off, const float* d_nrm,
                  int npairs, const kss_icp_params* p, const PairMode& M, const double* overlaps, kss_icp_result* results, double* info_all,
                  const RobustScale* rscales, const double* gicp_eps, const int32_t* symm_aligns) {
    KCHK(pair_mode_check(c, "pairs_run", M, d_nrm, true, rscales, gicp_eps, symm_aligns));
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<int64_t> ns(npairs), nt(npairs);
    for (int i = 0; i < npairs; ++i) { ns[i] = src_off[i + 1] - src_off[i]; nt[i] = tgt_off[i + 1] - tgt_off[i]; }
    IcpPlan pl;
    const auto t0 = std::chrono::steady_clock::now();
    KCHK(restore_zero_at_rest(c));
    DirtyGuard guard(c);
    c->timing = false;
    KCHK(build_plan(c, ns.data(), nt.data(), npairs, false, p->nn_sources_per_thread, p->nn_target_splits, p->nn_mode, pl));
    KCHK(stage_plan(c, pl));
    std::vector<PairbDesc> desc((size_t)npairs);
    int64_t total_rows = 0;
    for (int i = 0; i < npairs; ++i) {
        PairbDesc& d = desc[i];
        d.src_base = pl.g[i].src_base; d.ns = ns[i];
        // (the source normals are packed like the caller's sources and read by src_base + i)
        if ((M.gicp || M.symm) && d.src_base != src_off[i]) return set_err(c, KSS_ERR_ARG, "pairs_run: the plan's source segments are not the caller's offsets");
        d.tgt_off = tgt_off[i]; d.nt = nt[i];
        d.overlap = M.trimmed ? overlaps[i] : 1.0;
        d.row_base = (int32_t)total_rows; d.nrows = stream_blocks(ns[i]);
        total_rows += d.nrows;
        if (total_rows > 0x7fff0000ll) return set_err(c, KSS_ERR_ARG, "batch too large for 32-bit indexing");
    }
    KCHK(stage_pairb(c, desc, true));
    KCHK(ensure(c, c->p2l_idx, (size_t)pl.total_src * sizeof(int32_t)));
    KCHK(ensure(c, c->p2l_d2, (size_t)pl.total_src * sizeof(float)));
    KCHK(ensure(c, c->p2l_rows, (size_t)total_rows * P2L_NSUMS * sizeof(double)));
    KCHK(ensure(c, c->trim_state, (size_t)std::max(npairs, TRIM_NSTATE) * sizeof(TrimState)));
    bool rob_select = false;
    if (M.robust) {   // the per-pair scale table; the keys of the plane metric's median where a pair asks for one
        for (int i = 0; i < npairs; ++i) rob_select = rob_select || rscales[i].autoscale != 0;
        KCHK(upload(c, c->pb_rscale, rscales, (size_t)npairs * sizeof(RobustScale)));
        HIPCHK(c, hipStreamSynchronize(c->stream));   // (the caller's table may be pageable and short-lived)
        if (rob_select && M.plane) KCHK(ensure(c, c->rob_keys, (size_t)pl.total_src * sizeof(float)));
    }
    if (M.gicp || M.symm) KCHK(stage_pass_table(c, M, npairs, gicp_eps, symm_aligns));
    if (M.unique) {   // one claim table over the batch's targets (pair p's slots at tgt_off[p], counted from 0), the filtered idx / d2
        if (tgt_off[0] != 0) return set_err(c, KSS_ERR_ARG, "pairs_run: the target offsets must start at 0");
        KCHK(ensure(c, c->o2o_table, o2o_table_bytes(tgt_off[npairs], npairs)));
        KCHK(ensure(c, c->o2o_idx, (size_t)pl.total_src * sizeof(int32_t)));
        KCHK(ensure(c, c->o2o_d2, (size_t)pl.total_src * sizeof(float)));
    }
    if (M.mutual) {   // the filtered idx / d2; every pair's grid over its own target's box, the workspace and the cell-ordered sources
        if (tgt_off[0] != 0) return set_err(c, KSS_ERR_ARG, "pairs_run: the target offsets must start at 0");
        KCHK(ensure(c, c->o2o_idx, (size_t)pl.total_src * sizeof(int32_t)));
        KCHK(ensure(c, c->o2o_d2, (size_t)pl.total_src * sizeof(float)));
        KCHK(recip_setup(c, d_tgt, desc, pl.total_src, "pairs_run"));
    }
    KCHK(ensure_pinned(c, c->h_p2l, c->h_p2l_cap, (size_t)npairs * (P2L_NSUMS + KSS_TRIM_NINFO + 2) * sizeof(double)));   // (+ m, or m and u)
    KCHK(pack_clouds(c, pl, d_src, src_off, d_tgt, tgt_off, KSS_F32));
    KCHK(grid_setup(c, pl));
    KCHK(grid_setup_batch(c, pl));
    return pair_run_loop(c, pl, t0, guard, *p, M, d_tgt, d_nrm, false, rob_select, results, info_all);
}

// tau / m / k / kept of nseg segments of squared distances in one launch (kss_trim_threshold_batch_dev)
int trim_threshold_batch_dev(kss_ctx* c, const float* d_d2, const int64_t* off, int nseg, double max_d2, const double* overlaps, double* info_all) {
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<PairbDesc> desc((size_t)nseg);
    for (int i = 0; i < nseg; ++i) {
        PairbDesc& d = desc[i];
        d.src_base = off[i]; d.ns = off[i + 1] - off[i];
        d.tgt_off = 0; d.nt = 0; d.overlap = overlaps[i]; d.row_base = 0; d.nrows = 0;
    }
    KCHK(stage_pairb(c, desc, false));
    KCHK(ensure(c, c->trim_state, (size_t)std::max(nseg, TRIM_NSTATE) * sizeof(TrimState)));
    KCHK(ensure_pinned(c, c->h_p2l, c->h_p2l_cap, (size_t)nseg * (P2L_NSUMS + KSS_TRIM_NINFO) * sizeof(double)));
    launch_pairb_select(c->stream, d_d2, (const PairbDesc*)c->pb_desc.p, nseg, nullptr, max_d2, (TrimState*)c->trim_state.p, (double*)c->h_p2l_dev);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::memcpy(info_all, c->h_p2l, (size_t)nseg * KSS_TRIM_NINFO * sizeof(double));
    return KSS_OK;
}

// the one-to-one filter alone (kss_o2o_filter[_batch]_dev): the loops' three launches over nseg segments, then both counters of
// every segment read back (each holds its count minus one)
int o2o_filter_dev(kss_ctx* c, const int32_t* d_idx, const float* d_d2, const int64_t* off, const int64_t* nts, int nseg, double max_d2,
                   int32_t* d_idx_out, float* d_d2_out, double* info_all) {
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<int64_t> tgt_off((size_t)nseg + 1, 0);   // (one table over all segments' targets, counted from 0)
    for (int i = 0; i < nseg; ++i) tgt_off[i + 1] = tgt_off[i] + nts[i];
    std::vector<PairbDesc> desc;
    int64_t total_rows = 0;
    if (!pairb_desc_of(off, tgt_off.data(), nseg, desc, total_rows)) return set_err(c, KSS_ERR_ARG, "o2o_filter: batch too large for 32-bit indexing");
    const int64_t total_tgt = tgt_off[nseg];
    KCHK(stage_pairb(c, desc, true));
    KCHK(ensure(c, c->o2o_table, o2o_table_bytes(total_tgt, nseg)));
    unsigned* d_counters = (unsigned*)((unsigned long long*)c->o2o_table.p + total_tgt);
    const O2oArgs oa = {d_idx, d_d2, (const PairbDesc*)c->pb_desc.p, (const int32_t*)c->pb_rowpair.p, nullptr, max_d2,
                        (unsigned long long*)c->o2o_table.p, d_counters, d_idx_out, d_d2_out, nullptr};
    if (launch_o2o(c->stream, (int)total_rows, total_tgt, nseg, oa) != 0) return set_err(c, KSS_ERR_HIP, "hipMemsetAsync(claim table)");
    HIPCHK(c, hipGetLastError());
    std::vector<unsigned> cnt((size_t)nseg * 2);
    HIPCHK(c, hipMemcpyAsync(cnt.data(), d_counters, cnt.size() * sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (size_t q = 0; q < cnt.size(); ++q) info_all[q] = (double)(cnt[q] + 1u);
    return KSS_OK;
}

// the reciprocal filter alone (kss_recip_filter[_batch]_dev) over nseg >= 1 segments: the loops' setup and their reset and four
// launches on packed float triples, then every segment's counters read back (each holds its count minus one).  lone: the single-pair
// entry's one segment, launched as the single-pair loop launches it
int recip_filter_dev(kss_ctx* c, const float* d_src, const int64_t* off, const float* d_tgt, const int64_t* tgt_off, int nseg,
                     const int32_t* d_idx, const float* d_d2, double max_d2, bool nn_fma, int32_t* d_idx_out, float* d_d2_out,
                     double* info_all, bool lone) {
    HIPCHK(c, hipSetDevice(c->device));
    const char* who = lone ? "recip_filter" : "recip_filter_batch";
    std::vector<PairbDesc> desc;
    int64_t total_rows = 0;
    if (!pairb_desc_of(off, tgt_off, nseg, desc, total_rows))
        return set_err(c, KSS_ERR_ARG, (std::string(who) + ": batch too large for 32-bit indexing").c_str());
    if (!lone) KCHK(stage_pairb(c, desc, true));
    KCHK(recip_setup(c, d_tgt, desc, off[nseg], who, lone));
    const int64_t total_tgt = tgt_off[nseg];
    const RecipArgs ra = {{d_src, nullptr, nullptr, d_idx, d_d2, nullptr, max_d2}, d_tgt, (const PairbDesc*)c->pb_desc.p,
                          lone ? nullptr : (const int32_t*)c->pb_rowpair.p, nullptr, (const RecipPairDev*)c->recip_grids.p, c->o2o_table.p,
                          total_tgt, nseg, (float4*)c->recip_sorted.p, d_idx_out, d_d2_out, nullptr, desc[0], c->h_recip_grids[0]};
    if (launch_recip(c->stream, (int)total_rows, c->recip_total_cells, ra, nn_fma) != 0)
        return set_err(c, KSS_ERR_HIP, "hipMemsetAsync(reciprocal workspace)");
    HIPCHK(c, hipGetLastError());
    std::vector<unsigned> cnt((size_t)nseg * 4);
    HIPCHK(c, hipMemcpyAsync(cnt.data(), recip_counters(c->o2o_table.p, total_tgt), cnt.size() * sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < nseg; ++i)
        for (int q = 0; q < 3; ++q) info_all[(size_t)i * 3 + q] = (double)(cnt[(size_t)i * 4 + q] + 1u);
    return KSS_OK;
}

int nn_generic_dev(kss_ctx* c, const void* d_src, int64_t ns, const void* d_tgt, int64_t nt, int dtype,
                          int32_t* d_idx, float* d_d2, double sums_out[NSUMS]) {
    if (!c || !d_src || !d_tgt) return set_err(c, KSS_ERR_ARG, "nn: null cloud");
    if (ns <= 0 || nt <= 0) return set_err(c, KSS_ERR_ARG, "nn: empty cloud");
    HIPCHK(c, hipSetDevice(c->device));
    IcpPlan pl;
    KCHK(restore_zero_at_rest(c));
    DirtyGuard guard(c);
    KCHK(build_plan(c, &ns, &nt, 1, false, 0, 0, KSS_NN_AUTO, pl));
    KCHK(stage_plan(c, pl));
    const int64_t so[2] = {0, ns}, to[2] = {0, nt};
    KCHK(pack_clouds(c, pl, d_src, so, d_tgt, to, dtype));
    KCHK(grid_setup(c, pl));
    float I[16];
    mat4_identity(I);
    set_state(((PairState*)c->h_state)[0], I, 1, 0);
    KCHK(nn_pass(c, pl, false, (const float4*)c->src0.p, (float4*)c->cur[0].p, 1e300, d_idx, d_d2, true));
    if (sums_out) std::memcpy(sums_out, c->h_sums, NSUMS * sizeof(double));
    guard.ok = true;
    return KSS_OK;
}


}  // namespace kss
