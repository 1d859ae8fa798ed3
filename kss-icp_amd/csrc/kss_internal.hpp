// kss_internal.hpp -- shared declarations between the HIP kernels (kss_kernels.hip) and the
// C-ABI / host drivers (kss_ctx.hpp, kss_engine.hip, kss_api.hip).  Product code; gfx950 only.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "../../include/kssicp.h"
#include "kss_handover.hpp"
#include "kss_host_math.hpp"

namespace kss {

// ---- device-visible descriptors ---------------------------------------------------------------
// Per-pair state re-uploaded every ICP iteration (64 B): rows 0..2 of the Matrix4f to apply to
// the source on load, and whether the pair still iterates.
struct alignas(16) PairState {
    float m[12];
    int32_t active;
    int32_t apply;   // 0: copy source unchanged (identity guess, PCL copies the cloud)
    int32_t pad[2];
};

// One NN-sweep workgroup = (block of sources of one pair) x (one target split).
struct alignas(16) NNWork {
    int32_t pair;
    int32_t src_begin;   // first source point (global index into the float4 source arrays)
    int32_t src_count;   // <= 256 * S
    int32_t tgt_begin;   // first target point of this split (global index into tgt4), multiple of TILE from pair base
    int32_t tgt_count;   // targets in this split, multiple of TILE (sentinel padded)
    int32_t tgt_pair_base;  // first target of the pair (idx written relative to it)
    int32_t key_begin;   // where this block's keys start: keys[key_begin + local_source]
    int32_t write_src;   // split 0 writes the transformed sources
};

// One correspondence-reduce workgroup = 256 consecutive sources of one pair.
struct alignas(16) RedWork {
    int32_t pair;
    int32_t src_begin;
    int32_t src_count;      // <= 256
    int32_t key_begin;      // keys[key_begin + s * key_stride + t]
    int32_t key_stride;     // distance between splits (= padded source count of the pair)
    int32_t n_split;
    int32_t tgt_pair_base;
    int32_t partial_index;  // row in the partial-sums array
};

struct PairRed {            // final reduce: rows [first, first+count) of partials -> sums[pair]
    int32_t first;
    int32_t count;
};

// Uniform cell list over the target's bounding box (kss_grid.hip)
struct GridParams {
    float ox, oy, oz;   // bbox minimum
    float h, inv_h;     // cell edge
    float eps;          // absolute slack covering f32 rounding of the cell assignment
    int32_t gx, gy, gz; // cells per axis (x fastest in the linear cell index)
    int32_t rcap;       // shells searched before a query falls back to the brute-force list pass
};

// per-pair entry of the batched cell list (device table)
struct alignas(16) GridPairDev {
    GridParams gp;
    int32_t cell_base;          // first cell of this pair in the global cell arrays
    int32_t tgt_base, tgt_n;    // target segment in tgt4 (padded layout) and its real point count
    int32_t src_base, src_n;    // source segment
    int32_t tgt_pad;            // slots of the target segment in tgt4 (multiple of NN_TILE, +inf sentinels behind tgt_n)
    int32_t row_base, n_rows;   // this pair's chunks of 512 sources = workgroups of the fused pass = partial rows
    int32_t sorted_base;        // first slot of this pair's targets in the cell-ordered array (sum of the earlier pairs' target counts)
};

// one pair's target segment for the batched pack kernel
struct PackSeg {
    int64_t in_off;     // first point in the caller's packed array
    int64_t out_base;   // first slot in tgt4
    int64_t n;          // real points; slots [n, next segment) are sentinel padding
};

// one value of a row handed over between the workgroups of a reduction: {bits(value), sequence number} (kss_device.hpp)
struct alignas(16) Granule { unsigned long long bits, seq; };

// arguments of the fused cell-list pass (kss_grid.hip: grid_pass_kernel), by value
struct PassArgs {
    const float4* src_in; float4* src_out;      // cell-sorted sources (.w = original index): read, transformed copy written
    const int32_t* cell_start;                  // exclusive prefix of the cell counts; [-1] and [cells + 1] are readable
    const float4* sorted;                       // targets in cell order, .w = index within the pair's target
    const float4* tgt4;                         // targets in original order (fallback sweep, SEARCH = false gathers)
    float4* nn_win;                             // per source: its last winner {x, y, z, index in the pair's target}; .w = ~0: none
    float2* nn_state;                           // per source: {B, acc} of the skip test (grid_pass_kernel, phase A)
    int32_t chained;                            // 1: src_in is what the previous search pass wrote (its queries): displacements are measurable;
                                                // 2: the pair's state names the work buffer its last pass wrote (fitness pass)
    const float4* src_last0; const float4* src_last1;   // ... the two work buffers
    float skin;                                 // pruning radius grows by skin * cell edge; < 0: never skip (A/B switch)
    unsigned long long* keys;                   // single pair: key of the sources left to the list pass
    int32_t* list; int32_t* list_count;         // single pair: those sources
    const GridPairDev* pairs;                   // BATCH: per-pair table
    const int32_t* row_pair;                    // BATCH: pair of every row (= workgroup)
    const PairState* state;                     // BATCH: per-pair transforms; single pair: host-mapped transform of a gated launch or null
    GridPairDev pair0; PairState ps0;           // single pair: by value (no upload per iteration)
    int32_t total_rows, use_prev;
    int32_t gate_polls;                         // bound of the gate's poll loop (a kernel nobody answers leaves without touching anything)
    int32_t chain_len, gate_slot;               // chained launch: passes run by this one launch (1: a plain launch); first of the two gate records
    float4* src_alt;                            // chained launch: the other work buffer (== src_in), written by every second pass
    int32_t gate_seq;                           // gated single-pair launch: the stamp `state->pad[1]` must carry
    int32_t defer_pairs;                        // BATCH with more pairs than compute units: its pair count -- gridb_finalize_kernel adds
                                                // the rows up in the next launch (0: the pair's first workgroup, in this one)
    unsigned int* gate_dev;                     // ... and the device-side copy of the record (five 16-byte granules)
    double max_d2;
    Granule* rows;                              // NSUMS granules per row (kss_device.hpp: the row hand-over)
    unsigned long long* pub; unsigned long long seq;
    int32_t* idx_out; float* d2_out;
    unsigned long long* stamps;                 // diagnostics (null in production): see KSS_STAMP below
    int32_t test_torn;                          // test hook: one result slot is first stored with data that does not fit its check word
};

// ---- the pair-resident ICP kernel (kss_resident.hip) ---------------------------------------------------------------
constexpr int RES_THREADS = 1024;     // lanes of the workgroup that holds one pair
constexpr int RES_SMAX = 10;          // sources per lane: a pair of up to 10240 sources lives in registers
constexpr int RES_NQ = 640;           // search requests queued per round (the rest is queued again, or searched by its own lane)
constexpr int RES_QW = 4;             // words per request {query, pruning radius}; answered in place {winner | runner-up << 16, bound, fell back}
constexpr int RES_G = 4;              // source slots whose wave totals are in LDS at a time
constexpr int RES_LDS_MAX = 160 * 1024 - 256;   // dynamic LDS of a workgroup (the rest: its few static words)
struct ResArgs {
    const GridPairDev* pairs;                   // per-pair table (cell grid, segments, rows)
    const int32_t* cell_start;                  // exclusive prefix of the cell counts (global positions in `sorted`)
    const float4* sorted;                       // targets in cell order, .w = index within the pair's target
    const float4* src0;                         // sources in cell order, .w = global source index
    unsigned int* gate;                         // per pair 32 words of fine-grained device memory the host stores into (BAR)
    unsigned long long* pub;                    // host-mapped result slots: per pair NSUMS x {bits, seq | check << 32}
    unsigned long long seq0;                    // pass k of a pair publishes under seq0 + k
    unsigned int stamp0;                        // ... and then waits for the gate record stamped stamp0 + k + 1
    double max_d2;
    float skin;                                 // pruning radius grows by skin * cell edge; < 0: never skip (A/B switch)
    int32_t gate_polls, max_passes, full_always;
    int32_t ntc, tabc;                          // LDS capacities of this launch: targets (multiple of 64), table entries (multiple of 8)
    int32_t* idx_out; float* d2_out;            // fitness pass: per-source correspondences (null: not wanted)
    unsigned long long* exit_flags;             // host-mapped, one 16-byte granule per pair: {exit_tag, pair, searches asked for, check} stored when the pair's workgroup leaves
    unsigned int exit_tag;                      // what the flag carries (the two launches of a split batch tell theirs apart)
    // A batch of more pairs than the device runs at once is run as TWO launches (kss_engine.hip, resident_loop): every pair's
    // passes [0, split_at) first, then the rest in the order of decreasing cost, predicted from the searches the first passes
    // asked for.  Between the launches a pair's registers rest in memory: position + skip room, candidates.
    const int32_t* perm;                        // workgroup -> pair (null: identity)
    int32_t first_pass, split_at;               // this launch runs passes [first_pass, split_at) (split_at 0: to the end)
    float4* st_pos; unsigned int* st_wc;        // per source (cell order): {x, y, z, room}, {winner | runner-up << 16}
    unsigned long long* stamps;                 // diagnostics (null in production)
};
size_t resident_lds_bytes(int ntc, int tabc);
int launch_resident(hipStream_t st, bool fma, int npairs, const ResArgs& a, std::string& err);

// PCL's octree bounding cube (kss_octree.hip; replayed on the host by oct_first_point / oct_adopt)
struct OctBox {
    double min[3], max[3];
    double res;
    int32_t depth;
};

constexpr int NN_TILE = 256;      // targets staged per LDS tile (one float4 per thread)
constexpr int NN_SUB = 32;        // targets per sub-tile (arg-min bookkeeping granularity)
constexpr int NN_THREADS = 256;

// pcl::octree::OctreePointCloud (1.8.1) bounding-cube rules, restated from its published source (octree_pointcloud.hpp).
// Empty octree: cube = point +- resolution / 2, then getKeyBitSize(): depth = bits of the voxel count (>= 2 per axis),
// cube centred around the box.
inline void oct_first_point(OctBox& b, const float* p) {
    const float minValue = FLT_EPSILON;
    for (int k = 0; k < 3; ++k) { b.min[k] = p[k] - b.res / 2; b.max[k] = p[k] + b.res / 2; }
    unsigned maxv = 2;
    for (int k = 0; k < 3; ++k) maxv = std::max(maxv, (unsigned)std::ceil((b.max[k] - b.min[k] - minValue) / b.res));
    b.depth = (int)std::ceil(std::log2((double)maxv) - minValue);
    const double side = (double)(1u << b.depth) * b.res;
    for (int k = 0; k < 3; ++k) {
        const double over = (side - (b.max[k] - b.min[k])) / 2.0;
        if (over > minValue) { b.min[k] -= over; b.max[k] += over; }
    }
}
// adoptBoundingBoxToPoint: while the point is outside [min, max), add a level -- the old cube becomes the child on the
// far side of every violated UPPER bound (min moves down on the other axes).  false: deeper than 21 levels.
inline bool oct_adopt(OctBox& b, const float* p) {
    const float minValue = FLT_EPSILON;
    for (;;) {
        bool up[3], any = false;
        for (int k = 0; k < 3; ++k) { up[k] = p[k] >= b.max[k]; any = any || up[k] || p[k] < b.min[k]; }
        if (!any) return true;
        if (b.depth >= 21) return false;
        double side = (double)(1u << b.depth) * b.res;
        for (int k = 0; k < 3; ++k) if (!up[k]) b.min[k] -= side;
        ++b.depth;
        side = (double)(1u << b.depth) * b.res - minValue;
        for (int k = 0; k < 3; ++k) b.max[k] = b.min[k] + side;
    }
}

// ---- kernel launchers (kss_kernels.hip) ---------------------------------------------------------
void launch_pack_f3_to_f4(hipStream_t st, const float* d_in, int64_t n, float4* d_out, int64_t n_pad, bool sentinel);
void launch_pack_f64_to_f4(hipStream_t st, const double* d_in, int64_t n, float4* d_out, int64_t n_pad, bool sentinel);
void launch_empty(hipStream_t st);
// single pair: target (sentinel padded, + one bbox partial row of 6 floats per 256 slots) and source in ONE launch
int pack_pair_bbox_rows(int64_t nt_pad);
void launch_pack_pair(hipStream_t st, int dtype, const void* d_tgt, int64_t nt, float4* d_tgt_out, int64_t nt_pad, float* d_bbox_partial,
                      const void* d_src, int64_t ns, float4* d_src_out, unsigned int* d_box_host, unsigned box_tag);
void launch_pack_batch(hipStream_t st, const void* d_in, int dtype, const PackSeg* d_seg, int nseg, int64_t total_out, float4* d_out);

void launch_nn_sweep(hipStream_t st, int S, bool fma, const NNWork* d_work, int n_work,
                     const PairState* d_state, const float4* d_src_in, float4* d_src_out,
                     const float4* d_tgt4, unsigned long long* d_keys);

void launch_nn_sweep_list(hipStream_t st, int S, bool fma, const NNWork* d_work, int n_work,
                          const PairState* d_state, float4* d_src_cur, const float4* d_tgt4,
                          unsigned long long* d_keys, const int32_t* d_list, const int32_t* d_count);
// both cell lists of a single pair (count -> scan -> scatter -> rank fix, shared launches)
void launch_grid_build_pair(hipStream_t st, const float4* d_tgt, int nt, float4* d_src, int ns, const GridParams& gp, int32_t* d_counts,
                            int32_t* d_slot, int32_t* d_start, int32_t* d_block_sums, float4* d_sorted, float4* d_tmp);
size_t scan_scratch_bytes(int n);   // scratch of the cell-count scan over n cells
int grid_pass_blocks(int total_rows);
void launch_grid_pass(hipStream_t st, bool fma, bool full, bool batch, bool search, const PassArgs& a);
void launch_gridb_bbox(hipStream_t st, const float4* d_tgt, const GridPairDev* d_pairs, int npairs, float* d_bbox);
void launch_gridb_build_targets(hipStream_t st, const float4* d_tgt, int total_tgt_pad, const GridPairDev* d_pairs, int npairs,
                                int total_cells, int32_t* d_counts, int32_t* d_start, int32_t* d_block_sums, float4* d_sorted);
void launch_gridb_sort_sources(hipStream_t st, const float4* d_src, int total_src, const GridPairDev* d_pairs, int npairs,
                               int total_cells, int32_t* d_counts, int32_t* d_start, int32_t* d_block_sums, float4* d_tmp, float4* d_out);
int gridb_lds_max_cells(bool half);
// all of a batch's cell lists, one workgroup per pair, counters in LDS sized for the largest grid of the batch (max_cells <=
// gridb_lds_max_cells(half)); half: 16-bit counters, allowed when no pair has 65536 or more targets or sources
// (false: the device refused the LDS size -- the caller builds through the global-atomic path)
bool launch_gridb_build_lds(hipStream_t st, const float4* d_tgt4, float4* d_src, float4* d_tmp, const GridPairDev* d_pairs, int npairs,
                            int32_t* d_cell_start, float4* d_sorted, int max_cells, bool half);
void launch_grid_stats(hipStream_t st, const float4* d_src, int ns, const GridParams& gp, const int32_t* d_cell_start,
                       unsigned long long* d_out /* [0] evaluations of the 3x3x3 block, [1] occupied cells */);

void launch_corr_reduce(hipStream_t st, const RedWork* d_work, int n_work, const PairState* d_state,
                        const float4* d_src, const float4* d_tgt4, const unsigned long long* d_keys,
                        double max_d2, double* d_partials, int32_t* d_idx_out, float* d_d2_out, int index_in_w);
// small batches: reduce + per-pair final sum + publication in one launch (rows as granules, d_rows: NSUMS per work item)
void launch_corr_reduce_publish(hipStream_t st, const RedWork* d_work, int n_work, const PairState* d_state,
                                const float4* d_src, const float4* d_tgt4, const unsigned long long* d_keys,
                                double max_d2, Granule* d_rows, int32_t* d_idx_out, float* d_d2_out, int index_in_w,
                                const PairRed* d_pair_red, unsigned long long* d_pub, unsigned long long seq);
// the candidate batch of a registration (pairs sharing one small target): sweep + sums + publication in ONE launch per pass
size_t cand_pass_lds_bytes(int nt_pad);
int cand_pass_blocks_per_pair(int64_t ns);
bool launch_cand_pass(hipStream_t st, bool fma, int npairs, const PairState* d_state, const float4* d_src_in, float4* d_src_out, const float4* d_tgt,
                      int nt_pad, int ns, double max_d2, Granule* d_rows, unsigned long long* d_pub, unsigned long long seq,
                      int32_t* d_idx_out, float* d_d2_out);
// ... and the same batch with every workgroup RESIDENT for the whole registration (cand_resident_kernel): the target is staged
// once, the sources stay in registers, and between passes a candidate's workgroups wait at its gate record for the transform
// the host solves from the sums its last workgroup published -- the protocol of the pair-resident engine (ResArgs), one
// launch per batch instead of one per pass.  A workgroup owns up to CAND_TPW tiles of 32 sources of ONE candidate.
constexpr int CAND_TPW = 4;
struct CandArgs {
    const float4* src0;                         // candidate p's sources at src0 + p * ns (original order)
    const float4* tgt;                          // the shared target, nt_pad points (padding at +inf)
    int32_t nt_pad, ns;
    int32_t bpp, wpp, tpw;                      // tiles per candidate, workgroups per candidate, tiles per workgroup (<= CAND_TPW)
    double max_d2;
    Granule* rows;                              // one row of NSUMS granules per tile, tagged with the launch-and-pass number
    const unsigned int* gate;                   // per candidate 32 words the host stores into through the BAR
    unsigned long long* pub;                    // host-mapped result slots
    unsigned long long seq0;
    unsigned int stamp0;
    int32_t gate_polls, max_passes;
    int32_t* idx_out; float* d2_out;            // fitness pass: per-source correspondences (null: not wanted)
    unsigned long long* exit_flags;             // ... and the last one stores {stamp0, pair, 0, check} into the candidate's host-mapped granule
    unsigned long long* stamps;                 // diagnostics (null in production): 16 per candidate, written by its workgroup 0
};
int cand_resident_capacity(bool fma, int nt_pad);   // workgroups the device keeps resident at once (0: cannot run)
int launch_cand_resident(hipStream_t st, bool fma, int npairs, const CandArgs& a, std::string& err);
// idx-driven variant for kss_cov: d2 recomputed with the reference arithmetic
void launch_corr_reduce_idx(hipStream_t st, const float* d_src3, const float* d_tgt3, const int32_t* d_idx,
                            int64_t n, double max_d2, double* d_partials, int n_blocks);
void launch_finalize_sums(hipStream_t st, const PairRed* d_pairs, int n_pairs, const double* d_partials,
                          double* d_out /* n_pairs * NSUMS, device or host-mapped */);

// pre-shape statistics of one or two clouds: two launches (sequence numbers seq_sum, seq), result published to host-mapped
// {bits, seq} slots
void launch_preshape_pair(hipStream_t st, const void* const d_xyz[2], const int64_t n[2], int dtype, Granule* d_rows,
                          double* d_cent, unsigned long long* d_pub, unsigned long long seq_sum, unsigned long long seq);
void launch_sum_columns(hipStream_t st, const double* d_partials, int n_rows, int n_cols, double* d_out);
void launch_row_sums(hipStream_t st, const double* d_partials, int n_rows, int n_cols, double scale, double* d_out);

void launch_pose_apply(hipStream_t st, const double* d_in, int64_t n, const kss_pose& pose,
                       const double cs[6], double* d_out);
constexpr int POSE_MANY = 32;
void launch_pose_apply_many(hipStream_t st, const double* d_in, int64_t n, const kss_pose& pose, const double (*cs)[6], int count, double* d_out);
void launch_transform_apply_f64(hipStream_t st, const float T[16], const double* d_in, int64_t n, double* d_out);

void launch_transform_apply_f32(hipStream_t st, const float T[16], const float* d_in, int64_t n, float* d_out);
int octree_voxels_device(hipStream_t st, const float* d_pts, int n, const OctBox& box, float* d_cen, int* m_out, std::string& err,
                         const std::function<void*(int, size_t)>& scratch);
void launch_fps(hipStream_t st, const double* d_xyz, int n, int m, double* d_mind, int32_t* d_idx, double* d_out);

int rot_search_grain(int64_t ns, int64_t nt, int g);   // sources per workgroup = targets per tile: 256 or 128
void launch_rot_search(hipStream_t st, const double* d_src, int64_t ns, const float4* d_tgt4, int64_t nt_pad /* multiple of nth */,
                       const double* d_cs /* g*2: cos,sin */, int g, double* d_partials, int n_src_blocks /* ceil(ns / nth) */, int nth);

int knn_plan_splits(int nq, int nt_pad, int k, size_t* scratch_bytes);
void launch_knn_sweep(hipStream_t st, const float4* d_qry, int nq, const float4* d_tgt, int nt_pad, int k, int32_t* d_idx, float* d_d2,
                      int n_split, void* d_scratch);
void launch_normals(hipStream_t st, const float4* d_pts, int n, const int32_t* d_knn, int k, double* d_normals);

int preshape_blocks(int64_t n);
inline int stream_blocks(int64_t n) {   // streaming kernels without a hand-over: 256 CUs x 8 workgroups, grid-stride beyond
    return (int)std::max<int64_t>(1, std::min<int64_t>(2048, (n + 255) / 256));
}

// ---- the pair metrics' correspondence sums for one pair (kss_pair.hip) ----
// One pass = [keys launch + selection] + ONE rows launch + ONE final launch.  The rows launch is pair_rows_kernel<M, SRC> over a
// metric functor M (kss_pair_device.hpp): stream_blocks(n) workgroups of 256, lane t of workgroup b takes the sources
// b * 256 + t + k * 256 * grid in ORIGINAL index order, M's per-source body, then block_sum's wave tree and fixed wave order
// into one partial row per workgroup (M::KEYS: one key per source and no rows).  The bits depend on the source count only.
// The batch walk (kss_pairb.hip) gives every pair exactly this assignment, so a pair's bits are the same alone and in a batch.
static_assert(P2L_NSUMS == KSS_P2L_NSUMS, "kss_host_math.hpp and include/kssicp.h disagree");
// where the sources and the correspondences are: src3 (packed float triples, original order) or src4 (float4; with perm: cell
// order, perm[i] = slot of original source i); d2: the NN distances (null with src3: recomputed); sn: the source normals as
// packed float triples by ORIGINAL source index (generalized and symmetric forms)
struct PairSrc {
    const float* src3; const float4* src4; const int32_t* perm; const int32_t* idx; const float* d2; const float* sn;
    double max_d2;
};
// the single-pair walk's arguments, by value: n sources against the target tgt / nrm of nt points; rows: stream_blocks(n) rows
// of M::NC doubles, keys: n floats (M::KEYS)
struct PairArgs {
    PairSrc s;
    const float* tgt; const float* nrm;
    int64_t n, nt;
    double* rows; float* keys;
};
int p2l_rows_blocks(int64_t n);   // = stream_blocks(n)
// one launch of pair_rows_kernel<M, SRC>, SRC from s.src3 / s.perm (a metric without a form for packed float triples reads src4)
template <class M>
void launch_pair_rows(hipStream_t st, const PairArgs& a, const M& m);
void launch_p2l_perm(hipStream_t st, const float4* d_src, int64_t n, int32_t* d_perm);
// one workgroup: the fixed-order column sums of the plane record's rows into d_out (device or host-mapped), slot 31 as 0
void launch_p2l_final(hipStream_t st, const double* d_rows, int nrows, double* d_out);

// ---- voxelized generalized ICP (kss_vmap.hip, kss_pair.hip) ----
// A voxel map as the kernels see it, by value: the dense cell -> voxel table over dims[0] * dims[1] * dims[2] cells (-1: empty,
// lin = (cz * dims[1] + cy) * dims[0] + cx), the packed voxel records in ascending lin and the float origin and 1 / leaf of
// f_a = floorf((x_a - lo[a]) * inv).  base: the window's first cell per axis on that lattice (kss_vmap_shift; 0
// until a shift): a point is inside iff base[a] <= f_a < base[a] + dims[a], and its local cell is f_a - base[a].
constexpr int VMAP_NSTAT = 10;                   // {N, mean x y z, S00 S01 S02 S11 S12 S22}
constexpr int64_t VMAP_MAX_CELLS = 1ll << 26;
static_assert(VMAP_NSTAT == KSS_VMAP_NSTAT, "kss_internal.hpp and include/kssicp.h disagree");
struct VmapDev {
    const int32_t* cell; const double* rec;
    float lo[3]; float inv;
    int dims[3];
    int base[3];
};
struct VmapMove { float m[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}; };   // the upper three rows of a row-major float 4 x 4
// What the build hands back: the device arrays the map owns (cell; rec with acc and lin behind it in one allocation; after an
// insert a second allocation of that kind, not in use; freed by vmap_free) and its header.
// acc: VMAP_NACC doubles per voxel, the sums {s x y z, P00 P01 P02 P11 P12 P22} whose quotients by N are the record: what an
// insert continues.  A map without a voxel (vmap_empty) holds the table alone: rec, lin and acc are null.
constexpr int VMAP_NACC = 9;
constexpr int VMAP_NINSERT = 4;                  // {points added, points not mapped, points outside the box, voxels created}
constexpr int VMAP_NSHIFT = 4;                   // {voxels kept, voxels dropped, mapped points dropped, delta}
static_assert(VMAP_NINSERT == KSS_VMAP_NINSERT && VMAP_NSHIFT == KSS_VMAP_NSHIFT, "kss_internal.hpp and include/kssicp.h disagree");
struct VmapBuilt {
    int32_t* cell = nullptr; double* rec = nullptr; int64_t* lin = nullptr; double* acc = nullptr;
    int64_t cap = 0;                          // voxels the allocation behind rec has room for (>= nvox)
    void* spare = nullptr; int64_t spare_cap = 0;   // the allocation the last insert's records left behind: the next insert's
    void* work = nullptr; size_t work_bytes = 0;    // a coarse map's flags, numbering and scan scratch (vmap_coarsen_into): kept, so
                                                    // that a refresh allocates nothing; null for every other map
    int64_t mapped = 0, nvox = 0;
    int dims[3] = {0, 0, 0};
    int base[3] = {0, 0, 0};                  // the window's first cell per axis (kss_vmap_shift); |base|, |base + dims| <= 2^24
    float lo[3] = {0, 0, 0}, inv = 0;
};
// The build: the box of the mapped targets, vmap_empty's table over it, vmap_insert's pipeline with no pose and records of exactly
// the voxel count.  Eleven to thirteen launches (the two scans take two or three each), two memsets over three tables, three
// readback copies and three synchronisations (box, voxel count, end) on st; its scratch is allocated and freed inside.  0: built; 1: no mapped target, or a grid that is not
// finite or has more than VMAP_MAX_CELLS cells; 2: out of memory; 3: a HIP error (1 - 3: nothing is held).
int vmap_build(hipStream_t st, const float* d_tgt, const float* d_nrm, int64_t nt, float inv, VmapBuilt& out);
void vmap_free(VmapBuilt& b);
// An empty map over the box lo .. hi (kss_vmap_create_box): the table of -1 alone.  0: made; 1: a box that is not finite, is
// inverted or has more than VMAP_MAX_CELLS cells; 2: out of memory; 3: a HIP error.
int vmap_empty(hipStream_t st, const float lo[3], const float hi[3], float inv, VmapBuilt& out);
// n points (device, packed float triples, with their normals) into the map b at the HOST float 4 x 4 T (null: as they are):
// kss_vmap_insert's definition.  Every allocation precedes the first store into b's cell table, which is renumbered in place; the
// new records, lin and sums are built beside b's and take their place after the last synchronisation.  2 (out of memory): b is
// what it was.  counts: the VMAP_NINSERT tallies.  Scratch is allocated and freed inside.
int vmap_insert(hipStream_t st, VmapBuilt& b, const float* d_pts, const float* d_nrm, int64_t n, const float* T, int64_t counts[VMAP_NINSERT]);
// The window of b moved by k whole cells per axis (kss_vmap_shift's definition; the caller has checked that the new base is in
// range): O(voxels), no pass over the dense table.  Every allocation precedes the first store into b's table; the survivors are
// packed into b.spare, which then changes places with the records.  2 (out of memory): b is what it was.  counts: the VMAP_NSHIFT
// tallies.  k = 0 and a map without a voxel launch nothing.
int vmap_shift(hipStream_t st, VmapBuilt& b, const int64_t k[3], int64_t counts[VMAP_NSHIFT]);
// kss_vmap_recentre's k for the centre (finite) at the slack: false where an |f_a| is above 2^24
bool vmap_recentre_k(const VmapBuilt& b, const float centre[3], int64_t slack, int64_t k[3]);
// The pyramid (kss_vmap_coarsen).  vmap_coarsen_header: lo, inv, dims and base of the k-fold coarsening of src at
// the leaf k * leaf into h (nothing is allocated).  vmap_coarsen_table: the cell table of such a header, allocated and NOT filled
// (the fill writes every cell); 2: out of memory.  vmap_coarsen_into: dst, whose lo, inv and dims are that header's, refilled from
// src's kept sums -- its table, records and work area reused where they have room; every allocation precedes the first store
// into dst, 2 (out of memory): dst is what it was.  ONE synchronisation of st, where the voxel count comes back; the two launches
// behind it are not waited for (every reader of a map is ordered behind them on st or synchronises st first).
void vmap_coarsen_header(const VmapBuilt& src, int k, double leaf, VmapBuilt& h);
int vmap_coarsen_table(VmapBuilt& h);
int vmap_coarsen_into(hipStream_t st, const VmapBuilt& src, int k, VmapBuilt& dst);
struct GicpRot;
// one rows launch of pair_rows_kernel over VgicpMetric: a.n sources (packed float triples d_in, normals a.s.sn) against the map;
// T set: every source is first moved by *T and stored to d_out (not d_in); nb: the map's neighbourhood setting, 1 (the kernels as
// they were), 7 or 27 (VgicpMetric<MOVE, true>)
void launch_vgicp_rows(hipStream_t st, const PairArgs& a, const VmapDev& v, const VmapMove* T, const float* d_in, float* d_out, const GicpRot& Rn,
                       double e, int nb);
// exclusive scan of d_counts[0 .. n) into d_start[0 .. n] (kss_grid.hip); d_scratch holds scan_scratch_bytes(n)
void launch_scan(hipStream_t st, int32_t* d_counts, int ncells, int32_t* d_start, int32_t* d_scratch, bool clear);

// ---- trimmed ICP (kss_trim.hip) ----
// What one digit of the radix select hands to the next, and the last one to the sums kernels of the same pass: the key
// prefix found so far, the rank inside the keys that carry it, m candidates, k = trim_rank_of(m, overlap); after the last digit
// cut = tau widened (-1: no candidate, nothing is kept) and kept = the candidates <= tau.  Four of them per context: step d
// reads [d] and writes [d + 1], so nothing is updated in place and nothing has to be reset between passes.
struct alignas(16) TrimState {
    unsigned prefix, pad;
    long long rank, m, k;
    double cut;
    long long kept;
};
constexpr int TRIM_NSTATE = 4;
// k of the definition: one IEEE f64 multiplication, then ceil; the device code and kss_trim_rank share this function
__host__ __device__ inline long long trim_rank_of(long long m, double overlap) {
    if (m == 0) return 0;
    const double x = overlap * (double)m;
    const long long k = (long long)ceil(x);
    return k < 1 ? 1 : k;
}
int trim_hist_blocks(int64_t n);
size_t trim_rows_bytes(int64_t n);
// four plain launches: tau / m / k of d_d2[0..n) into d_state[TRIM_NSTATE - 1] and {m, k, tau, kept} into d_info (may be
// null); d_rows holds trim_rows_bytes(n)
void launch_trim_select(hipStream_t st, const float* d_d2, int64_t n, double max_d2, double overlap, unsigned* d_rows,
                        TrimState* d_state, double* d_info);
// the KSS_NSUMS record from the point metric's rows (slots 17..19 are 0)
void launch_trim_point_final(hipStream_t st, const double* d_rows, int nrows, double* d_out);
// the similarity step's KSS_NSUMS record from SimMetric's rows (slot 17 kept, 18 and 19 are 0)
void launch_sim_final(hipStream_t st, const double* d_rows, int nrows, double* d_out);
void launch_f64_to_f32(hipStream_t st, const double* d_in, int64_t n, float* d_out);

// ---- robust ICP ----
// The scale of a call: fixed (c2 = scale^2) or automatic (K = (tune * 1.4826)^2 and min2 = min_scale^2, all formed on the
// host; the pass's c2 = robust_scale2_of(median key) is derived by the rows and final kernels from the selection's TrimState).
struct RobustScale {
    int loss = 0, autoscale = 0;
    double c2 = 0.0, K = 0.0, min2 = 0.0;
};
// the weighted record's final launches: the column sums of d_rows (KSS_P2L_NSUMS or KSS_NSUMS doubles) into d_out and {m, c2,
// sum of weights, cnt} into d_info.  d_sel: the TrimState the selection's last step left (automatic scale), null for the fixed one.
void launch_robust_plane_final(hipStream_t st, const double* d_rows, int nrows, const RobustScale& rs, const TrimState* d_sel, double* d_out,
                               double* d_info);
void launch_robust_point_final(hipStream_t st, const double* d_rows, int nrows, const RobustScale& rs, const TrimState* d_sel, double* d_out,
                               double* d_info);


// ---- the same metrics for many pairs per call (kss_pairb.hip) ----
// one pair (or one segment of kss_trim_threshold_batch) as the batched kernels see it
struct alignas(16) PairbDesc {
    int64_t src_base, ns;      // the pair's sources in the batch-wide per-source arrays (idx, d2, perm)
    int64_t tgt_off, nt;       // its target in the caller's packed float triples (points), normals alike
    double overlap;
    int32_t row_base, nrows;   // its partial rows: stream_blocks(ns) of them, the single-pair kernel's count
};
// What one pass of one pair needs beyond its descriptor (generalized and symmetric forms): the rotation block of the transform
// accumulated so far (row-major, the float bits the single-pair call takes as Rn), the pair's align_normals (symmetric) and
// e = 1 - epsilon (generalized).  One entry per pair; the host rewrites the rotations before every pass, align / e are staged
// once per call.
struct PairPass {
    float r[9];
    int32_t align;
    double e;
};
static_assert(sizeof(PairPass) == 48, "the host and the device table share this layout");
// The batch walk's arguments, by value: the sources and the clouds batch-wide (s.src3 is null; s.sn packed like the sources, by
// global original index), the per-pair tables -- desc, state (the NN pass's per-pair states, null: every pair is active), rs
// (robust: one RobustScale per pair), ts (trimmed: the selection's TrimState per pair; robust: the median key's, written for
// the automatic pairs alone), pass (generalized / symmetric) --, the row -> pair table, total_rows rows and the batch-wide keys.
struct PairbArgs {
    PairSrc s;
    const float* tgt; const float* nrm;
    const PairbDesc* desc; const int32_t* row_pair; const PairState* state; const RobustScale* rs; TrimState* ts; const PairPass* pass;
    double* rows; float* keys;
};
// one launch of pairb_rows_kernel<M, perm given> over total_rows = the sum of the pairs' stream_blocks(ns) workgroups:
// every active pair's rows (M::KEYS: every active automatic pair's keys by global source index, NaN: no candidate)
template <class M>
void launch_pairb_rows(hipStream_t st, int total_rows, const PairbArgs& a);
// one launch each, one workgroup per pair:
// every active pair's TrimState into d_ts[pair] and {m, k, tau, kept} into d_info[pair * KSS_TRIM_NINFO]
void launch_pairb_select(hipStream_t st, const float* d_d2, const PairbDesc* d_desc, int npairs, const PairState* d_state, double max_d2,
                         TrimState* d_ts, double* d_info);
// the median key of every active AUTOMATIC pair into a.ts[pair] (the others' entries are not written), over d_keys within bound
void launch_pairb_robust_select(hipStream_t st, int npairs, const PairbArgs& a, const float* d_keys, double bound);
// every active pair's record into d_out[pair * KSS_P2L_NSUMS] (the point metric fills KSS_NSUMS of them) ...
// (sim: the similarity step's record, slot 17 kept)
void launch_pairb_final(hipStream_t st, bool plane, int npairs, const PairbArgs& a, double* d_out, bool sim = false);
// ... and the weighted one, with {m, c2, sum of weights, cnt} into d_info[pair * KSS_ROBUST_NINFO]
void launch_pairb_robust_final(hipStream_t st, bool plane, int npairs, const PairbArgs& a, double* d_out, double* d_info);

// ---- voxelized generalized ICP for many scans per call (kss_pairb.hip) ----
// What one pass of one scan needs beyond its descriptor: the float 3 x 4 step T_{k-1} its sources take on the way in (read by the
// moving form only), the rotation block of its accumulated transform (the float bits the single-scan call takes as Rn),
// e = 1 - epsilon and whether the scan still takes part.  One entry per scan; the host rewrites the table before every pass.
struct VgicpbPass {
    float t[12];
    float r[9];
    int32_t active;
    double e;
};
static_assert(sizeof(VgicpbPass) == 96, "the host and the device table share this layout");
// The batch walk's arguments, by value: the map, the batch-wide positions in (packed float triples by global original index) and,
// moving form, out (another array), the source normals laid out like them, the per-scan descriptors (src_base, ns, row_base,
// nrows are read), the row -> scan table, the pass table and total_rows rows of KSS_P2L_NSUMS doubles.
struct VgicpbArgs {
    VmapDev v;
    const float* in; float* out; const float* sn;
    double max_d2;
    const PairbDesc* desc; const int32_t* row_pair; const VgicpbPass* pass;
    double* rows;
    int nb = 1;   // the map's neighbourhood setting (kss_vmap_set_neighbourhood): 1, 7 or 27
};
// one launch over total_rows = the sum of the scans' stream_blocks(ns) workgroups: every active scan's rows; move: its sources
// are first moved by its own pass[scan].t and stored to a.out; a.nb of 7 or 27: the neighbourhood kernels
void launch_vgicpb_rows(hipStream_t st, int total_rows, bool move, const VgicpbArgs& a);
// one workgroup per scan: every active scan's record into d_out[scan * KSS_P2L_NSUMS] (device or host-mapped), slot 31 as 0
void launch_vgicpb_final(hipStream_t st, int nscans, const VgicpbArgs& a, double* d_out);

// ---- one-to-one rejection (kss_o2o.hip) ----
// The filter's arguments, by value: idx / d2 the NN pass's, batch-wide by original source index (a pair's at desc[p].src_base, its
// idx counting inside its own target); desc / row_pair / state as in PairbArgs (row_pair null: the one pair desc[0]; state null:
// every pair is active); table: one uint64 per target of the batch, pair p's at desc[p].tgt_off; counters: two uint32 per pair
// behind the table ({m, u}, each MINUS ONE: they start at all ones with the table); idx_out / d2_out: the filtered arrays, laid out
// like idx / d2 (either may be null, either may be its input); info_m: one double per pair, m as the resolve launch publishes it
// (device or host-mapped, may be null).
struct O2oArgs {
    const int32_t* idx; const float* d2;
    const PairbDesc* desc; const int32_t* row_pair; const PairState* state;
    double max_d2;
    unsigned long long* table; unsigned* counters;
    int32_t* idx_out; float* d2_out;
    double* info_m;
};
size_t o2o_table_bytes(int64_t total_tgt, int npairs);
// table reset, claim, resolve: three launches for total_rows = the sum of the pairs' nrows workgroups.  0, or the hipError_t of the reset.
int launch_o2o(hipStream_t st, int total_rows, int64_t total_tgt, int npairs, const O2oArgs& a);

// ---- reciprocal rejection, one pair or many per call (kss_recip.hip) ----
// The uniform cell grid a pair's moving sources are binned into every pass: fixed on the host once per call from the bounding box
// of the pair's target (recip_grid_of); a coordinate's cell is clamp(floor((v - o) * inv_h), 0, g - 1) per axis, x fastest in the
// linear index.
struct RecipGrid {
    float ox, oy, oz, inv_h;
    int32_t gx, gy, gz;
};
constexpr int RECIP_BOX_BLOCKS = 256;   // box partials of a single pair at most: 6 floats {min xyz, max xyz} each
constexpr int RECIP_GMAX = 64;          // cells per axis at most
constexpr int RECIP_CELLS = 32768;      // cells aimed at at most per pair (the pair's one scan workgroup walks them all every pass)
// one pair's grid -- recip_grid_of(the box of ITS target, ITS source count) -- and where its cells start in the call's cell counts
struct alignas(16) RecipPairDev {
    RecipGrid g;
    int32_t cell_base;
};
static_assert(sizeof(RecipPairDev) == 32, "the host and the device table share this layout");
// The filter's arguments, by value.  s: the sources' CURRENT positions call-wide (s.src3: the filter alone, packed triples by global
// source index; else s.src4, with s.perm where the cell-list setup re-ordered them) and the NN pass's s.idx / s.d2 by original source
// index, a pair's at desc[p].src_base, idx counting inside its own target; tgt: the call's packed float triples; desc / row_pair /
// state as in O2oArgs (state null: every pair is active); grids: one RecipPairDev per pair.  row_pair null: ONE pair, whose
// descriptor and grid are lone_desc and lone_grid here in the struct -- desc and grids are not read (launch_recip takes the
// kernels' LONE instances).
// work: recip_work_bytes(total_tgt, npairs, total_cells) of workspace, all ones before every pass -- the claim table (one uint64
// per target of the call, pair p's at desc[p].tgt_off), four uint32 counters {m, u, r, unused} per pair, one uint32 per cell of
// every pair (pair p's at grids[p].cell_base), each MINUS ONE.  sorted: one float4 {x, y, z, bits(index inside the pair)} per source
// of the call, pair p's cell-ordered sources in [src_base, src_base + ns).  idx_out / d2_out: the filtered arrays, laid out like
// s.idx / s.d2 (either may be null, either may be its input); info_mu: two doubles {m, u} per pair (device or host-mapped, may be
// null).
struct RecipArgs {
    PairSrc s;
    const float* tgt;
    const PairbDesc* desc; const int32_t* row_pair; const PairState* state; const RecipPairDev* grids;
    void* work; int64_t total_tgt; int32_t npairs;
    float4* sorted;
    int32_t* idx_out; float* d2_out;
    double* info_mu;
    PairbDesc lone_desc; RecipPairDev lone_grid;
};
__host__ __device__ inline int64_t recip_cells(const RecipGrid& g) { return (int64_t)g.gx * g.gy * g.gz; }
size_t recip_work_bytes(int64_t total_tgt, int npairs, int64_t total_cells);
__host__ __device__ inline unsigned* recip_counters(void* work, int64_t total_tgt) { return (unsigned*)((unsigned long long*)work + total_tgt); }
// every pair's target box in ONE launch: `split` partials of 6 floats {min xyz, max xyz} per pair, pair p's at d_box + 6 * split * p
// (d_desc null: the one pair `lone`)
void launch_recip_bbox(hipStream_t st, const float* d_tgt, const PairbDesc* d_desc, const PairbDesc& lone, int npairs, int split, float* d_box);
// reset, claim + count, scan, scatter, resolve + check: the reset and four launches, total_rows workgroups in the walks and the
// resolve, one workgroup per pair in the scan.  0, or the hipError_t of the reset.
int launch_recip(hipStream_t st, int total_rows, int64_t total_cells, const RecipArgs& a, bool nn_fma);

// The host arithmetic of the filters' setup, free of the device (tools/recip_host_check.hip runs it under the host sanitizers).
constexpr int64_t PAIRB_INDEX_MAX = 0x7fff0000ll;   // rows, targets, cells and box partials of a call are 32-bit indices
// nseg segments as the batched kernels see them: sources [off[i], off[i + 1]), targets [tgt_off[i], tgt_off[i + 1]), the rows
// numbered in order.  false: more rows or targets than PAIRB_INDEX_MAX.
inline bool pairb_desc_of(const int64_t* off, const int64_t* tgt_off, int nseg, std::vector<PairbDesc>& desc, int64_t& total_rows) {
    desc.resize((size_t)nseg);
    total_rows = 0;
    for (int i = 0; i < nseg; ++i) {
        PairbDesc& d = desc[i];
        d.src_base = off[i]; d.ns = off[i + 1] - off[i];
        d.tgt_off = tgt_off[i]; d.nt = tgt_off[i + 1] - tgt_off[i]; d.overlap = 1.0;
        d.row_base = (int32_t)total_rows; d.nrows = stream_blocks(d.ns);
        total_rows += d.nrows;
        if (total_rows > PAIRB_INDEX_MAX || tgt_off[i + 1] - tgt_off[0] > PAIRB_INDEX_MAX) return false;
    }
    return true;
}
// The grid for n sources over the box [mn, mx] (a box that is not finite, or a point: one cell).  The cell edge aims at
// min(n / 2, RECIP_CELLS) cells over the axes of non-zero extent -- a few sources per cell for a cloud that fills its box, some tens
// for a surface -- with at most RECIP_GMAX cells per axis; an axis of zero extent gets one cell.
inline RecipGrid recip_grid_of(const float mn[3], const float mx[3], int64_t n) {
    RecipGrid g = {0.0f, 0.0f, 0.0f, 0.0f, 1, 1, 1};
    double ext[3], vol = 1.0, emax = 0.0;
    int k = 0;
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(mn[a]) || !std::isfinite(mx[a]) || mx[a] < mn[a]) return g;
        ext[a] = (double)mx[a] - (double)mn[a];
        if (ext[a] > 0.0) { ++k; vol *= ext[a]; emax = std::max(emax, ext[a]); }
    }
    if (k == 0) return g;
    const double want = (double)std::max<int64_t>(1, std::min<int64_t>(n / 2, RECIP_CELLS));
    const float h = (float)std::max(std::pow(vol / want, 1.0 / k), emax / (RECIP_GMAX - 0.5));
    const float inv_h = 1.0f / h;
    if (!(h > 0.0f) || !std::isfinite(inv_h) || !std::isfinite(h)) return g;
    g.ox = mn[0]; g.oy = mn[1]; g.oz = mn[2];
    g.inv_h = inv_h;
    int* gg[3] = {&g.gx, &g.gy, &g.gz};
    for (int a = 0; a < 3; ++a)
        *gg[a] = ext[a] > 0.0 ? (int)std::max(1.0, std::min((double)RECIP_GMAX, std::floor(ext[a] / (double)h) + 1.0)) : 1;
    return g;
}
// Every pair's {grid, first cell} from the box partials as launch_recip_bbox wrote them (`split` per pair): the cell total, or -1
// where it passes PAIRB_INDEX_MAX.
inline int64_t recip_grids_of(const float* box, int split, const std::vector<PairbDesc>& desc, std::vector<RecipPairDev>& grids) {
    grids.resize(desc.size());
    int64_t cells = 0;
    for (size_t p = 0; p < desc.size(); ++p) {
        float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (int b = 0; b < split; ++b)
            for (int k = 0; k < 3; ++k) {
                mn[k] = std::fmin(mn[k], box[(p * split + b) * 6 + k]);
                mx[k] = std::fmax(mx[k], box[(p * split + b) * 6 + 3 + k]);
            }
        grids[p].g = recip_grid_of(mn, mx, desc[p].ns);
        grids[p].cell_base = (int32_t)cells;
        cells += recip_cells(grids[p].g);
        if (cells > PAIRB_INDEX_MAX) return -1;
    }
    return cells;
}

// AIVS down-sampler (kss_aivs.hip): indices of the selected points in the reference's output order
int aivs_device(hipStream_t st, const double* d_xyz, int n, int point_num, std::vector<int32_t>& out_idx, std::string& err,
                const std::function<void*(size_t)>& scratch);

}  // namespace kss
