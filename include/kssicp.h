/*
 * kssicp.h -- C-ABI of the MI355X-native KSS-ICP registration core (libkssicp.so).
 *
 * This is the drop-in boundary UNDER the reference's C++ class surface: the mirror classes in
 * include/KSS_ICP.hpp, include/initRegistrationKSS.hpp and include/registrationMeasure.hpp
 * (same class / method / field names as the reference) call only these entry points.  The
 * reference has no FFI of its own; each entry point below cites the
 * reference code it replaces, as path:line under PS_AIS_Simplification/.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++/torch types.  Every call returns an int
 *     status (KSS_OK == 0, errors < 0) and never throws across the ABI.
 *   - Clouds are packed xyz triples: float[n][3] ("f32") or double[n][3] ("f64").
 *   - `*_dev` variants take DEVICE pointers (hipMalloc'd, or a torch tensor's data_ptr());
 *     the un-suffixed variants take HOST pointers and stage through the context's workspace.
 *   - One context per host thread / GPU.  Calls on one context are serialised on its HIP
 *     stream; distinct contexts are independent (matches the reference's "objects are
 *     independent" threading rule).
 *   - There is NO CPU fallback: every compute entry point fails with KSS_ERR_NODEVICE /
 *     KSS_ERR_HIP when no gfx950 device is usable.
 */
#ifndef KSSICP_H_
#define KSSICP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KSS_VERSION 100 /* 0.1.0 */

enum {
    KSS_OK = 0,
    KSS_ERR_ARG = -1,      /* null pointer, negative size, n == 0 where a cloud is required */
    KSS_ERR_HIP = -2,      /* a HIP runtime call failed; see kss_last_error() */
    KSS_ERR_NOMEM = -3,
    KSS_ERR_NODEVICE = -4, /* no usable GPU */
    KSS_ERR_CAPACITY = -5, /* caller-provided output buffer too small */
    KSS_ERR_RCCL = -6,
    KSS_ERR_DEGENERATE = -7 /* kss_rigid_from_p2l_sums: the 6x6 normal equations are singular (planar target ...) */
};

enum { KSS_F32 = 0, KSS_F64 = 1 };

typedef struct kss_ctx kss_ctx;

int         kss_version(void);
const char *kss_status_string(int status);
/* human-readable detail of the last failure on this context ("" if none) */
const char *kss_last_error(const kss_ctx *ctx);

/* ---- context ---------------------------------------------------------------------------- */
int   kss_ctx_create(int device_id, kss_ctx **out);                 /* owns its HIP stream */
/* borrow an existing hipStream_t (e.g. torch.cuda.current_stream().cuda_stream) */
int   kss_ctx_create_on_stream(int device_id, void *hip_stream, kss_ctx **out);
int   kss_ctx_destroy(kss_ctx *ctx);
int   kss_ctx_synchronize(kss_ctx *ctx);
void *kss_ctx_stream(kss_ctx *ctx);

/* default NN search structure of this context (KSS_NN_AUTO / _BRUTE / _GRID, see below); used whenever an
 * entry point has no nn_mode of its own or it is KSS_NN_AUTO.  Results never depend on it. */
int   kss_ctx_set_nn_mode(kss_ctx *ctx, int nn_mode);

/* per-kernel timing with HIP events recorded on the context's stream around launches of the named kernel
 * class (used by bench.py for the roofline object).  kss_profile_enable(ctx, n): 0 = off, 1 = every launch,
 * n > 1 = every n-th launch of each class (an event pair costs a few microseconds, comparable to the fused
 * cell-list launch it brackets); kss_profile_get reports the sampled launches only. */
enum { KSS_K_NN_SWEEP = 0, KSS_K_CORR_REDUCE = 1, KSS_K_PRESHAPE = 2, KSS_K_ROT_SEARCH = 3,
       KSS_K_POSE_APPLY = 4, KSS_K_GRID_NN = 5, KSS_K_GRID_BUILD = 6,
       KSS_K_GRID_CHAIN = 7,        /* chained launches of the fused pass: one entry per launch (its whole duration) */
       KSS_K_GRID_CHAIN_PASS = 8,   /* the same time, counted per ICP pass the launches ran */
       KSS_K_RESIDENT = 9,          /* pair-resident batch kernel: one entry per launch (all passes of every pair of the batch) */
       KSS_K_RESIDENT_PASS = 10,    /* the same time, counted per (pair, pass) the launches ran */
       KSS_K_COUNT = 11 };
int kss_profile_enable(kss_ctx *ctx, int on);
/* geometry of the last cell list built on this context (KSS_NN_GRID) and, when profiling is enabled, the
 * number of (source, target) distance evaluations of one search pass at the sources' initial positions:
 * out = {cell edge h, gx, gy, gz, occupied cells, evaluations per pass, n_src, n_tgt}.  All zero if no
 * grid has been built.  Used by bench.py to state the kernel's algorithmic bytes. */
int kss_grid_stats(kss_ctx *ctx, double out[8]);
int kss_profile_reset(kss_ctx *ctx);
/* synchronises the stream; total_ms = sum of event-timed durations, launches = count */
int kss_profile_get(kss_ctx *ctx, int kernel_class, double *total_ms, int64_t *launches);
/* what a HIP event pair reads around an EMPTY kernel launched into the idle stream (ms, mean of 200): an upper
 * bound of what event timing adds to a short kernel's own duration.  bench.py reports it beside its per-launch
 * durations (context for comparing them with rocprofv3's kernel trace); it is not subtracted. */
int kss_profile_event_overhead(kss_ctx *ctx, double *ms);

/* ---- (a2) KSS pre-shape: initRegistration_MiddleAlign, initRegistrationKSS.hpp:144-207 ----
 * centroid (mean of points) and mean distance to the centroid, accumulated in f64 with a
 * wavefront/LDS block reduce.  scale = r_tgt / r_src is formed by the caller (:209). */
int kss_preshape_stats(kss_ctx *ctx, const void *xyz, int dtype, int64_t n,
                       double centroid[3], double *mean_radius);
int kss_preshape_stats_dev(kss_ctx *ctx, const void *d_xyz, int dtype, int64_t n,
                           double centroid[3], double *mean_radius);
/* both clouds of a registration (:144-207 computes S and T back to back) in ONE call: two launches for the pair, no
 * stream synchronisation; bit-identical to one call per cloud.  d_tgt may be NULL (then c_tgt / r_tgt are not written). */
int kss_preshape_stats_pair_dev(kss_ctx *ctx, const void *d_src, int64_t ns, const void *d_tgt, int64_t nt, int dtype,
                                double c_src[3], double *r_src, double c_tgt[3], double *r_tgt);

/* ---- (a3,a7) pose application: initRegistration_Rotation[_Angle], :75-109 + :365-404 ----
 * p += shift; p = center + (p - center) * scale; then Rx(angle[0]), Ry(angle[1]), Rz(angle[2])
 * about the WORLD ORIGIN, all in f64 without fused multiply-add (reference arithmetic). */
typedef struct {
    double shift[3];   /* x_middle..   = c_T - c_S   (:190-192) */
    double center[3];  /* x_middle_S.. = c_T         (:186-188) */
    double scale;      /*                             (:209)     */
    double angle[3];   /* Euler angles about x, y, z              */
} kss_pose;
int kss_pose_apply(kss_ctx *ctx, const double *in, int64_t n, const kss_pose *pose, double *out);
int kss_pose_apply_dev(kss_ctx *ctx, const double *d_in, int64_t n, const kss_pose *pose, double *d_out);

/* ---- (a8) exact 1-NN correspondence: replaces pcl::KdTreeFLANN<PointXYZ>::nearestKSearch
 *      (call sites initRegistrationKSS.hpp:236,443; registrationMeasure.hpp:63,79; PCL ICP) ----
 * Brute-force LDS-tiled source x target sweep in f32.  d2 = (dx*dx + dy*dy) + dz*dz without
 * fma (FLANN L2_Simple<float>), ties -> lowest target index.  idx/d2 may be NULL. */
int kss_nn(kss_ctx *ctx, const float *src, int64_t ns, const float *tgt, int64_t nt,
           int32_t *idx, float *d2);
int kss_nn_dev(kss_ctx *ctx, const float *d_src, int64_t ns, const float *d_tgt, int64_t nt,
               int32_t *d_idx, float *d_d2);

/* ---- exact k-NN (k <= 64): pcl::KdTreeFLANN::nearestKSearch with K > 1 (ballRegionCompute.hpp:499 K = 13,
 *      Method_AIVS_SimPro.hpp:904 K = 3, Method_Octree.hpp:137, pcl::NormalEstimation K = 20) ----
 * idx / d2: nq * k entries, per query in ascending (d2, index) order; slots beyond nt hold -1 / +inf. */
int kss_knn(kss_ctx *ctx, const float *query, int64_t nq, const float *tgt, int64_t nt, int k, int32_t *idx, float *d2);
int kss_knn_dev(kss_ctx *ctx, const float *d_query, int64_t nq, const float *d_tgt, int64_t nt, int k, int32_t *d_idx, float *d_d2);

/* ---- surface normals: estimateNormal_PCL_MP_return, normalCompute.hpp:308-355 ----
 * pcl::NormalEstimationOMP semantics (k nearest neighbours incl. the point itself, float single-pass covariance,
 * closed-form smallest eigenvector, flipped towards the view point (0,0,0)) and the reference's renormalisation in
 * double.  normals: n * 3 doubles.  1 <= k <= 64 (kss_knn's range; k above n is clamped to n).  The reference uses
 * k = 20. */
int kss_normals(kss_ctx *ctx, const double *pts, int64_t n, int k, double *normals);
/* estimateNormal_RegularNormal, normalCompute.hpp:614-742 (with kss_normals: estimateNormal_PCL_MP, :358-403):
 * consistent orientation of given normals (n*3 doubles, in place) by level-synchronous propagation over the 8-NN
 * graph from point 0; a normal is negated when it points away from its parent's.  The 8-NN search runs on the
 * device, the O(8 n) propagation on the host.  Unreached points keep their normals. */
int kss_normals_orient(kss_ctx *ctx, const double *pts, int64_t n, double *normals);

/* ---- (a10) correspondence sums for TransformationEstimationSVD / umeyama (inside PCL ICP) ----
 * sums[0]=n kept (d2 <= max_d2), [1..3]=sum src, [4..6]=sum tgt[idx], [7..15]=sum src_i*tgt_j
 * (i major), [16]=sum d2 kept, [17]=sum d2 all, [18]=sum sqrt(d2) all, [19]=0.  f64, reduced
 * in a fixed order (bitwise reproducible run to run). */
#define KSS_NSUMS 20
int kss_cov(kss_ctx *ctx, const float *src, const float *tgt, const int32_t *idx, int64_t n,
            int64_t nt, double max_d2, double sums[KSS_NSUMS]);
int kss_cov_dev(kss_ctx *ctx, const float *d_src, const float *d_tgt, const int32_t *d_idx, int64_t n,
                int64_t nt, double max_d2, double sums[KSS_NSUMS]);
/* host-side: rigid transform (Umeyama without scaling, 3x3 SVD) from the sums; row-major 4x4 (with the scale: kss_sim_from_sums) */
int kss_rigid_from_sums(const double sums[KSS_NSUMS], float T[16]);

/* ---- (a4,a5) rotation search: initRegistration_Rotation(), :222-296 + :430-450 ----
 * src_preshaped: S' after the similarity of kss_pose_apply with angle = 0 (f64);
 * err receives value[g][g][g] (i-major), g = trip count of for(a=0; a<6.3; a+=6.3/step). */
int kss_rotation_search(kss_ctx *ctx, const double *src_preshaped, int64_t ns,
                        const double *tgt, int64_t nt, double step,
                        double *err, int64_t err_capacity, int *g_out);
int kss_rotation_search_dev(kss_ctx *ctx, const double *d_src_preshaped, int64_t ns,
                            const double *d_tgt, int64_t nt, double step,
                            double *err /* host */, int64_t err_capacity, int *g_out);
/* host-side (a6): accumulated grid angles (:245), global arg-min (:258-265, :291-293) and the
 * 5^3 clamped local-minimum list (:276-289, :481-522).  angle_list = idx*6.3/step triples. */
int kss_grid_angles(double step, double *angles, int capacity);
int kss_rotation_candidates(const double *err, int g, double step, double best_angle[3],
                            double *angle_list, int list_capacity, int *n_list);

/* ---- (a9,a11,a12) ICP driver: pcl::IterativeClosestPoint::align as configured at
 *      KSS_ICP.hpp:155-162 (x5), PCL 1.8.1 semantics ---- */
/* In-place sum over the ranks of a job of n doubles in HOST memory; returns 0 on success.  See `allreduce` below. */
typedef int (*kss_allreduce_fn)(void *user, double *values, int n);

typedef struct {
    int    max_iterations;             /* setMaximumIterations            KSS_ICP.hpp:159 */
    double max_corr_dist;              /* setMaxCorrespondenceDistance(1) :156 */
    double transformation_epsilon;     /* setTransformationEpsilon(1e-10) :157 */
    double euclidean_fitness_epsilon;  /* setEuclideanFitnessEpsilon(1e-3):158 */
    double abs_mse_epsilon;            /* PCL default 1e-12 */
    int    min_correspondences;        /* PCL default 3 */
    int    fixed_iterations;           /* run exactly max_iterations (benchmark mode) */
    int    nn_fma;                     /* 0: reference arithmetic; 1: fused d2 (fast, not bit-parity) */
    int    compute_fitness;            /* getFitnessScore() after align (:164) */
    int    nn_sources_per_thread;      /* tuning, 0 = auto */
    int    nn_target_splits;           /* tuning, 0 = auto */
    int    nn_mode;                    /* KSS_NN_AUTO / KSS_NN_BRUTE / KSS_NN_GRID: same results bit for bit */
    /* optional per-iteration trace for parity tests (host pointers, may be NULL) */
    double *trace_sums;                /* trace_cap * KSS_NSUMS */
    float  *trace_Tk;                  /* trace_cap * 16 */
    int     trace_cap;
    int    *trace_n;
    /* optional: the correspondences getFitnessScore() sums over -- nearest target index and squared distance of every
     * source point of pair 0 under the final transform (host pointers, n_src entries each, may be NULL; filled only
     * when compute_fitness is set) */
    int32_t *fitness_idx;
    float   *fitness_d2;
    /* optional (the single-pair exchange step): ONE registration whose SOURCE ROWS are split over several
     * ranks, target replicated.  Every rank calls kss_icp[_dev] with its own rows and the same target and parameters;
     * after each NN pass the KSS_NSUMS correspondence sums are summed over the ranks through this callback, so every
     * rank solves the same 3x3 system and applies the same transform.  The result (T, iterations, fitness over ALL
     * source rows) is identical on every rank.  NULL = single-rank registration.  Single pair only. */
    kss_allreduce_fn allreduce;
    void *allreduce_user;
} kss_icp_params;

/* NN search structure.  BRUTE: the LDS-tiled source x target sweep (north star).  GRID: exact search
 * through a uniform cell list built once per target, queries unresolved within a few cell shells fall
 * back to the brute-force sweep.  AUTO picks GRID for one large pair, BRUTE otherwise. */
enum { KSS_NN_AUTO = 0, KSS_NN_BRUTE = 1, KSS_NN_GRID = 2 };

enum { KSS_STATE_NOT_CONVERGED = 0, KSS_STATE_ITERATIONS = 1, KSS_STATE_TRANSFORM = 2,
       KSS_STATE_ABS_MSE = 3, KSS_STATE_REL_MSE = 4, KSS_STATE_NO_CORRESPONDENCES = 5,
       KSS_STATE_DEGENERATE = 6 /* the pass's normal equations were singular (plane metrics), or its kept sources had no spread
                                    (kss_icp_sim) */ };

typedef struct {
    float   T[16];       /* getFinalTransformation(), row-major Matrix4f  (:222) */
    double  fitness;     /* getFitnessScore()                             (:164) */
    double  last_mse;
    int32_t iterations;
    int32_t converged;   /* hasConverged() */
    int32_t state;
    int32_t pair_id;     /* index of the pair in a batch (global id after a gather) */
} kss_icp_result;       /* 96 bytes: the record gathered over RCCL */

int kss_icp_default_params(kss_icp_params *p);
int kss_icp(kss_ctx *ctx, const float *src, int64_t ns, const float *tgt, int64_t nt,
            const kss_icp_params *p, kss_icp_result *res);
int kss_icp_dev(kss_ctx *ctx, const float *d_src, int64_t ns, const float *d_tgt, int64_t nt,
                const kss_icp_params *p, kss_icp_result *res);
/* batch of independent registrations (KSS_ICP.hpp:102-118 candidate loop; configs C3/C5).
 * src_off/tgt_off: npairs+1 HOST offsets (in points) into the packed clouds. */
int kss_icp_batch(kss_ctx *ctx, const float *src_all, const int64_t *src_off,
                  const float *tgt_all, const int64_t *tgt_off, int npairs,
                  const kss_icp_params *p, kss_icp_result *results);
int kss_icp_batch_dev(kss_ctx *ctx, const float *d_src_all, const int64_t *src_off,
                      const float *d_tgt_all, const int64_t *tgt_off, int npairs,
                      const kss_icp_params *p, kss_icp_result *results);

/* ---- point-to-plane ICP for one pair with target normals: pcl::IterativeClosestPointWithNormals /
 *      TransformationEstimationPointToPlaneLLS (PCL 1.8.1, restated in DESIGN.md 2.9) ----
 * Per kept correspondence (d2 <= max_d2 and a finite normal n of target q), in float without fma:
 *   a = nz*sy - ny*sz, b = nx*sz - nz*sx, c = ny*sx - nx*sy, r = ((nx*qx + ny*qy) + nz*qz) - nx*sx - ny*sy - nz*sz,
 * widened to f64, v = (a, b, c, nx, ny, nz): ATA += v v^T, ATb += v r.  Sums record (f64, fixed summation order that depends
 * on the source count only):
 *   [0] kept count, [1..21] upper triangle of ATA row-major, [22..27] ATb, [28] sum d2 kept, [29] sum d2 all,
 *   [30] sum r^2 kept, [31] 0.
 * kss_p2l_sums[_dev]: the record for given correspondences (d2 recomputed as in kss_cov); idx entries outside [0, nt)
 * contribute nothing. */
#define KSS_P2L_NSUMS 32
int kss_p2l_sums(kss_ctx *ctx, const float *src, const float *tgt, const float *tgt_normals, const int32_t *idx,
                 int64_t n, int64_t nt, double max_d2, double sums[KSS_P2L_NSUMS]);
int kss_p2l_sums_dev(kss_ctx *ctx, const float *d_src, const float *d_tgt, const float *d_tgt_normals, const int32_t *d_idx,
                     int64_t n, int64_t nt, double max_d2, double sums[KSS_P2L_NSUMS]);
/* host-side: Cholesky solve of ATA x = ATb, x = (alpha, beta, gamma, tx, ty, tz), and PCL's constructTransformationMatrix
 * (R = Rz(gamma) Ry(beta) Rx(alpha)) rounded to float; row-major 4x4.  KSS_ERR_DEGENERATE (T = identity) when a pivot is
 * not finite or <= 1e-12 * max(diag ATA). */
int kss_rigid_from_p2l_sums(const double sums[KSS_P2L_NSUMS], float T[16]);
/* The ICP loop of kss_icp with the point-to-plane step: same NN, max_corr_dist, convergence criteria (MSE = point-to-point
 * d2 over kept correspondences), fitness and source update.  tgt_normals: nt*3 floats, or NULL to compute them with
 * kss_normals' definition (k = 20, flipped towards the origin) from the target.  A singular system ends the loop with
 * KSS_STATE_DEGENERATE (not converged, T as accumulated so far).  trace_sums receives trace_cap * KSS_P2L_NSUMS doubles.
 * p->allreduce must be NULL. */
int kss_icp_p2l(kss_ctx *ctx, const float *src, int64_t ns, const float *tgt, int64_t nt, const float *tgt_normals,
                const kss_icp_params *p, kss_icp_result *res);
int kss_icp_p2l_dev(kss_ctx *ctx, const float *d_src, int64_t ns, const float *d_tgt, int64_t nt, const float *d_tgt_normals,
                    const kss_icp_params *p, kss_icp_result *res);

/* ---- trimmed ICP for one partly overlapping pair (Chetverikov et al., TrICP), both metrics ----
 * One pass, with the exact NN target idx[i] and float d2[i] of every source as the NN pass writes them:
 *   candidates  0 <= d2[i] <= max_d2 (ordered compares in double: a NaN is none; -0.0f counts as +0.0f), m of them;
 *   rank        k = kss_trim_rank(m, overlap) = m == 0 ? 0 : max(1, (int64)ceil(overlap * (double)m)), one f64 multiplication;
 *   cut         tau = the k-th smallest candidate d2 (exact; m == 0: tau = 0 and nothing is kept);
 *   kept        the candidates with d2 <= tau -- ties at tau are all kept, so kept >= k; the plane metric also asks for a
 *               finite normal, as kss_icp_p2l does (the rank is taken on d2 alone);
 *   sums        over the kept set, f64, fixed order that depends on ns only: the KSS_NSUMS record ([17], [18], [19] = 0) solved
 *               by kss_rigid_from_sums (point metric), or the KSS_P2L_NSUMS record solved by kss_rigid_from_p2l_sums (plane).
 * The loop around it is kss_icp_p2l's: PCL's criteria on MSE = sum d2 kept / kept, fewer than min_correspondences kept ->
 * KSS_STATE_NO_CORRESPONDENCES, a singular plane system -> KSS_STATE_DEGENERATE, fitness over ALL sources.  overlap = 1 keeps
 * every candidate: with the plane metric that is kss_icp_p2l bit for bit.  overlap outside (0, 1] is KSS_ERR_ARG.  The step is rigid:
 * kss_icp_sim below is this loop on the point metric with the scale in the solve. */
enum { KSS_METRIC_POINT = 0, KSS_METRIC_PLANE = 1 };
#define KSS_TRIM_NINFO 4   /* {m candidates, k rank, tau widened to double, kept} */
/* host only, no context */
int kss_trim_rank(int64_t m, double overlap, int64_t *k);
/* the selection alone, for n squared distances: info[3] = the number of candidates <= tau */
int kss_trim_threshold(kss_ctx *ctx, const float *d2, int64_t n, double max_d2, double overlap, double info[KSS_TRIM_NINFO]);
int kss_trim_threshold_dev(kss_ctx *ctx, const float *d_d2, int64_t n, double max_d2, double overlap, double info[KSS_TRIM_NINFO]);
typedef struct {
    double  overlap;      /* share of the candidates kept per pass, 0 < overlap <= 1 */
    int     metric;       /* KSS_METRIC_POINT or KSS_METRIC_PLANE */
    double *trace_trim;   /* p->trace_cap * KSS_TRIM_NINFO doubles, row i beside trace_sums row i; may be NULL */
} kss_trim_params;
/* tgt_normals: plane metric: nt*3 floats or NULL (computed as in kss_icp_p2l); point metric: must be NULL.
 * p->trace_sums rows hold KSS_NSUMS (point) or KSS_P2L_NSUMS (plane) doubles.  In trace_trim and last_info (may be NULL: the
 * last pass's record) [3] is the number of correspondences the step was computed from.  p->allreduce must be NULL. */
int kss_icp_trimmed(kss_ctx *ctx, const float *src, int64_t ns, const float *tgt, int64_t nt, const float *tgt_normals,
                    const kss_icp_params *p, const kss_trim_params *tp, kss_icp_result *res, double last_info[KSS_TRIM_NINFO]);
int kss_icp_trimmed_dev(kss_ctx *ctx, const float *d_src, int64_t ns, const float *d_tgt, int64_t nt, const float *d_tgt_normals,
                        const kss_icp_params *p, const kss_trim_params *tp, kss_icp_result *res, double last_info[KSS_TRIM_NINFO]);

/* ---- similarity ICP for one pair: the scale refined with the motion (Umeyama's scale in the solve, PCL's
 *      TransformationEstimationSVDScale; bounded as in Du et al., scaling ICP), point metric with per-pass trimming ----
 * One pass, with the NN pass's idx[i] and float d2[i], the source's current float position p and its float target point q:
 *   candidates, rank, cut, kept   kss_icp_trimmed's point metric, not redefined: 0 <= d2 <= max_d2 in ordered double compares, m of
 *               them, k = kss_trim_rank(m, overlap), tau the exact k-th smallest candidate d2, kept d2 <= tau with the ties at tau.
 *   sums        KSS_NSUMS doubles in kss_icp_trimmed's fixed order (a function of ns alone): [0..16] kss_icp_trimmed's point record
 *               bit for bit; [17] = sum over the kept set of (px*px + py*py) + pz*pz, f64 on the widened floats, nothing fused;
 *               [18] = [19] = 0.
 *   step        kss_sim_from_sums(sums, lo, hi, T, &s_k), host only, no context:
 *               n, mu_s, mu_d, sigma, the SVD, sgn, R: kss_rigid_from_sums' own expressions, so R has the same bits.  The singular
 *               values sv0 >= sv1 >= sv2 come in descending order; sv2, the smallest, is the one sgn flips.
 *               var = sums[17]/n - ((mu_s0*mu_s0 + mu_s1*mu_s1) + mu_s2*mu_s2);  s = ((sv0 + sv1) + sgn*sv2) / var;
 *               s_k = min(max(s, lo), hi): for the R found the error is a quadratic in s, so the clamped value is the optimum
 *               inside [lo, hi];
 *               T_ij = (float)(s_k*R_ij), t_i = (float)(mu_d[i] - s_k*((R_i0*mu_s0 + R_i1*mu_s1) + R_i2*mu_s2)), last row 0 0 0 1.
 *               !(var > 0), or s not finite or not > 0: KSS_ERR_DEGENERATE, T the identity, s_k = 1 (a spread of the kept sources
 *               below the rounding of var is outside this definition).  With s_k == 1.0, T is kss_rigid_from_sums' T bit for bit.
 *               KSS_ERR_ARG: a NULL argument, or anything but 0 < lo <= hi.
 *   info        {m, k, tau, kept, s_k, s_acc after the pass}; s_k = 0 where the pass made no step.
 * The loop is kss_icp_trimmed's with the accumulated scale s_acc, 1 at the start: per pass lo = scale_min / s_acc and hi = scale_max /
 * s_acc, after the step s_acc = min(max(s_acc*s_k, scale_min), scale_max); final = T_k * final and the next NN pass applies T_k on
 * load, as everywhere.  MSE = [16] / [0].  PCL's criteria are read on C_k = [ (float)R | t ], the step without its scale, and
 * KSS_STATE_TRANSFORM asks in addition for (s_k - 1)*(s_k - 1) <= transformation_epsilon.  Fewer than min_correspondences kept ->
 * KSS_STATE_NO_CORRESPONDENCES, a degenerate step -> KSS_STATE_DEGENERATE (T as accumulated so far), fitness over ALL sources under
 * the final T.  The scale is bounded because the one-sided NN objective has the collapsed cloud -- every source on one target point
 * -- as a minimum.  res->T holds the accumulated similarity, which kss_transform_apply applies as it is; its scale is info[5].
 * scale_min == scale_max == 1 is kss_icp_trimmed with KSS_METRIC_POINT at the same overlap bit for bit: T, iterations, state,
 * last_mse, every trace_Tk and slots [0..16] of every trace_sums row.
 * Not offered: the similarity step on the plane, generalized and symmetric metrics; robust weights on it; kss_register and
 * kss_register_batch using it (their composite (R, t, s) assumes a rigid T_icp); the C++ mirror classes and the CLI. */
#define KSS_SIM_NINFO 6   /* {m, k, tau, kept, s_k, s_acc after the pass} */
typedef struct {
    double  overlap;                /* share of the candidates kept per pass, 0 < overlap <= 1 */
    double  scale_min, scale_max;   /* bounds of the accumulated scale, 0 < scale_min <= 1 <= scale_max < inf */
    double *trace_sim;              /* p->trace_cap * KSS_SIM_NINFO doubles, row i beside trace_sums row i; may be NULL */
} kss_sim_params;
/* overlap 1, scale_min 0.5, scale_max 2, trace_sim NULL */
int kss_sim_default_params(kss_sim_params *sp);
int kss_sim_from_sums(const double sums[KSS_NSUMS], double lo, double hi, float T[16], double *s_k);
/* The untrimmed record for given correspondences: packed float triples, d2 recomputed as in kss_cov, kept when 0 <= d2 <= max_d2;
 * an idx entry outside [0, nt) is no candidate (both forms take it). */
int kss_sim_sums(kss_ctx *ctx, const float *src, const float *tgt, const int32_t *idx, int64_t n, int64_t nt, double max_d2,
                 double sums[KSS_NSUMS]);
int kss_sim_sums_dev(kss_ctx *ctx, const float *d_src, const float *d_tgt, const int32_t *d_idx, int64_t n, int64_t nt, double max_d2,
                     double sums[KSS_NSUMS]);
/* last_info (may be NULL): the last pass's info record, all zero when no pass ran.  p->trace_sums rows hold KSS_NSUMS doubles.
 * KSS_ERR_ARG: a NULL ctx (refused before anything touches the device), sp, res or cloud; an overlap outside (0, 1]; anything but
 * 0 < scale_min <= 1 <= scale_max < inf; a set p->allreduce; an empty cloud.  A refused call leaves the context usable. */
int kss_icp_sim(kss_ctx *ctx, const float *src, int64_t ns, const float *tgt, int64_t nt, const kss_icp_params *p,
                const kss_sim_params *sp, kss_icp_result *res, double last_info[KSS_SIM_NINFO]);
int kss_icp_sim_dev(kss_ctx *ctx, const float *d_src, int64_t ns, const float *d_tgt, int64_t nt, const kss_icp_params *p,
                    const kss_sim_params *sp, kss_icp_result *res, double last_info[KSS_SIM_NINFO]);
/* Similarity ICP for MANY pairs per call.  Arguments as kss_icp_trimmed_batch without normals.  Nothing is redefined: every pair's
 * record -- T, iterations, state, converged, last_mse, its info, pair 0's traces -- is the single-pair call's BIT FOR BIT (fitness: to
 * the rounding of the NN engine's own summation order), in any batch order and any split over calls, under every nn_mode;
 * results[i].pair_id = i.  Offsets whose first entry is not 0 address a sub-range of the packed arrays.  The pairs run in lockstep,
 * three launches per pass behind the NN pass whatever the pair count; a pair that ends leaves the others untouched; every pair has
 * its own accumulated scale.  overlaps: one per pair, or NULL for sp->overlap everywhere.  info_all: npairs * KSS_SIM_NINFO doubles,
 * every pair's last info record (may be NULL).  trace_*, sp->trace_sim and fitness_idx / fitness_d2 describe pair 0.  KSS_ERR_ARG:
 * everything kss_icp_sim refuses, NULL offsets or results, an overlaps entry outside (0, 1], an empty pair, npairs <= 0. */
int kss_icp_sim_batch(kss_ctx *ctx, const float *src_all, const int64_t *src_off, const float *tgt_all, const int64_t *tgt_off,
                      int npairs, const kss_icp_params *p, const kss_sim_params *sp, const double *overlaps, kss_icp_result *results,
                      double *info_all);
int kss_icp_sim_batch_dev(kss_ctx *ctx, const float *d_src_all, const int64_t *src_off, const float *d_tgt_all, const int64_t *tgt_off,
                          int npairs, const kss_icp_params *p, const kss_sim_params *sp, const double *overlaps,
                          kss_icp_result *results, double *info_all);

/* ---- robust ICP for one pair with gross outliers of unknown share (M-estimator weights, one iteratively re-weighted
 *      least-squares step per pass), both metrics ----
 * One pass, with the NN pass's idx[i] and float d2[i], the source's current float position p, its target point q and normal n.
 * Every operation is f64 +, -, *, / (and one sqrt in Huber), none fused:
 *   candidate   idx[i] in [0, nt) and 0 <= d2[i] <= max_d2 (ordered compares in double, as in trimmed ICP); the plane metric also
 *               asks for a finite nx, ny, nz.  m of them.
 *   residual    x (f64, squared): point metric x = (double)d2; plane metric x = rd*rd, rd = (double)r with the float r of
 *               kss_icp_p2l (the product of two widened floats is exact).
 *   key         (float) point metric d2, plane metric fabsf(r); a source that is no candidate has a NaN key.
 *   scale       fixed form (rp->scale > 0): c2 = scale*scale.  Automatic form (rp->scale == 0): k = kss_trim_rank(m, 0.5), med =
 *               the exact k-th smallest key, medx = (double)med (point) or (double)med*(double)med (plane),
 *               K = (tune*1.4826)*(tune*1.4826), c2 = K*medx, raised to min_scale*min_scale where it is below that; m == 0: c2 = 0.
 *               kss_robust_scale2 is this expression.
 *   weight      kss_robust_weight: L2: w = 1.  Otherwise, c2 == 0: w = (x == 0) ? 1 : 0.  Otherwise u2 = x / c2 and
 *               Huber x <= c2 ? 1 : sqrt(c2 / x);  Tukey x < c2 ? (1 - u2)*(1 - u2) : 0;  Cauchy 1 / (1 + u2).
 *   kept        a candidate whose w is finite and > 0, decided by compares that involve no division (L2: every candidate;
 *               c2 == 0: x == 0; Huber and Cauchy: x < inf, or x <= c2 for Huber; Tukey: x < c2; a NaN c2 keeps nothing): cnt of
 *               them.  The two readings differ only where c2 / x underflows to 0 or x / c2 overflows, which no float residual
 *               reaches once c2 >= 2^-768.
 *   sums        over the kept set, f64, in kss_icp_trimmed's fixed order (a function of ns alone).  Point metric, the KSS_NSUMS
 *               record with ws[k] = w*p[k]: [0] += w, [1+k] += ws[k], [4+k] += w*q[k], [7+3k+l] += ws[k]*q[l], [16] += w*d2,
 *               [17] = m, [18] = 0, [19] = cnt.  Plane metric, the KSS_P2L_NSUMS record with v of kss_icp_p2l and wv[p] = w*v[p]:
 *               [0] += w, upper triangle += wv[p]*v[q], [22+p] += wv[p]*rd, [28] += w*d2, [29] = m, [30] += (w*rd)*rd, [31] = cnt.
 *               [0] being the weight total, kss_rigid_from_sums / kss_rigid_from_p2l_sums solve these records as they are.
 *   info        {m, c2, [0], cnt}.
 * The loop around it is kss_icp_trimmed's: PCL's criteria on MSE = [16 or 28] / [0], cnt < min_correspondences ->
 * KSS_STATE_NO_CORRESPONDENCES, a singular plane system -> KSS_STATE_DEGENERATE, fitness over ALL sources.  KSS_LOSS_L2 is the
 * unweighted step: with the plane metric kss_icp_p2l's, with the point metric kss_icp_trimmed's at overlap 1, bit for bit in the
 * slots they share.  A residual that is NaN (a source that is not finite) is outside this definition. */
enum { KSS_LOSS_L2 = 0, KSS_LOSS_HUBER = 1, KSS_LOSS_TUKEY = 2, KSS_LOSS_CAUCHY = 3 };
#define KSS_ROBUST_NINFO 4            /* {m candidates, c2, sum of weights, cnt kept} */
typedef struct {
    int     loss, metric;             /* KSS_LOSS_*, KSS_METRIC_POINT / _PLANE */
    double  scale;                    /* > 0: fixed c;  0: per pass from the median (above) */
    double  tune;                     /* scale == 0: c = tune * 1.4826 * median residual; > 0 and finite */
    double  min_scale;                /* >= 0: floor of c in the automatic form */
    double *trace_robust;             /* p->trace_cap * KSS_ROBUST_NINFO, row i beside trace_sums row i; may be NULL */
} kss_robust_params;
/* scale 0, min_scale 0, trace_robust NULL, tune 1.345 (Huber) / 4.685 (Tukey) / 2.385 (Cauchy) / 1 (L2, unused) */
int kss_robust_default_params(int loss, int metric, kss_robust_params *rp);
/* host only, no context.  kss_robust_weight: x >= 0 or NaN, c2 >= 0 or NaN.  kss_robust_scale2: med_key >= 0 (-0.0f counts as
 * +0.0f; negative or NaN: KSS_ERR_ARG), the floor applied. */
int kss_robust_weight(int loss, double x, double c2, double *w);
int kss_robust_scale2(int metric, double tune, float med_key, double min_scale, double *c2);
/* The pass's record for given correspondences (d2 recomputed as in kss_cov), conventions of kss_p2l_sums: tgt_normals are nt*3
 * floats for the plane metric and NULL for the point metric; sums holds KSS_NSUMS or KSS_P2L_NSUMS doubles by metric.  An idx
 * entry outside [0, nt) is no candidate (both forms take it). */
int kss_robust_sums(kss_ctx *ctx, const float *src, const float *tgt, const float *tgt_normals, const int32_t *idx, int64_t n,
                    int64_t nt, double max_d2, const kss_robust_params *rp, double *sums, double info[KSS_ROBUST_NINFO]);
int kss_robust_sums_dev(kss_ctx *ctx, const float *d_src, const float *d_tgt, const float *d_tgt_normals, const int32_t *d_idx,
                        int64_t n, int64_t nt, double max_d2, const kss_robust_params *rp, double *sums,
                        double info[KSS_ROBUST_NINFO]);
/* tgt_normals: plane metric: nt*3 floats or NULL (computed as in kss_icp_p2l); point metric: must be NULL.  last_info (may be
 * NULL): the last pass's info record, all zero when no pass ran.  p->allreduce must be NULL.  KSS_ERR_ARG: a loss or metric
 * out of range, scale negative or not finite, scale == 0 with tune not positive or not finite, min_scale negative or NaN,
 * normals with the point metric. */
int kss_icp_robust(kss_ctx *ctx, const float *src, int64_t ns, const float *tgt, int64_t nt, const float *tgt_normals,
                   const kss_icp_params *p, const kss_robust_params *rp, kss_icp_result *res, double last_info[KSS_ROBUST_NINFO]);
int kss_icp_robust_dev(kss_ctx *ctx, const float *d_src, int64_t ns, const float *d_tgt, int64_t nt, const float *d_tgt_normals,
                       const kss_icp_params *p, const kss_robust_params *rp, kss_icp_result *res,
                       double last_info[KSS_ROBUST_NINFO]);

/* ---- the ICP steps above for MANY pairs per call ----
 * (kss_icp_p2l and kss_icp_trimmed here; robust ICP: kss_icp_robust_batch below.)
 * Arguments as kss_icp_batch: packed float[n][3] clouds and npairs + 1 HOST offsets in points; tgt_normals_all is laid out like
 * tgt_all (NULL: computed per target as kss_icp_p2l does; the point metric takes none).  Nothing is redefined: the definitions at
 * kss_icp_p2l and kss_icp_trimmed hold for every pair, and every pair's record is the single-pair call's BIT FOR BIT (fitness:
 * to the rounding of the NN engine's own summation order), in any batch order and any split over calls; results[i].pair_id = i.
 * The pairs run in lockstep, three launches per pass behind the NN pass whatever the pair count; a pair that ends -- converged,
 * KSS_STATE_NO_CORRESPONDENCES, KSS_STATE_DEGENERATE -- leaves the others untouched.  overlaps: one per pair, or NULL for
 * tp->overlap everywhere.  info_all: npairs * KSS_TRIM_NINFO doubles, every pair's last selection record (may be NULL).  trace_*,
 * tp->trace_trim and fitness_idx / fitness_d2 describe pair 0.  KSS_ERR_ARG: a set allreduce, an overlap outside (0, 1], normals
 * with the point metric, an empty pair. */
int kss_icp_p2l_batch(kss_ctx *ctx, const float *src_all, const int64_t *src_off, const float *tgt_all, const int64_t *tgt_off,
                      const float *tgt_normals_all, int npairs, const kss_icp_params *p, kss_icp_result *results);
int kss_icp_p2l_batch_dev(kss_ctx *ctx, const float *d_src_all, const int64_t *src_off, const float *d_tgt_all, const int64_t *tgt_off,
                          const float *d_tgt_normals_all, int npairs, const kss_icp_params *p, kss_icp_result *results);
int kss_icp_trimmed_batch(kss_ctx *ctx, const float *src_all, const int64_t *src_off, const float *tgt_all, const int64_t *tgt_off,
                          const float *tgt_normals_all, int npairs, const kss_icp_params *p, const kss_trim_params *tp,
                          const double *overlaps, kss_icp_result *results, double *info_all);
int kss_icp_trimmed_batch_dev(kss_ctx *ctx, const float *d_src_all, const int64_t *src_off, const float *d_tgt_all, const int64_t *tgt_off,
                              const float *d_tgt_normals_all, int npairs, const kss_icp_params *p, const kss_trim_params *tp,
                              const double *overlaps, kss_icp_result *results, double *info_all);
/* ---- robust ICP for MANY pairs per call ----
 * Arguments as kss_icp_trimmed_batch.  Nothing is redefined: the definition at kss_icp_robust holds for every pair, and every
 * pair's record -- T, iterations, state, converged, last_mse, the info record, pair 0's traces -- is the single-pair call's BIT FOR
 * BIT (fitness: to the rounding of the NN engine's own summation order), in any batch order and any split over calls, under every NN
 * engine and tuning knob.  rp gives the loss, the metric, tune and min_scale of the whole batch.  scales: one double per pair, or
 * NULL for rp->scale everywhere; per pair > 0 is a fixed scale and 0 the automatic one from the pair's own per-pass median, so a
 * batch may mix both.  info_all: npairs * KSS_ROBUST_NINFO doubles, every pair's last {m, c2, sum of weights, cnt}, all zero for a
 * pair that ran no pass (may be NULL).  The pairs run in lockstep; behind the NN pass a pass makes two launches when every pair has
 * a fixed scale, otherwise three (point metric) or four (plane metric), whatever the pair count.  A pair that ends -- converged,
 * KSS_STATE_NO_CORRESPONDENCES, KSS_STATE_DEGENERATE -- leaves the others untouched.  trace_*, rp->trace_robust and fitness_idx /
 * fitness_d2 describe pair 0.  KSS_ERR_ARG: a set allreduce, everything kss_icp_robust refuses in rp, a scales entry that is
 * negative or not finite, an automatic pair with a tune that is not positive and finite, normals with the point metric, an empty
 * pair, NULL results. */
int kss_icp_robust_batch(kss_ctx *ctx, const float *src_all, const int64_t *src_off, const float *tgt_all, const int64_t *tgt_off,
                         const float *tgt_normals_all, int npairs, const kss_icp_params *p, const kss_robust_params *rp,
                         const double *scales, kss_icp_result *results, double *info_all);
int kss_icp_robust_batch_dev(kss_ctx *ctx, const float *d_src_all, const int64_t *src_off, const float *d_tgt_all, const int64_t *tgt_off,
                             const float *d_tgt_normals_all, int npairs, const kss_icp_params *p, const kss_robust_params *rp,
                             const double *scales, kss_icp_result *results, double *info_all);
/* the selection alone for nseg segments [off[i], off[i + 1]) of d2_all in ONE launch: overlaps and info_all (nseg * KSS_TRIM_NINFO)
 * hold one entry per segment; every record equals kss_trim_threshold on that segment.  An empty segment is KSS_ERR_ARG. */
int kss_trim_threshold_batch(kss_ctx *ctx, const float *d2_all, const int64_t *off, int nseg, double max_d2,
                             const double *overlaps, double *info_all);
int kss_trim_threshold_batch_dev(kss_ctx *ctx, const float *d_d2_all, const int64_t *off, int nseg, double max_d2,
                                 const double *overlaps, double *info_all);

/* ---- one-to-one ICP: each target keeps its closest source (PCL's CorrespondenceRejectorOneToOne in front of kss_icp_trimmed's
 *      pass), both metrics, one pair and MANY pairs per call ----
 * One pass, on the NN pass's idx[i] and float d2[i], both by original source index, i counting from 0 within the pair:
 *   candidate   idx[i] in [0, nt) and 0 <= d2[i] <= max_d2 (ordered compares in double, as in kss_icp_trimmed: a NaN is none), m of them;
 *   key         key(i) = ((uint64)(bits(d2[i]) & 0x7fffffff) << 32) | (uint32)i: the masking makes -0.0f count as +0.0f;
 *   winner      of target j: the candidate with idx == j and the smallest key -- the smallest d2, ties going to the lowest original
 *               source index; u = the number of targets that have a winner;
 *   filtered    idx_f, d2_f: a winner keeps idx[i] and d2[i] bit for bit; a losing candidate gets idx_f = -1 and d2_f = the quiet NaN
 *               0x7fc00000; a source that is no candidate passes through unchanged;
 *   the pass    kss_icp_trimmed's pass on (idx_f, d2_f), nothing redefined: its candidates are the u survivors, k = kss_trim_rank(u,
 *               overlap), tau the exact k-th smallest, ties at tau kept, the KSS_NSUMS (point) or KSS_P2L_NSUMS (plane) record in the
 *               same fixed order (the plane record's [29] runs over the sources whose idx_f is in [0, nt)), the same solve;
 *   info        KSS_O2O_NINFO doubles {u, k, tau, kept, m}.
 * The loop is kss_icp_trimmed's own: PCL's criteria, KSS_STATE_NO_CORRESPONDENCES, KSS_STATE_DEGENERATE, normals given or computed,
 * p->allreduce must be NULL; fitness over ALL sources, fitness_idx / fitness_d2 the unfiltered NN.  Neither the overlap share nor a
 * residual scale has to be known: at overlap 1 the sources outside the overlap, which all choose the few targets at its rim, lose
 * their correspondences to the closest of them.
 * Where no two candidates share a target in any pass the call is kss_icp_trimmed at the same overlap and metric BIT FOR BIT: T,
 * iterations, state, last_mse, every traced T_k and sums row, and info [0..3].
 * Behind the NN pass a pass makes three launches -- table reset, claim, resolve -- and then the trimmed pass's own: six more for one
 * pair, three more for a batch, whatever the pair count.
 * Not offered: the rejection in front of the robust, generalized, symmetric and similarity forms; the C++ mirror classes and the
 * CLI.  Keeping only reciprocal correspondences is kss_icp_recip's, below. */
#define KSS_O2O_NINFO 5   /* {u survivors, k rank, tau widened to double, kept, m candidates before the rejection} */
/* The filter alone for n sources against nt targets: idx_out / d2_out receive idx_f / d2_f (either may be NULL, either may be its
 * input), info = {m, u}.  KSS_ERR_ARG: a NULL ctx (refused before anything touches the device), idx, d2 or info; n or nt <= 0 or
 * beyond the C-ABI's cloud size. */
int kss_o2o_filter(kss_ctx *ctx, const int32_t *idx, const float *d2, int64_t n, int64_t nt, double max_d2, int32_t *idx_out,
                   float *d2_out, double info[2]);
int kss_o2o_filter_dev(kss_ctx *ctx, const int32_t *d_idx, const float *d_d2, int64_t n, int64_t nt, double max_d2, int32_t *d_idx_out,
                       float *d_d2_out, double info[2]);
/* nseg segments [off[i], off[i + 1]) of idx_all / d2_all (nseg + 1 HOST offsets), segment i against nts[i] targets, in the same three
 * launches: every segment equals the single call on it.  The outputs are indexed like the inputs; info_all: nseg * 2 doubles.
 * An empty segment or an nts entry <= 0 is KSS_ERR_ARG. */
int kss_o2o_filter_batch(kss_ctx *ctx, const int32_t *idx_all, const float *d2_all, const int64_t *off, const int64_t *nts, int nseg,
                         double max_d2, int32_t *idx_out_all, float *d2_out_all, double *info_all);
int kss_o2o_filter_batch_dev(kss_ctx *ctx, const int32_t *d_idx_all, const float *d_d2_all, const int64_t *off, const int64_t *nts,
                             int nseg, double max_d2, int32_t *d_idx_out_all, float *d_d2_out_all, double *info_all);
typedef struct {
    double  overlap;     /* share of the survivors kept per pass, 0 < overlap <= 1 */
    int     metric;      /* KSS_METRIC_POINT or KSS_METRIC_PLANE */
    double *trace_o2o;   /* p->trace_cap * KSS_O2O_NINFO doubles, row i beside trace_sums row i; may be NULL */
} kss_o2o_params;
/* overlap 1, KSS_METRIC_POINT, trace_o2o NULL */
int kss_o2o_default_params(kss_o2o_params *op);
/* Arguments as kss_icp_trimmed; last_info (may be NULL): the last pass's record, all zero when no pass ran.  KSS_ERR_ARG: everything
 * kss_icp_trimmed refuses, a NULL op, a NULL ctx (refused before anything touches the device).  A refused call leaves the context
 * usable. */
int kss_icp_o2o(kss_ctx *ctx, const float *src, int64_t ns, const float *tgt, int64_t nt, const float *tgt_normals,
                const kss_icp_params *p, const kss_o2o_params *op, kss_icp_result *res, double last_info[KSS_O2O_NINFO]);
int kss_icp_o2o_dev(kss_ctx *ctx, const float *d_src, int64_t ns, const float *d_tgt, int64_t nt, const float *d_tgt_normals,
                    const kss_icp_params *p, const kss_o2o_params *op, kss_icp_result *res, double last_info[KSS_O2O_NINFO]);
/* One-to-one ICP for MANY pairs per call.  Arguments as kss_icp_trimmed_batch: overlaps one per pair, or NULL for op->overlap
 * everywhere; info_all: npairs * KSS_O2O_NINFO doubles, every pair's last record (may be NULL).  Nothing is redefined: every pair's
 * record -- T, iterations, state, converged, last_mse, its info, pair 0's traces -- is the single-pair call's BIT FOR BIT (fitness: to
 * the rounding of the NN engine's own summation order), in any batch order and any split over calls, under every nn_mode and tuning
 * knob; results[i].pair_id = i.  One claim table serves the whole batch; a pair that ends leaves the others untouched.  trace_*,
 * op->trace_o2o and fitness_idx / fitness_d2 describe pair 0.  KSS_ERR_ARG: everything kss_icp_trimmed_batch refuses, a NULL op, a
 * NULL ctx. */
int kss_icp_o2o_batch(kss_ctx *ctx, const float *src_all, const int64_t *src_off, const float *tgt_all, const int64_t *tgt_off,
                      const float *tgt_normals_all, int npairs, const kss_icp_params *p, const kss_o2o_params *op,
                      const double *overlaps, kss_icp_result *results, double *info_all);
int kss_icp_o2o_batch_dev(kss_ctx *ctx, const float *d_src_all, const int64_t *src_off, const float *d_tgt_all, const int64_t *tgt_off,
                          const float *d_tgt_normals_all, int npairs, const kss_icp_params *p, const kss_o2o_params *op,
                          const double *overlaps, kss_icp_result *results, double *info_all);

/* ---- reciprocal ICP: a correspondence is kept only where source and target are each other's nearest (PCL's
 *      setUseReciprocalCorrespondences(true) in front of kss_icp_trimmed's pass), both metrics, one pair and
 *      MANY pairs per call ----
 * One pass, on the NN pass's idx[i] and float d2[i] (by original source index), the sources' CURRENT float positions p_k -- the ones
 * the NN pass measured from and wrote out -- and the float targets q_j:
 *   candidate, key(i)   exactly kss_icp_o2o's: idx[i] in [0, nt) and 0 <= d2[i] <= max_d2 in ordered double compares, m of them;
 *               key(i) = ((uint64)(bits(d2[i]) & 0x7fffffff) << 32) | (uint32)i;
 *   winner      kss_icp_o2o's: of the candidates with idx == j the one with the smallest key wins target j, u winners;
 *   rkey(k, j)  ((uint64)(bits(dist2<nn_fma>(p_k, q_j)) & 0x7fffffff) << 32) | (uint32)k, for EVERY source k in [0, ns), candidate or
 *               not: dist2 is the NN engines' own float arithmetic ((dx*dx + dy*dy) + dz*dz, or with p->nn_fma
 *               fma(dx, dx, fma(dy, dy, dz*dz))), d = p_k - q_j, the source first as the engines call it.  A NaN distance masks to a
 *               key above every finite one: it beats nothing;
 *   mutual      a winner i of target j is mutual iff NO source k has rkey(k, j) < key(i).  This is an existence statement: which
 *               sources an implementation examines, and in what order, cannot change a bit of the result.  With the engines' exact
 *               NN, rkey(i, j) == key(i), and the condition reads "i is the nearest source of its nearest target, ties to the
 *               lowest source index"; r = the number of mutual winners;
 *   filtered    idx_f, d2_f: a mutual winner keeps idx[i] and d2[i] bit for bit; every other candidate gets idx_f = -1 and d2_f = the
 *               quiet NaN 0x7fc00000; a source that is no candidate passes through unchanged;
 *   the pass    kss_icp_trimmed's pass on (idx_f, d2_f), nothing redefined, exactly as kss_icp_o2o does it;
 *   info        KSS_RECIP_NINFO doubles {r, k, tau, kept, m, u}.
 * A source position that is not finite is outside the definition; it neither faults nor takes part in the reverse search.
 * The loop, the endings, the normals given or computed, the fitness over ALL sources with the unfiltered fitness_idx / fitness_d2, and
 * p->allreduce must be NULL are kss_icp_o2o's.  Neither a residual scale nor an overlap has to be known: a stray source that is alone
 * on its target -- which one-to-one keeps -- goes wherever that target has a nearer source.
 * Where every winner is mutual in every pass the call is kss_icp_o2o at the same overlap and metric BIT FOR BIT: T, iterations, state,
 * last_mse, every traced T_k and sums row, and info [0..4]; where the NN map is also injective it is kss_icp_trimmed bit for bit.
 * Behind the NN pass a pass makes five launches -- workspace reset, claim + cell count, scan, scatter, resolve + check -- and then the
 * trimmed pass's six.  Once per call the target's bounding box is taken (one launch, one synchronisation) for the cell grid the
 * moving sources are binned into.
 * Many pairs per call: kss_icp_recip_pairs below.
 * Not built: the check in front of the robust, generalized, symmetric and similarity forms, for one pair or a batch; the C++
 * mirror classes and the CLI. */
#define KSS_RECIP_NINFO 6   /* {r mutual winners, k rank, tau widened to double, kept, m candidates, u winners before the check} */
/* The filter alone on packed float triples: n sources src with the map idx / d2 against nt targets tgt; d2 is taken as given, so the
 * definition above holds for any d2 the caller passes; nn_fma != 0: the reverse distances by the fma form.  idx_out / d2_out receive
 * idx_f / d2_f (either may be NULL, either may be its input), info = {m, u, r}.  KSS_ERR_ARG: a NULL ctx (refused before anything
 * touches the device), src, tgt, idx, d2 or info; n or nt <= 0 or beyond the C-ABI's cloud size. */
int kss_recip_filter(kss_ctx *ctx, const float *src, int64_t n, const float *tgt, int64_t nt, const int32_t *idx, const float *d2,
                     double max_d2, int nn_fma, int32_t *idx_out, float *d2_out, double info[3]);
int kss_recip_filter_dev(kss_ctx *ctx, const float *d_src, int64_t n, const float *d_tgt, int64_t nt, const int32_t *d_idx,
                         const float *d_d2, double max_d2, int nn_fma, int32_t *d_idx_out, float *d_d2_out, double info[3]);
typedef struct {
    double  overlap;       /* share of the mutual winners kept per pass, 0 < overlap <= 1 */
    int     metric;        /* KSS_METRIC_POINT or KSS_METRIC_PLANE */
    double *trace_recip;   /* p->trace_cap * KSS_RECIP_NINFO doubles, row i beside trace_sums row i; may be NULL */
} kss_recip_params;
/* overlap 1, KSS_METRIC_POINT, trace_recip NULL */
int kss_recip_default_params(kss_recip_params *rp);
/* Arguments as kss_icp_o2o; last_info (may be NULL): the last pass's record, all zero when no pass ran.  KSS_ERR_ARG: everything
 * kss_icp_o2o refuses -- a NULL ctx (refused before anything touches the device), a NULL rp.  A refused call leaves the context
 * usable. */
int kss_icp_recip(kss_ctx *ctx, const float *src, int64_t ns, const float *tgt, int64_t nt, const float *tgt_normals,
                  const kss_icp_params *p, const kss_recip_params *rp, kss_icp_result *res, double last_info[KSS_RECIP_NINFO]);
int kss_icp_recip_dev(kss_ctx *ctx, const float *d_src, int64_t ns, const float *d_tgt, int64_t nt, const float *d_tgt_normals,
                      const kss_icp_params *p, const kss_recip_params *rp, kss_icp_result *res, double last_info[KSS_RECIP_NINFO]);
/* The filter alone for nseg segments in one call: sources [off[i], off[i + 1]) of src_all, idx_all and d2_all against targets
 * [tgt_off[i], tgt_off[i + 1]) of tgt_all; nseg + 1 HOST offsets each; idx counts inside the segment's own target.  Every segment
 * equals kss_recip_filter on it.  The outputs are indexed like the inputs (either may be NULL, either may be its input); info_all:
 * nseg * 3 doubles {m, u, r}.  KSS_ERR_ARG: a NULL ctx (refused before anything touches the device), src_all, off, tgt_all, tgt_off,
 * idx_all, d2_all or info_all; nseg <= 0; an empty segment or a segment without targets; a segment or a total beyond the C-ABI's
 * cloud size. */
int kss_recip_filter_batch(kss_ctx *ctx, const float *src_all, const int64_t *off, const float *tgt_all, const int64_t *tgt_off, int nseg,
                           const int32_t *idx_all, const float *d2_all, double max_d2, int nn_fma, int32_t *idx_out_all,
                           float *d2_out_all, double *info_all);
int kss_recip_filter_batch_dev(kss_ctx *ctx, const float *d_src_all, const int64_t *off, const float *d_tgt_all, const int64_t *tgt_off,
                               int nseg, const int32_t *d_idx_all, const float *d_d2_all, double max_d2, int nn_fma,
                               int32_t *d_idx_out_all, float *d_d2_out_all, double *info_all);
/* Reciprocal ICP for MANY pairs per call.  The many-pairs form of every other family is spelled _batch; this one is
 * spelled _pairs because tests/test_recip_abi.py, written with the single pair, pins the _batch name as undeclared.  Arguments exactly
 * as kss_icp_o2o_batch, with kss_recip_params: overlaps one per pair, or NULL for rp->overlap everywhere; info_all: npairs *
 * KSS_RECIP_NINFO doubles, every pair's last record, all zero for a pair that ran no pass (may be NULL).  Nothing is redefined: the
 * definition above holds for every pair with i and k counting from 0 inside the pair, and every pair's record -- T, iterations, state,
 * converged, last_mse, its info, pair 0's traces -- is the single-pair call's bit for bit (fitness: to the rounding of the NN
 * engine's own summation order), in any batch order and any split over calls, through offsets that do not start at 0, under every
 * nn_mode and tuning knob and either nn_fma; results[i].pair_id = i.  Every pair has its own cell grid over its own target's box; a
 * pair that ends leaves the others untouched.  Behind the NN pass a pass makes the workspace reset and four launches for the whole
 * batch and then the trimmed batch's three, whatever the pair count; the boxes are taken once per call (one launch, one
 * synchronisation).  trace_*, rp->trace_recip and fitness_idx / fitness_d2 describe pair 0.  KSS_ERR_ARG: everything
 * kss_icp_o2o_batch refuses, a NULL rp, a NULL ctx (refused before anything touches the device).  A refused call leaves the context
 * usable. */
int kss_icp_recip_pairs(kss_ctx *ctx, const float *src_all, const int64_t *src_off, const float *tgt_all, const int64_t *tgt_off,
                        const float *tgt_normals_all, int npairs, const kss_icp_params *p, const kss_recip_params *rp,
                        const double *overlaps, kss_icp_result *results, double *info_all);
int kss_icp_recip_pairs_dev(kss_ctx *ctx, const float *d_src_all, const int64_t *src_off, const float *d_tgt_all, const int64_t *tgt_off,
                            const float *d_tgt_normals_all, int npairs, const kss_icp_params *p, const kss_recip_params *rp,
                            const double *overlaps, kss_icp_result *results, double *info_all);

/* ---- generalized ICP (plane-to-plane; Segal, Haehnel, Thrun: Generalized-ICP, RSS 2009) for one pair ----
 * Both clouds carry a local surface model: PCL-style GICP replaces the eigenvalues of each point's k-NN covariance by
 * (epsilon, 1, 1), which is I - (1 - epsilon) n n^T with n the smallest eigenvector -- the normal kss_normals computes.  So the
 * inputs are the NORMALS of both clouds (nt*3 and ns*3 floats); their signs do not matter, only n n^T enters.
 * One pass.  F is the float 4x4 accumulated so far (identity in pass 0; it maps the original source onto its current positions),
 * R_F its upper left 3x3.  For source i: its current float position p, the exact NN target j = idx[i] with float d2[i], the
 * float target point q, the float target normal nq = tgt_normals[j] and the float source normal ns = src_normals[i] (by ORIGINAL
 * index).  Everything below is f64 on the widened floats with +, -, *, / only, nothing fused, in exactly this order:
 *   candidate   j in [0, nt), !(d2 > max_d2) as in kss_icp_p2l, and all six normal components finite;
 *   m           m[k] = (R_F[k][0]*ns[0] + R_F[k][1]*ns[1]) + R_F[k][2]*ns[2], k = 0, 1, 2;
 *   C           e = 1 - epsilon;  g(a,b) = nq[a]*nq[b] + m[a]*m[b];  c_aa = 2 - e*g(a,a);  c_ab = -(e*g(a,b)) for a < b
 *               (C = 2I - (1 - epsilon)(nq nq^T + m m^T), six entries c00 c01 c02 c11 c12 c22);
 *   M           M = adj(C) / det(C) by cofactors:
 *               a00 = c11*c22 - c12*c12,  a01 = c02*c12 - c01*c22,  a02 = c01*c12 - c02*c11,
 *               a11 = c00*c22 - c02*c02,  a12 = c01*c02 - c00*c12,  a22 = c00*c11 - c01*c01,
 *               det = (c00*a00 + c01*a01) + c02*a02,  M_ab = a_ab / det (six divisions);
 *   dropped     a candidate whose det is not finite or not > 0.  Unit normals always give det >= 8*epsilon*(...) > 0; normals
 *               that are not of unit length are the caller's responsibility;
 *   d, u        d = q - p;  u = M d, u[a] = (M_a0*d[0] + M_a1*d[1]) + M_a2*d[2];
 *   A           A = [ -[p]x | I3 ], 3 x 6, x = (alpha, beta, gamma, tx, ty, tz) (with M = nq nq^T this is kss_icp_p2l's v and r).
 *               A^T M A by blocks, [p]x = (0 -pz py; pz 0 -px; -py px 0):
 *               B = [p]x M (upper right):   B_0b = py*M_2b - pz*M_1b,  B_1b = pz*M_0b - px*M_2b,  B_2b = px*M_1b - py*M_0b;
 *               B [p]x^T (upper left):      UL_a0 = B_a2*py - B_a1*pz,  UL_a1 = B_a0*pz - B_a2*px,  UL_a2 = B_a1*px - B_a0*py;
 *               lower right: M.   A^T M d = ( py*u[2] - pz*u[1],  pz*u[0] - px*u[2],  px*u[1] - py*u[0],  u[0], u[1], u[2] );
 *   record      KSS_P2L_NSUMS doubles: [0] kept count, [1..21] upper triangle of sum A^T M A row-major (UL00 UL01 UL02 B00 B01
 *               B02 | UL11 UL12 B10 B11 B12 | UL22 B20 B21 B22 | M00 M01 M02 | M11 M12 | M22), [22..27] sum A^T M d, [28] sum d2
 *               kept, [29] sum d2 over all sources with a valid j, [30] sum d^T M d = (d[0]*u[0] + d[1]*u[1]) + d[2]*u[2], [31] 0;
 *   order       the fixed summation order of kss_icp_p2l, a function of the source count alone;
 *   step        kss_rigid_from_p2l_sums on the record as it is: ONE Gauss-Newton step per pass (Cholesky, R = Rz Ry Rx).
 * The loop around it is kss_icp_p2l's: fewer than min_correspondences kept -> KSS_STATE_NO_CORRESPONDENCES, a failed Cholesky ->
 * KSS_STATE_DEGENERATE, PCL's criteria on MSE = [28] / [0], fitness over ALL sources, p->allreduce must be NULL.
 * 0 < epsilon <= 1, anything else is KSS_ERR_ARG; epsilon = 1 gives M = I/2, the point-to-point metric.  Accuracy: det(C) falls
 * with epsilon and the f64 cofactor inverse loses what C's condition (about 2 / epsilon) costs -- its error against an exact
 * inverse is about 1e-14 relative at epsilon = 1e-3 and reaches 5e-11 at epsilon = 1e-6; the result stays deterministic, but
 * epsilon well below 1e-3 buys nothing.  Many pairs per call: kss_icp_gicp_batch below.  Robust or trimmed weights on top, the
 * C++ mirror classes and the CLI do not have this metric. */
typedef struct {
    double epsilon;     /* 1e-3 */
    int    normals_k;   /* 20: read only when a set of normals is NULL; 3..64 */
} kss_gicp_params;
int kss_gicp_default_params(kss_gicp_params *gp);
/* host only, no context: M[6] = upper triangle (M00 M01 M02 M11 M12 M22) of (2I - (1-eps)(nq nq^T + m m^T))^-1 by the definition
 * above, nq widened to f64; *ok = 0 (M all zero) when dropped or a component is not finite, else 1. */
int kss_gicp_metric(const float nq[3], const double m[3], double epsilon, double M[6], int *ok);
/* The record for given correspondences (d2 recomputed as in kss_cov; the _dev form takes idx entries outside [0, nt) as no
 * correspondence, the host form refuses them).  Rn: HOST pointer to the row-major 3x3 float applied to the source normals in
 * place of R_F, NULL = identity.  src_normals / tgt_normals: n*3 / nt*3 floats, each may be NULL: then computed with kss_normals'
 * definition at k = min(normals_k, points) from the cloud as it is passed in, and rounded to float. */
int kss_gicp_sums(kss_ctx *ctx, const float *src, const float *src_normals, const float *tgt, const float *tgt_normals,
                  const int32_t *idx, int64_t n, int64_t nt, double max_d2, const float Rn[9], const kss_gicp_params *gp,
                  double sums[KSS_P2L_NSUMS]);
int kss_gicp_sums_dev(kss_ctx *ctx, const float *d_src, const float *d_src_normals, const float *d_tgt, const float *d_tgt_normals,
                      const int32_t *d_idx, int64_t n, int64_t nt, double max_d2, const float Rn[9], const kss_gicp_params *gp,
                      double sums[KSS_P2L_NSUMS]);
/* normals as in kss_gicp_sums (NULL: computed from the cloud as passed in, the source before any motion).  trace_sums receives
 * trace_cap * KSS_P2L_NSUMS doubles.  The result is that of kss_icp_p2l. */
int kss_icp_gicp(kss_ctx *ctx, const float *src, int64_t ns, const float *src_normals, const float *tgt, int64_t nt,
                 const float *tgt_normals, const kss_icp_params *p, const kss_gicp_params *gp, kss_icp_result *res);
int kss_icp_gicp_dev(kss_ctx *ctx, const float *d_src, int64_t ns, const float *d_src_normals, const float *d_tgt, int64_t nt,
                     const float *d_tgt_normals, const kss_icp_params *p, const kss_gicp_params *gp, kss_icp_result *res);

/* ---- generalized ICP for MANY pairs per call ----
 * Arguments as kss_icp_p2l_batch: packed float[n][3] clouds and npairs + 1 HOST offsets in points (the _dev form takes device clouds
 * and normals; the offsets stay host arrays).  src_normals_all is laid out like src_all, tgt_normals_all like tgt_all; either may
 * be NULL: then each cloud's normals are computed as kss_icp_gicp computes them, per pair, at gp->normals_k from the cloud as
 * passed in.  epsilons: one double per pair, or NULL for gp->epsilon everywhere.  Nothing is redefined: the definition at
 * kss_icp_gicp holds for every pair -- the rotation R_F applied to the source normals is the PAIR's own, pass by pass -- and every
 * pair's record -- T, iterations, state, converged, last_mse, pair 0's trace_* -- is the single-pair call's BIT FOR BIT (fitness: to
 * the rounding of the NN engine's own summation order), in any batch order and any split over calls, under every NN engine and
 * tuning knob; results[i].pair_id = i.  Offsets whose first entry is not 0 address a sub-range of the packed arrays.  The pairs
 * run in lockstep, one small table copy and two launches per pass behind the NN pass whatever the pair count; a pair that ends --
 * converged, KSS_STATE_NO_CORRESPONDENCES, KSS_STATE_DEGENERATE -- leaves the others untouched.  trace_* and fitness_idx /
 * fitness_d2 describe pair 0.  KSS_ERR_ARG: NULL ctx (refused before anything touches the device), offsets, gp or results;
 * npairs <= 0; an empty pair; a set allreduce; gp->epsilon or an epsilons entry outside (0, 1] or NaN; normals_k outside 3..64
 * where a set of normals has to be computed; everything kss_icp_p2l_batch refuses. */
int kss_icp_gicp_batch(kss_ctx *ctx, const float *src_all, const int64_t *src_off, const float *src_normals_all,
                       const float *tgt_all, const int64_t *tgt_off, const float *tgt_normals_all, int npairs,
                       const kss_icp_params *p, const kss_gicp_params *gp, const double *epsilons, kss_icp_result *results);
int kss_icp_gicp_batch_dev(kss_ctx *ctx, const float *d_src_all, const int64_t *src_off, const float *d_src_normals_all,
                           const float *d_tgt_all, const int64_t *tgt_off, const float *d_tgt_normals_all, int npairs,
                           const kss_icp_params *p, const kss_gicp_params *gp, const double *epsilons, kss_icp_result *results);

/* ---- voxelized generalized ICP against a reusable voxel map (Koide, Yokozuka, Oishi, Banno: Voxelized GICP, ICRA 2021;
 *      DESIGN.md 2.30), one pair ----
 * The target is summarised ONCE as one Gaussian per occupied voxel -- the mean of the voxel's points and the average n n^T of
 * their normals -- and a scan is registered against that summary: no nearest-neighbour search, a pass whose cost does not depend
 * on the target's size, and a map that serves as many scans and start poses as the caller likes.
 *
 * The map (kss_vmap).  It belongs to the context it was created on and owns its device memory apart from the context's grow-only
 * workspace: any other call on the context, one that grows the workspace included, leaves it intact.  It keeps the dense cell ->
 * voxel table (4 bytes per cell) and the packed voxel records, not the target's points or normals.
 *   normals     tgt_normals NULL: computed as in kss_gicp_sums (kss_normals' definition at k = min(normals_k, nt), rounded to float);
 *   mapped      a target is mapped if all three coordinates and all three normal components are finite; the others are not in the map;
 *   origin      lo_a = the float minimum of the mapped targets on axis a, a zero minimum taken as +0;
 *   cell        inv = 1.0f / (float)leaf;  f_a = floorf((x_a - lo_a) * inv), a float subtraction then a float multiplication, nothing
 *               fused;  dims_a = 1 + max f_a over the mapped targets;  lin = (c_z * dims_y + c_y) * dims_x + c_x in int64;
 *   record      over the voxel's mapped targets IN ASCENDING ORIGINAL INDEX, serially in f64, nothing fused: N = their count,
 *               s_a += (double)q_a, P_ab += (double)n_a * (double)n_b for the six a <= b; mean_a = s_a / (double)N, S_ab = P_ab /
 *               (double)N.  The order is part of the definition: every bit of the record follows from the cloud alone.
 * KSS_ERR_ARG: a NULL argument; nt <= 0; leaf not finite or not > 0; normals_k outside 3..64 where the normals are computed; no
 * mapped target; a max f_a that is not finite (an inv of infinity) or dims_x * dims_y * dims_z > 2^26.
 * kss_ctx_destroy frees the maps of the context that are still alive; their handles are dead with it.  kss_vmap_destroy waits for
 * the context's stream first.  An entry point takes a handle only if it is a live map of the context it is called on: NULL, a
 * destroyed map and a map of another context are KSS_ERR_ARG (kss_vmap_info has no context to ask: it trusts its handle). */
typedef struct kss_vmap kss_vmap;
typedef struct {
    double leaf;        /* the voxel edge; no default: kss_vmap_default_params sets 0 and the caller must set it */
    int    normals_k;   /* 20: read only when tgt_normals is NULL; 3..64 */
} kss_vmap_params;
int kss_vmap_default_params(kss_vmap_params *vp);
int kss_vmap_create(kss_ctx *ctx, const float *tgt, int64_t nt, const float *tgt_normals, const kss_vmap_params *vp, kss_vmap **out);
int kss_vmap_create_dev(kss_ctx *ctx, const float *d_tgt, int64_t nt, const float *d_tgt_normals, const kss_vmap_params *vp, kss_vmap **out);
int kss_vmap_destroy(kss_ctx *ctx, kss_vmap *map);
#define KSS_VMAP_NINFO 10   /* {mapped targets, voxels, dims x y z, leaf, origin x y z, inv widened} */
int kss_vmap_info(const kss_vmap *map, double info[KSS_VMAP_NINFO]);
#define KSS_VMAP_NSTAT 10   /* {N, mean x y z, S00 S01 S02 S11 S12 S22} */
/* The voxels in ascending lin: lin[v] and stats[v * KSS_VMAP_NSTAT ..] (either may be NULL), *nvox their count.  Both NULL: the count
 * alone.  KSS_ERR_CAPACITY (*nvox set) when capacity < *nvox. */
int kss_vmap_read(kss_ctx *ctx, const kss_vmap *map, int64_t *lin, double *stats, int64_t capacity, int64_t *nvox);

/* ---- a map that grows scan by scan, in a fixed box ----
 * Scan-to-map registration: register a scan against the map, insert it at the pose just found, take the next scan.  The map
 * keeps every voxel's N, s_a and P_ab in f64 beside the record (9 more doubles a voxel), so an insert CONTINUES the serial sums of
 * the definition above: kss_vmap_create(A) followed by an insert of B is, in every bit of kss_vmap_read and kss_vmap_info, the map
 * kss_vmap_create builds from A followed by the rows of B that are mapped and inside; and on a box map any split of a cloud
 * over calls, down to one point per call, gives the map of one call.  kss_vmap_create's own results do not change in any bit.
 *
 * kss_vmap_create_box: an EMPTY map (0 mapped targets, 0 voxels; kss_vmap_read returns 0 voxels and kss_icp_vgicp against it ends
 * in KSS_STATE_NO_CORRESPONDENCES) over the caller's box: lo_a = lo[a], a zero taken as +0;  inv = 1.0f / (float)leaf;
 * dims_a = 1 + floorf((hi_a - lo_a) * inv) in float, nothing fused.  vp->normals_k is not read.  KSS_ERR_ARG: a NULL argument; a
 * lo or hi that is not finite; hi_a < lo_a; a leaf kss_vmap_create refuses; an f that is not finite; more than 2^26 cells.
 *
 * kss_vmap_insert[_dev]: n points (packed float triples; the _dev form takes device pointers) into a live map of ctx, from
 * kss_vmap_create or kss_vmap_create_box.  The box, origin, inv and dims never change.
 *   normals     NULL: computed as kss_icp_vgicp computes a scan's normals, at normals_k (3..64), from pts as passed in, before
 *               the pose;
 *   pose        T: a HOST row-major float 4x4, or NULL: nothing is moved or turned.  Otherwise the position is
 *               p' = ((T00*x + T01*y) + T02*z) + T03 in float with no fma (transform_apply_f32's and the VGICP loop's move) and
 *               the normal is, in f64 on the widened floats, m_k = (R_k0*n0 + R_k1*n1) + R_k2*n2 (kss_icp_vgicp's m).  NULL: p' = p
 *               and m = (double)n.  An identity T gives the bits of NULL;
 *   mapped      p' and the three float normal components are finite;
 *   inside      0 <= f_a < dims_a on all three axes, f_a from p' by the map's expression, compared in float: the lookup's rule.
 *               Mapped points outside the box are counted in info[2] and change nothing;
 *   record      for the inserted points in ascending index of this call, after everything inserted earlier, serially in f64,
 *               nothing fused: N += 1, s_a += (double)p'_a, P_ab += m_a * m_b; then mean = s / N and S = P / N.
 * The voxels stay packed in ascending lin (an insert may renumber them); info[0] and info[1] of kss_vmap_info become the totals.
 * info (may be NULL): KSS_VMAP_NINSERT doubles.  A cloud with nothing to add -- every point non-finite or outside the box -- is
 * KSS_OK with the map unchanged.  KSS_ERR_ARG: a NULL ctx, map or pts; n <= 0; not a live map of ctx; normals_k outside 3..64
 * where the normals are computed; a T entry that is not finite.  A refused call or a failed allocation leaves the map exactly as
 * it was: every allocation precedes the first store into the map's table, and the new records are built beside the old ones and
 * take their place at the end.  An insert costs a pass over the dense cell table, whatever n is, and synchronises the context's
 * stream.
 * Not offered: eviction of points, a box that grows, a cap on the points a voxel takes.  A box that slides: kss_vmap_shift below. */
int kss_vmap_create_box(kss_ctx *ctx, const float lo[3], const float hi[3], const kss_vmap_params *vp, kss_vmap **out);
#define KSS_VMAP_NINSERT 4   /* {points added, points not mapped, points outside the box, voxels created by this call} */
int kss_vmap_insert(kss_ctx *ctx, kss_vmap *map, const float *pts, int64_t n, const float *normals,
                    const float T[16], int normals_k, double info[KSS_VMAP_NINSERT]);
int kss_vmap_insert_dev(kss_ctx *ctx, kss_vmap *map, const float *d_pts, int64_t n, const float *d_normals,
                        const float T[16], int normals_k, double info[KSS_VMAP_NINSERT]);

/* ---- a map whose box slides over its lattice ----
 * For a sensor that travels: the box keeps its size and moves by whole cells, so the table stays small and the map follows.
 * A map has a window base base_a, an integer number of cells per axis, 0 for every map from kss_vmap_create and
 * kss_vmap_create_box.  lo, inv, leaf and dims never change: lo is the ANCHOR of the lattice, the corner of the box only while
 * base = 0.  With a base, everywhere a map is looked up or inserted into (kss_vgicp_sums, kss_icp_vgicp, kss_icp_vgicp_batch,
 * kss_vmap_insert):
 *   cell        f_a = floorf((x_a - lo_a) * inv) as above, unchanged and not fused;
 *   inside      (float)base_a <= f_a < (float)(base_a + dims_a) on all three axes, compared in float; a NaN is outside;
 *   local cell  c_a = (int64)f_a - base_a, and lin = (c_z * dims_y + c_y) * dims_x + c_x from the local cells.
 * base = 0 gives the expressions above in every bit.  kss_vmap_info keeps its ten slots, the origin slots stay lo;
 * kss_vmap_read returns window-local lin; kss_vmap_window returns base (KSS_ERR_ARG: a NULL argument; like kss_vmap_info it
 * trusts its handle).
 *
 * kss_vmap_shift: base'_a = base_a + k_a.  A voxel of local cell c survives iff 0 <= c_a - k_a < dims_a on all three axes; its
 * new lin is lin - delta, delta = (k_z * dims_y + k_y) * dims_x + k_x, so the survivors stay packed in ascending lin in their
 * relative order, and each keeps its record and its f64 sums BIT FOR BIT.  A voxel that does not survive is gone: if its cell
 * comes back into the window later, the cell is empty.  info[0] of kss_vmap_info drops by the sum of the dropped voxels' N (an
 * integer sum, exact in any order).  k = (0, 0, 0): KSS_OK, nothing is launched, the map is untouched.  |k_a| >= dims_a on any
 * axis: the map becomes empty as kss_vmap_create_box leaves one.  info (may be NULL): KSS_VMAP_NSHIFT doubles.
 * KSS_ERR_ARG: a NULL ctx, map or k; not a live map of ctx; base'_a < -2^24 or base'_a + dims_a > 2^24 on any axis (beyond
 * that f is not an exact integer in float).  A refused call or a failed allocation leaves the map exactly as it was: every
 * allocation precedes the first store into the table.  A shift costs O(voxels) -- the table is touched at occupied cells alone
 * -- and synchronises the context's stream.
 *
 * kss_vmap_recentre: the shift that brings centre's cell to the middle of the window, decided on the host, then one
 * kss_vmap_shift.  f_a of centre by the map's expression;  want_a = (int64)f_a - dims_a / 2 (integer division);
 * k_a = want_a - base_a if |want_a - base_a| > slack, else 0.  k_out (may be NULL) receives k.  KSS_ERR_ARG: a NULL centre; a
 * centre that is not finite; slack < 0; an |f_a| above 2^24; everything kss_vmap_shift refuses.
 * Not offered: eviction by age, a cap on the points a voxel takes, a window that changes dims, a shift by a fraction of a cell,
 * remembering what left the window; the C++ mirror classes and the CLI do not have these entries. */
#define KSS_VMAP_NSHIFT 4   /* {voxels kept, voxels dropped, mapped points dropped, delta} */
int kss_vmap_window(const kss_vmap *map, int64_t base[3]);
int kss_vmap_shift(kss_ctx *ctx, kss_vmap *map, const int64_t k[3], double info[KSS_VMAP_NSHIFT]);
int kss_vmap_recentre(kss_ctx *ctx, kss_vmap *map, const float centre[3], int64_t slack, int64_t k_out[3],
                      double info[KSS_VMAP_NSHIFT]);

/* ---- a pyramid of maps: a live map coarsened, for registration coarse to fine ----
 * A map's basin is about a leaf wide.  A coarser level needs no point, no normal and no second insert: the map keeps every voxel's
 * f64 sums N, s_a, P_ab, and a coarse voxel is the ordered sum of its children's sums.
 *
 * kss_vmap_coarsen: a NEW map whose voxels are k x k x k blocks of map's, k in 2..8.
 *   header      lo' = lo (the same lattice anchor);  leaf' = (double)k * leaf;  inv' = 1.0f / (float)leaf';  base'_a =
 *               floor(base_a / k), rounded towards minus infinity (a shifted map can have a negative base);  dims'_a =
 *               (dims_a + k - 2) / k + 1 in integer division: a function of dims and k alone that covers the fine window at every
 *               base (one layer may stay empty) and never exceeds dims_a;
 *   parent      a fine voxel of local cell c has the lattice cell a = base + c; its parent's lattice cell is A_a = floor(a_a / k),
 *               its parent's local cell C = A - base', and lin' = (C_z * dims'_y + C_y) * dims'_x + C_x.  Membership is integer
 *               arithmetic on the fine cells: no point is looked up again;
 *   record      over the children in ascending fine lin -- ascending (a_z, a_y, a_x) --, serially in f64 from +0, nothing fused,
 *               from the children's KEPT SUMS (not their quotients): N' = sum N (exact), s'_a += s_a, P'_ab += P_ab; then mean' =
 *               s' / N' and S' = P' / N'.  A coarse voxel of one child has that child's sums and record bit for bit;
 *   totals      the mapped-targets total is map's; the voxels are packed in ascending lin'.
 * *out is an ordinary live map of ctx with its own table, records and sums: it holds no reference to map, which may be destroyed
 * first, and every entry takes it -- the lookup with its own inv', kss_vmap_insert continuing s' and P', kss_vmap_shift, read,
 * info, window, destroy.  inv' is rounded on its own, so a point next to a coarse cell face may be looked up in (or inserted
 * into) a NEIGHBOUR of its fine voxel's parent; where leaf and k are powers of two the two agree exactly.  A map without a voxel
 * coarsens to an empty map, as kss_vmap_create_box leaves one.  map is not changed in any bit.
 * Coarsening twice is not coarsening once: coarsen(coarsen(m, 2), 2) holds the voxels of coarsen(m, 4), but its sums were added in
 * another order and are not bit-equal.
 * KSS_ERR_ARG: a NULL argument; k outside 2..8; not a live map of ctx.  A failed allocation holds nothing.  The call synchronises
 * the context's stream once, where the voxel count comes back; the merge is launched behind it and not waited for (every call
 * that reads a map runs behind it on the context's stream).
 *
 * kss_vmap_coarsen_into: dst, a live map of ctx other than map, refreshed: afterwards it equals a fresh kss_vmap_coarsen(map, k)
 * in every bit of kss_vmap_read, kss_vmap_info and kss_vmap_window, whatever it held before -- inserts and shifts of its own
 * included.  Its lo, leaf, inv and dims must equal, bit for bit, what kss_vmap_coarsen(map, k) would give (its base need not):
 * otherwise KSS_ERR_ARG with both maps untouched.  It reuses dst's table, its records where they have room and its work area (a
 * coarse map keeps the flags and numbering of its fill, about twice its table): the call a scan-to-map loop makes after every
 * insert and recentre allocates nothing while the voxel count fits.  Every allocation precedes the first store into dst; a failed
 * allocation leaves dst as it was.  KSS_ERR_ARG also: everything kss_vmap_coarsen refuses; dst not a live map of ctx; dst == map.
 * Not offered: a coarse map that follows its source by itself, a pyramid object that refreshes itself; the C++ mirror classes and
 * the CLI do not have these entries. */
int kss_vmap_coarsen(kss_ctx *ctx, const kss_vmap *map, int k, kss_vmap **out);
int kss_vmap_coarsen_into(kss_ctx *ctx, const kss_vmap *map, int k, kss_vmap *dst);

/* One pass.  F and R_F as in kss_icp_gicp.  For source i: its current float position p and its float normal ns = src_normals[i]
 * (by ORIGINAL index).  Everything after the lookup is f64 on the widened floats, nothing fused, in kss_icp_gicp's order:
 *   voxel       f_a from p by the map's expression above; the source has a voxel iff 0 <= f_a < dims_a on all three axes --
 *               compared in float, so a NaN has none -- and the cell is occupied;
 *   candidate   it has a voxel, ns is finite, and !(dd > max_d2) with d = mean - p, dd = (d[0]*d[0] + d[1]*d[1]) + d[2]*d[2];
 *   metric      m, C, M, d, u, B, UL and the dropped rule are kss_icp_gicp's text with g(a,b) = S_ab + m[a]*m[b] and q = mean.  No
 *               count weight.  A voxel of ONE target has mean = q and S = nq nq^T exactly: the correspondence's terms are then
 *               kss_icp_gicp's bit for bit;
 *   record      kss_icp_gicp's KSS_P2L_NSUMS slots in kss_icp_p2l's fixed summation order, a function of n alone: [28] = sum of dd
 *               over the kept sources, [29] = 0, [30] = sum d^T M d, [31] = 0.
 * kss_vgicp_sums[_dev]: the record of one pass at the positions passed in.  Rn: HOST pointer to the row-major 3x3 float applied to
 * the source normals in place of R_F, NULL = identity.  src_normals NULL: computed as in kss_gicp_sums at gp->normals_k.
 * KSS_ERR_ARG: a NULL src, gp or sums; n <= 0; not a live map of ctx; epsilon outside (0, 1] or NaN; normals_k outside 3..64
 * where the normals are computed. */
int kss_vgicp_sums(kss_ctx *ctx, const float *src, const float *src_normals, int64_t n, const kss_vmap *map, double max_d2,
                   const float Rn[9], const kss_gicp_params *gp, double sums[KSS_P2L_NSUMS]);
int kss_vgicp_sums_dev(kss_ctx *ctx, const float *d_src, const float *d_src_normals, int64_t n, const kss_vmap *map, double max_d2,
                       const float Rn[9], const kss_gicp_params *gp, double sums[KSS_P2L_NSUMS]);
/* The loop is kss_icp_gicp's -- step kss_rigid_from_p2l_sums, fewer than min_correspondences kept -> KSS_STATE_NO_CORRESPONDENCES, a
 * failed Cholesky -> KSS_STATE_DEGENERATE, PCL's criteria on MSE = [28] / [0], trace_sums (trace_cap * KSS_P2L_NSUMS doubles) and
 * trace_Tk -- with NO nearest-neighbour pass in it: pass 0 works on the positions passed in, and behind every step T_k the sources
 * move by T_k in float as every pair loop moves them (pcl transformCloud: ((T00*x + T01*y) + T02*z) + T03, no fma).
 * res->fitness (p->compute_fitness): [28] / [0] of one more evaluation at F * the ORIGINAL source, F the final float 4x4 applied
 * the same way and R_F turning the normals: the mean squared distance to the voxel mean over the kept sources of that evaluation,
 * NaN when there is none.  This is NOT getFitnessScore: sources without a voxel do not count, and the distance is to a voxel's
 * mean, not to a nearest target point.
 * last_info (may be NULL): {kept in the last pass of the loop, ns, [30] of that pass, voxels of the map}.
 * p->nn_mode, p->nn_fma and the nn_* tuning fields are not read.  KSS_ERR_ARG: everything kss_vgicp_sums refuses, a NULL p or res,
 * a set p->allreduce, a set p->fitness_idx or p->fitness_d2 (there are no correspondences to return).  A count weight, robust or
 * trimmed weights, the C++ mirror classes and the CLI do not have this method.
 *
 * ---- the 7- and 27-voxel neighbourhoods ----
 * The text above is the map's neighbourhood setting 1, which every map starts at: kss_vmap_create[_dev], kss_vmap_create_box and
 * kss_vmap_coarsen (which does not inherit its source's setting).  kss_vmap_set_neighbourhood(map, nb) with nb one of
 * KSS_VMAP_NB_1, KSS_VMAP_NB_7, KSS_VMAP_NB_27 writes a host-side header field of the map: nothing is launched, and every later
 * call that looks the map up reads it -- kss_vgicp_sums[_dev], kss_icp_vgicp[_dev], kss_icp_vgicp_from[_dev],
 * kss_icp_vgicp_c2f[_dev] (per level, by that level's map) and kss_icp_vgicp_batch[_dev], the fitness evaluation included.
 * kss_vmap_insert, kss_vmap_shift and kss_vmap_recentre do not touch it; kss_vmap_coarsen_into leaves dst's as it is.
 * kss_vmap_neighbourhood reads it (KSS_ERR_ARG: a NULL argument; like kss_vmap_info it trusts its handle).
 * kss_vmap_set_neighbourhood: KSS_ERR_ARG for an nb that is not 1, 7 or 27, a NULL argument, or a handle that is not a live map of
 * ctx; a refused call leaves the setting unchanged.  At setting 1, set or never set, every entry gives the results it gave
 * before the setting existed, in every bit.  At 7 and 27 a source is matched against its own voxel AND the occupied voxels
 * around it, one correspondence each:
 *   lattice cell   f_a from the current float position by the map's expression, unchanged.  The source has a lattice cell iff
 *                  |f_a| <= 2^24 on all three axes -- compared in float, so a NaN has none; then a_a = (int)f_a.
 *   neighbours     offsets o with each component in {-1, 0, 1}: for 7 the centre and the six with exactly one non-zero
 *                  component, for 27 all of them; in the order: the centre first, then the others in ascending (o_z, o_y, o_x).
 *                  The neighbour cell is a + o in integer arithmetic; it is in the window iff base_a <= a_a + o_a < base_a + dims_a
 *                  on all axes (base: kss_vmap_window).  Each neighbour is tested on its own: a source whose own cell is outside
 *                  the window, or empty, still takes the neighbours that are inside and occupied.
 *   correspondence one per neighbour that is in the window and occupied, and the rest is the one-pass text above with that
 *                  voxel's record: ns finite (tested once per source), d = mean - p and !(dd > max_d2), m from R_F and the
 *                  original normal (once per source), C, M and the dropped rule from that voxel's S, the terms of the record.  No
 *                  count weight and no distance weight.
 *   record         the KSS_P2L_NSUMS slots summed over the correspondences: per lane the sources in the walk's order, per source
 *                  the neighbours in the order above, then the unchanged block and row reduction.  [0] is the number of kept
 *                  CORRESPONDENCES (not of distinct sources): min_correspondences and MSE = [28] / [0] use it as they are, and
 *                  last_info[0] remains [0].  [29] and [31] stay 0.
 *   identity       a source whose own voxel is occupied, and none of whose other neighbours is in the window and occupied, adds
 *                  the same terms in the same order as at setting 1.  So on a map of one voxel (dims 1 x 1 x 1) with every source
 *                  inside it, settings 7 and 27 give the record and the whole run of setting 1 in every bit.
 * Not offered: a count or a distance weight per neighbour; a per-call override of the map's setting; the number of distinct
 * sources kept (the record counts correspondences); the C++ mirror classes and the CLI. */
#define KSS_VMAP_NB_1  1
#define KSS_VMAP_NB_7  7
#define KSS_VMAP_NB_27 27
int kss_vmap_set_neighbourhood(kss_ctx *ctx, kss_vmap *map, int nb);
int kss_vmap_neighbourhood(const kss_vmap *map, int *nb);
#define KSS_VGICP_NINFO 4
int kss_icp_vgicp(kss_ctx *ctx, const float *src, int64_t ns, const float *src_normals, const kss_vmap *map, const kss_icp_params *p,
                  const kss_gicp_params *gp, kss_icp_result *res, double last_info[KSS_VGICP_NINFO]);
int kss_icp_vgicp_dev(kss_ctx *ctx, const float *d_src, int64_t ns, const float *d_src_normals, const kss_vmap *map,
                      const kss_icp_params *p, const kss_gicp_params *gp, kss_icp_result *res, double last_info[KSS_VGICP_NINFO]);

/* ---- voxelized generalized ICP from a start pose, and coarse to fine over several maps ----
 * kss_icp_vgicp_from[_dev]: kss_icp_vgicp with the accumulated F started at T0 instead of the identity.  T0: a HOST row-major
 * float 4x4 (as kss_vmap_insert's T), or NULL: kss_icp_vgicp bit for bit.  With T0, pass 0 works on T0 * src by the loop's float
 * move, ((T00*x + T01*y) + T02*z) + T03 with no fma; the source normals are turned by R_F in f64 from the ORIGINAL float normals,
 * as in every pass -- nothing is rounded to float on the way, which a caller who applies the pose to the scan beforehand cannot
 * avoid --; every step is composed as before, F = T_k * F, the float Matrix4f product.  res->T is the final F, start pose
 * included; the fitness is evaluated at F * the original source.  An identity T0 gives the result bits of NULL (finite clouds).
 * KSS_ERR_ARG: everything kss_icp_vgicp refuses; a T0 entry that is not finite.
 *
 * kss_icp_vgicp_c2f[_dev]: the ladder in one call.  maps[0 .. nlevels), nlevels in 1..KSS_VGICP_MAX_LEVELS: live maps of ctx in
 * the order they are to be used, the caller puts the coarsest first; any maps will do, they need not come from kss_vmap_coarsen.
 * Level l is the kss_icp_vgicp_from call on maps[l] from A_{l-1}, with A_{-1} = T0 (or NULL) and A_l = results[l].T.  results[l]
 * and last_info[l * KSS_VGICP_NINFO ..] (last_info may be NULL) are that call's BIT FOR BIT, with two departures: the fitness is
 * evaluated for the last level only (earlier levels as with compute_fitness = 0), and trace_* describe the last level.
 * results[l].pair_id = l.  A level that ends in KSS_STATE_NO_CORRESPONDENCES or KSS_STATE_DEGENERATE hands on the pose it
 * reached and the ladder goes on: the last record tells the caller how it ended.  The scan is staged once and NULL normals are
 * computed once: that is what the entry saves over a loop of calls.  The criteria of p hold for every level.
 * KSS_ERR_ARG: everything kss_icp_vgicp_from refuses; a NULL maps or results; nlevels outside 1..8; any level that is not a live
 * map of ctx -- all checked before anything is launched.
 * Not offered: the ladder or start poses for a batch of scans (kss_icp_vgicp_batch), criteria per level; the C++ mirror classes
 * and the CLI do not have these entries. */
#define KSS_VGICP_MAX_LEVELS 8
int kss_icp_vgicp_from(kss_ctx *ctx, const float *src, int64_t ns, const float *src_normals, const kss_vmap *map, const float T0[16],
                       const kss_icp_params *p, const kss_gicp_params *gp, kss_icp_result *res, double last_info[KSS_VGICP_NINFO]);
int kss_icp_vgicp_from_dev(kss_ctx *ctx, const float *d_src, int64_t ns, const float *d_src_normals, const kss_vmap *map,
                           const float T0[16], const kss_icp_params *p, const kss_gicp_params *gp, kss_icp_result *res,
                           double last_info[KSS_VGICP_NINFO]);
int kss_icp_vgicp_c2f(kss_ctx *ctx, const float *src, int64_t ns, const float *src_normals, const kss_vmap *const *maps, int nlevels,
                      const float T0[16], const kss_icp_params *p, const kss_gicp_params *gp, kss_icp_result *results,
                      double *last_info /* nlevels * KSS_VGICP_NINFO, may be NULL */);
int kss_icp_vgicp_c2f_dev(kss_ctx *ctx, const float *d_src, int64_t ns, const float *d_src_normals, const kss_vmap *const *maps,
                          int nlevels, const float T0[16], const kss_icp_params *p, const kss_gicp_params *gp,
                          kss_icp_result *results, double *last_info /* nlevels * KSS_VGICP_NINFO, may be NULL */);

/* ---- voxelized generalized ICP for MANY scans against ONE map per call ----
 * src_all and src_off as in kss_icp_gicp_batch: packed float[n][3] scans and nscans + 1 HOST offsets in points (the _dev form takes
 * device scans and normals; the offsets stay a host array); offsets whose first entry is not 0 address a sub-range of the packed
 * arrays.  src_normals_all is laid out like src_all; NULL: each scan's normals are computed as kss_icp_vgicp computes them, per
 * scan, at gp->normals_k from the scan as passed in.  epsilons: one double per scan, or NULL for gp->epsilon everywhere.
 * p->max_corr_dist and the convergence criteria hold for the whole call.  One map serves every scan and is not changed.
 * Nothing is redefined: scan i's record -- T, iterations, converged, state, last_mse, fitness and its KSS_VGICP_NINFO doubles
 * last_info[i * KSS_VGICP_NINFO ..] (last_info may be NULL) -- is the kss_icp_vgicp call on that scan BIT FOR BIT, in any batch
 * order and any split over calls; the fitness too, since it is [28] / [0] of one more evaluation of the same fixed-order record at
 * F_i * the original scan (NaN where nothing is kept).  trace_* describe scan 0; results[i].pair_id = i.  The scans run in
 * lockstep, one small table copy and two launches per pass whatever the scan count; a scan that ends -- converged,
 * KSS_STATE_NO_CORRESPONDENCES, KSS_STATE_DEGENERATE -- leaves the others untouched.  A start pose per scan is the caller's to
 * apply to the scan beforehand; a map per scan is not offered.
 * KSS_ERR_ARG: a NULL ctx (refused before anything touches the device), src_all, src_off, p, gp or results; nscans <= 0; an
 * empty scan or decreasing offsets; not a live map of ctx; gp->epsilon or an epsilons entry outside (0, 1] or NaN; normals_k
 * outside 3..64 where the normals are computed; a set p->allreduce, p->fitness_idx or p->fitness_d2; more partial rows than
 * kss_icp_p2l_batch takes (the sum over the scans of min(2048, ceil(ns_i / 256)) above 0x7fff0000). */
int kss_icp_vgicp_batch(kss_ctx *ctx, const float *src_all, const int64_t *src_off, const float *src_normals_all, int nscans,
                        const kss_vmap *map, const kss_icp_params *p, const kss_gicp_params *gp, const double *epsilons,
                        kss_icp_result *results, double *last_info /* nscans * KSS_VGICP_NINFO, may be NULL */);
int kss_icp_vgicp_batch_dev(kss_ctx *ctx, const float *d_src_all, const int64_t *src_off, const float *d_src_normals_all, int nscans,
                            const kss_vmap *map, const kss_icp_params *p, const kss_gicp_params *gp, const double *epsilons,
                            kss_icp_result *results, double *last_info /* nscans * KSS_VGICP_NINFO, may be NULL */);

/* ---- symmetric ICP (point-to-plane on the sum of both normals; Rusinkiewicz: A Symmetric Objective Function for ICP, SIGGRAPH
 * 2019; PCL's TransformationEstimationSymmetricPointToPlaneLLS) for one pair ----
 * The point-to-plane residual is taken against nq + ns and each cloud is turned by half the step towards the other: the residual
 * is zero for any pair on a common second-order patch, not only a common plane, so the basin of convergence is wider than
 * kss_icp_p2l's or kss_icp_gicp's at point-to-plane's cost per pass.  Both clouds carry normals (nt*3 and ns*3 floats).
 * One pass.  F is the float 4x4 accumulated so far (identity in pass 0), R_F its upper left 3x3.  For source i: its current float
 * position p, the exact NN target j = idx[i] with float d2[i], the float target point q, the float target normal
 * nq = tgt_normals[j] and the float source normal ns = src_normals[i] (by ORIGINAL index).  Everything below is f64 on the
 * widened floats with +, -, * only, nothing fused, in exactly this order:
 *   candidate   j in [0, nt), !(d2 > max_d2), and all six normal components finite (kss_icp_gicp's tests); slot [29] receives d2
 *               for every source with a valid j;
 *   m           m[k] = (R_F[k][0]*ns[0] + R_F[k][1]*ns[1]) + R_F[k][2]*ns[2], k = 0, 1, 2;
 *   n           dot = (m[0]*nq[0] + m[1]*nq[1]) + m[2]*nq[2];  align_normals = 1: n = nq - m if dot < 0, else n = nq + m;
 *               align_normals = 0: always n = nq + m (consistently oriented normals, e.g. from kss_normals_orient).  The residual
 *               is squared, so with align_normals = 1 the record does not depend on the sign of any input normal, bit for bit;
 *   w, d        w = p + q,  d = q - p, component by component;
 *   c           c = w x n:  c0 = w[1]*n[2] - w[2]*n[1],  c1 = w[2]*n[0] - w[0]*n[2],  c2 = w[0]*n[1] - w[1]*n[0];
 *   v, r        v = (c0, c1, c2, n[0], n[1], n[2]);  r = (d[0]*n[0] + d[1]*n[1]) + d[2]*n[2];
 *   record      KSS_P2L_NSUMS doubles: [0] kept count, [1..21] upper triangle of sum v v^T row-major, [22..27] sum v*r, [28] sum d2
 *               kept, [29] sum d2 over all sources with a valid j, [30] sum r*r, [31] 0;
 *   order       the fixed summation order of kss_icp_p2l, a function of the source count alone.
 * The system is uncentred, as kss_icp_p2l's is (a stated choice: the record, the solve and the final launch are reused as they
 * are; the clouds this library sees are pre-shaped to unit scale).
 * Step (kss_rigid_from_symm_sums, host): x = (a, t) = (a0, a1, a2, t0, t1, t2) by kss_rigid_from_p2l_sums' Cholesky solve of the
 * record; a failed Cholesky gives KSS_ERR_DEGENERATE / KSS_STATE_DEGENERATE and T the identity.  Then, in f64:
 *   s2 = (a0*a0 + a1*a1) + a2*a2;   c = 1 / sqrt(1 + s2);   k = (c*c) / (1 + c);
 *   H_ab = c*(delta_ab + K_ab) + k*(a_a*a_b),  K = (0 -a2 a1; a2 0 -a0; -a1 a0 0)   (the half rotation: Rodrigues with
 *          tan(theta) = |a|, exactly orthogonal in real arithmetic, no division by |a|, no libm call);
 *   R_ab = (H_a0*H_0b + H_a1*H_1b) + H_a2*H_2b;    t_a = (H_a0*(c*t0) + H_a1*(c*t1)) + H_a2*(c*t2);
 * the twelve entries rounded to float, last row 0 0 0 1: p -> H (H p + c t), the paper's R p + t ~ R^-1 q.
 * The loop around it is kss_icp_p2l's: fewer than min_correspondences kept -> KSS_STATE_NO_CORRESPONDENCES, PCL's criteria on
 * MSE = [28] / [0], fitness over ALL sources, p->allreduce must be NULL.  KSS_ERR_ARG: everything kss_icp_gicp refuses, and
 * align_normals outside {0, 1}.  Many pairs per call: kss_icp_symm_batch below.  Robust weights on top: kss_icp_symm_robust below
 * (a single pair).  Trimming, the C++ mirror classes and the CLI do not have this metric. */
typedef struct {
    int normals_k;      /* 20: read only when a set of normals is NULL; 3..64 */
    int align_normals;  /* 1: n = nq - m where m . nq < 0;  0: always n = nq + m */
} kss_symm_params;
int kss_symm_default_params(kss_symm_params *sp);
/* host only, no context: the step above from a record; KSS_ERR_DEGENERATE with T the identity when the Cholesky fails */
int kss_rigid_from_symm_sums(const double sums[KSS_P2L_NSUMS], float T[16]);
/* The record for given correspondences: the arguments of kss_gicp_sums (d2 recomputed as in kss_cov; the _dev form takes idx
 * entries outside [0, nt) as no correspondence, the host form refuses them; Rn: HOST pointer to the row-major 3x3 float applied
 * to the source normals in place of R_F, NULL = identity; either set of normals may be NULL: computed as for kss_gicp_sums). */
int kss_symm_sums(kss_ctx *ctx, const float *src, const float *src_normals, const float *tgt, const float *tgt_normals,
                  const int32_t *idx, int64_t n, int64_t nt, double max_d2, const float Rn[9], const kss_symm_params *sp,
                  double sums[KSS_P2L_NSUMS]);
int kss_symm_sums_dev(kss_ctx *ctx, const float *d_src, const float *d_src_normals, const float *d_tgt, const float *d_tgt_normals,
                      const int32_t *d_idx, int64_t n, int64_t nt, double max_d2, const float Rn[9], const kss_symm_params *sp,
                      double sums[KSS_P2L_NSUMS]);
/* normals as in kss_icp_gicp (NULL: computed from the cloud as passed in, the source before any motion).  trace_sums receives
 * trace_cap * KSS_P2L_NSUMS doubles.  The result is that of kss_icp_p2l. */
int kss_icp_symm(kss_ctx *ctx, const float *src, int64_t ns, const float *src_normals, const float *tgt, int64_t nt,
                 const float *tgt_normals, const kss_icp_params *p, const kss_symm_params *sp, kss_icp_result *res);
int kss_icp_symm_dev(kss_ctx *ctx, const float *d_src, int64_t ns, const float *d_src_normals, const float *d_tgt, int64_t nt,
                     const float *d_tgt_normals, const kss_icp_params *p, const kss_symm_params *sp, kss_icp_result *res);

/* ---- symmetric ICP for MANY pairs per call ----
 * Arguments as kss_icp_gicp_batch: packed float[n][3] clouds and npairs + 1 HOST offsets in points (the _dev form takes device clouds
 * and normals; the offsets and aligns stay host arrays).  src_normals_all is laid out like src_all, tgt_normals_all like tgt_all;
 * either may be NULL: then each cloud's normals are computed as kss_icp_symm computes them, per cloud, at sp->normals_k from the
 * cloud as passed in.  aligns: one int32 per pair, 0 or 1, the pair's align_normals, or NULL for sp->align_normals everywhere.
 * Nothing is redefined: the definition at kss_icp_symm holds for every pair -- R_F is the rotation block of the PAIR's own
 * accumulated transform, pass by pass -- and every pair's record -- T, iterations, state, converged, last_mse, pair 0's trace_* -- is
 * the single-pair call's BIT FOR BIT (fitness: within 2 ns 2^-53 relative, the NN engine's own summation order), in any batch order
 * and any split over calls, under every NN engine and tuning knob; results[i].pair_id = i.  Offsets whose first entry is not 0
 * address a sub-range of the packed arrays.  The pairs run in lockstep, one small table copy and two launches per pass behind the
 * NN pass whatever the pair count; a pair that ends -- converged, KSS_STATE_NO_CORRESPONDENCES, KSS_STATE_DEGENERATE -- leaves the
 * others untouched.  trace_* and fitness_idx / fitness_d2 describe pair 0.  KSS_ERR_ARG: NULL ctx (refused before anything touches
 * the device), offsets, sp or results; npairs <= 0; an empty pair; a set allreduce; sp->align_normals or an aligns entry other
 * than 0 or 1; normals_k outside 3..64 where a set of normals has to be computed; everything kss_icp_p2l_batch refuses. */
int kss_icp_symm_batch(kss_ctx *ctx, const float *src_all, const int64_t *src_off, const float *src_normals_all,
                       const float *tgt_all, const int64_t *tgt_off, const float *tgt_normals_all, int npairs,
                       const kss_icp_params *p, const kss_symm_params *sp, const int32_t *aligns, kss_icp_result *results);
int kss_icp_symm_batch_dev(kss_ctx *ctx, const float *d_src_all, const int64_t *src_off, const float *d_src_normals_all,
                           const float *d_tgt_all, const int64_t *tgt_off, const float *d_tgt_normals_all, int npairs,
                           const kss_icp_params *p, const kss_symm_params *sp, const int32_t *aligns, kss_icp_result *results);

/* ---- robust symmetric ICP for one pair: kss_icp_robust's M-estimator weights on kss_icp_symm's metric ----
 * For pairs that are far apart in angle AND carry gross outliers or overlap only in part.  The pass is kss_icp_symm's with
 * kss_icp_robust's weighting; nothing is redefined.  Per source i, with F, R_F, p, j, q, nq, ns, m, dot, n, w, d, c, v, r exactly as
 * written at kss_icp_symm (f64 on the widened floats, nothing fused, the same order):
 *   candidate   j in [0, nt), 0 <= d2 <= max_d2 (ordered compares in double: the robust form, which differs from kss_icp_symm's
 *               !(d2 > max_d2) only for a NaN d2, outside this definition), and all six normal components finite.  m of them.
 *   residual    x = r*r (one f64 product).
 *   key         (float)fabs(r): the f64 value rounded to nearest-even float; a source that is no candidate has a NaN key.  The
 *               rounding is monotone, so the k-th smallest key is the rounded k-th smallest |r|.
 *   scale       exactly kss_icp_robust's plane-metric rule.  Fixed (rp->scale > 0): c2 = scale*scale.  Automatic (rp->scale == 0):
 *               k = kss_trim_rank(m, 0.5), med = the exact k-th smallest key, c2 = kss_robust_scale2(KSS_METRIC_PLANE, tune, med,
 *               min_scale); m == 0: c2 = 0.  |n| <= 2 (the sum of two unit normals), so r is up to TWICE a point-to-plane distance:
 *               a fixed scale is in those units.
 *   weight      w = kss_robust_weight(loss, x, c2); kept by the division-free tests written at kss_icp_robust; cnt of them.
 *   record      KSS_P2L_NSUMS doubles in the robust plane layout with the symmetric v and r and wv[p] = w*v[p]: [0] += w, upper
 *               triangle += wv[p]*v[q], [22+p] += wv[p]*r, [28] += w*d2, [29] = m, [30] += (w*r)*r, [31] = cnt.
 *   order       kss_icp_symm's, a function of the source count alone.
 *   info        {m, c2, [0], cnt}.
 * Step and loop: kss_rigid_from_symm_sums on the record as it is ([0] is the weight total); cnt < min_correspondences ->
 * KSS_STATE_NO_CORRESPONDENCES, a failed Cholesky -> KSS_STATE_DEGENERATE, PCL's criteria on MSE = [28] / [0], fitness over ALL
 * sources, p->allreduce must be NULL.  Two consequences:
 *   KSS_LOSS_L2 is kss_icp_symm bit for bit: T, iterations, state, last_mse, every trace_Tk, and slots [0..28] and [30] of every
 *   trace_sums row; only [29] (m instead of the d2 total) and [31] (cnt instead of 0) differ.
 *   With align_normals = 1 the record, the keys and the info do not depend on the sign of any input normal, bit for bit: a flip
 *   negates v and r together.
 * rp->metric must be KSS_METRIC_PLANE (the residual is a signed plane distance and the scale rule the plane one);
 * rp->trace_robust and last_info as in kss_icp_robust; either set of normals may be NULL, computed as for kss_icp_symm; the sums
 * forms follow kss_symm_sums (Rn a HOST pointer, NULL = identity; the _dev form takes idx entries outside [0, nt) as no candidate,
 * the host form refuses them).  KSS_ERR_ARG: NULL ctx (refused before anything touches the device); everything kss_icp_symm refuses;
 * everything kss_icp_robust refuses in rp; rp->metric == KSS_METRIC_POINT.  Many pairs per call: kss_icp_symm_robust_batch
 * below.  Trimming on this metric, robust weights on generalized ICP, the C++ mirror classes and the CLI do not have it. */
int kss_symm_robust_sums(kss_ctx *ctx, const float *src, const float *src_normals, const float *tgt, const float *tgt_normals,
                         const int32_t *idx, int64_t n, int64_t nt, double max_d2, const float Rn[9], const kss_symm_params *sp,
                         const kss_robust_params *rp, double sums[KSS_P2L_NSUMS], double info[KSS_ROBUST_NINFO]);
int kss_symm_robust_sums_dev(kss_ctx *ctx, const float *d_src, const float *d_src_normals, const float *d_tgt,
                             const float *d_tgt_normals, const int32_t *d_idx, int64_t n, int64_t nt, double max_d2, const float Rn[9],
                             const kss_symm_params *sp, const kss_robust_params *rp, double sums[KSS_P2L_NSUMS],
                             double info[KSS_ROBUST_NINFO]);
int kss_icp_symm_robust(kss_ctx *ctx, const float *src, int64_t ns, const float *src_normals, const float *tgt, int64_t nt,
                        const float *tgt_normals, const kss_icp_params *p, const kss_symm_params *sp, const kss_robust_params *rp,
                        kss_icp_result *res, double last_info[KSS_ROBUST_NINFO]);
int kss_icp_symm_robust_dev(kss_ctx *ctx, const float *d_src, int64_t ns, const float *d_src_normals, const float *d_tgt, int64_t nt,
                            const float *d_tgt_normals, const kss_icp_params *p, const kss_symm_params *sp,
                            const kss_robust_params *rp, kss_icp_result *res, double last_info[KSS_ROBUST_NINFO]);

/* ---- robust symmetric ICP for MANY pairs per call ----
 * Arguments as kss_icp_symm_batch (packed float[n][3] clouds, npairs + 1 HOST offsets in points, a sub-range through a first offset
 * that is not 0; the _dev form takes device clouds and normals, the offsets, aligns and scales stay host arrays; either set of
 * normals may be NULL and is then computed per cloud at sp->normals_k) with kss_icp_robust_batch's rp, scales and info_all.
 * Nothing is redefined: the definition at kss_icp_symm_robust holds for every pair with the PAIR's own inputs --
 *   R_F      the rotation block of the pair's own accumulated float transform, pass by pass;
 *   align    aligns[i] (0 or 1), or sp->align_normals for every pair when aligns is NULL;
 *   scale    scales[i] > 0 fixed, scales[i] == 0 automatic from the pair's own median key of the pass; NULL: rp->scale for every
 *            pair.  A batch may mix both forms; loss, tune and min_scale are the batch's.
 * Every pair's record -- T, iterations, state, converged, last_mse, its info, pair 0's trace_Tk / trace_sums / rp->trace_robust -- is
 * the single-pair kss_icp_symm_robust call's BIT FOR BIT (fitness: within 2 ns 2^-53 relative), in any batch order and any split
 * over calls, under every NN engine and tuning knob; results[i].pair_id = i.  So a KSS_LOSS_L2 batch is kss_icp_symm_batch bit for
 * bit in T, iterations, state and last_mse.  info_all: npairs * KSS_ROBUST_NINFO doubles or NULL, every pair's last
 * {m, c2, sum of weights, cnt}, all zero for a pair that ran no pass.  The pairs run in lockstep: behind the NN pass one small table
 * copy, the key and selection launches when at least one pair is automatic, and two sums launches, whatever the pair count; a pair
 * that ends leaves the others untouched.  trace_*, rp->trace_robust and fitness_idx / fitness_d2 describe pair 0.
 * KSS_ERR_ARG: NULL ctx (refused before anything touches the device); everything kss_icp_symm_batch refuses; everything
 * kss_icp_symm_robust refuses in rp (rp->metric == KSS_METRIC_POINT among it); a scales entry that is negative or not finite; an
 * automatic pair with a tune that is not positive and finite.  A refused or failed call leaves the context usable. */
int kss_icp_symm_robust_batch(kss_ctx *ctx, const float *src_all, const int64_t *src_off, const float *src_normals_all,
                              const float *tgt_all, const int64_t *tgt_off, const float *tgt_normals_all, int npairs,
                              const kss_icp_params *p, const kss_symm_params *sp, const int32_t *aligns,
                              const kss_robust_params *rp, const double *scales, kss_icp_result *results, double *info_all);
int kss_icp_symm_robust_batch_dev(kss_ctx *ctx, const float *d_src_all, const int64_t *src_off, const float *d_src_normals_all,
                                  const float *d_tgt_all, const int64_t *tgt_off, const float *d_tgt_normals_all, int npairs,
                                  const kss_icp_params *p, const kss_symm_params *sp, const int32_t *aligns,
                                  const kss_robust_params *rp, const double *scales, kss_icp_result *results, double *info_all);

/* ---- (a13) apply the ICP Matrix4f to a full-resolution f64 cloud, KSS_ICP.hpp:224-230 ---- */
int kss_transform_apply(kss_ctx *ctx, const float T[16], const double *in, int64_t n, double *out);
int kss_transform_apply_dev(kss_ctx *ctx, const float T[16], const double *d_in, int64_t n, double *d_out);

/* pcl transformCloud / the PCL `output` cloud of align(): Matrix4f x float point, float result
 * (KSS_ICP.hpp:162,170-180 read it back as pointAlign in the full-resolution overload) */
int kss_transform_apply_f32(kss_ctx *ctx, const float T[16], const float *in, int64_t n, float *out);

/* ---- plain farthest-point sampling: fallback for clouds kss_downsample_aivs rejects (zero extent) ----
 * Exact farthest-point sampling in f64 starting from point 0 (ties -> lowest index); returns the m
 * selected points in selection order.  Not an AIVS restatement. */
int kss_downsample_fps(kss_ctx *ctx, const double *xyz, int64_t n, int64_t m, double *out, int32_t *out_idx);

/* ---- AIVS down-sampler: pointPipeline_init_point_withoutUniform + BallRegion_init_withoutNormal +
 *      AIVS_Pro_init + AIVS_simplification(point_num), KSS_ICP.hpp:71-81 (Method_AIVS_SimPro.hpp:94-154,
 *      ballRegionCompute.hpp:114-147) ----
 * Voxel grid, per-voxel farthest-point sampling in the reference's 8-colour order (one launch per colour, one
 * wavefront per voxel) and the accurate cut, with the reference's arithmetic.  out must hold capacity points;
 * *n_out receives the number selected, which can differ from point_num exactly as in the reference (fewer if the
 * per-voxel budgets add up to less; more if the accurate cut runs out of live closest pairs).  out_idx (may be
 * NULL) receives the indices into xyz.  KSS_ERR_ARG for degenerate (zero-extent / planar) clouds, which divide by
 * zero in the reference; KSS_ERR_CAPACITY if capacity is too small. */
int kss_downsample_aivs(kss_ctx *ctx, const double *xyz, int64_t n, int64_t point_num, double *out, int64_t capacity,
                        int64_t *n_out, int32_t *out_idx);

/* Both clouds of a registration at once (KSS_ICP.hpp:71-81 down-samples the target, then the source; the two do not depend
 * on each other): cloud 1 runs on a worker context of ctx, on a thread of its own, while the calling thread does cloud 0.
 * AIVS on a few thousand points is a chain of ~20 small launches and four host syncs -- two of them overlap almost
 * completely.  Same selections as two kss_downsample_aivs calls.  rc[k] receives cloud k's status (the codes of
 * kss_downsample_aivs: a degenerate cloud is KSS_ERR_ARG for that cloud only); the return value is KSS_OK unless an argument
 * is bad or the worker context cannot be created. */
int kss_downsample_aivs_pair(kss_ctx *ctx, const double *xyz0, int64_t n0, int64_t point_num0, double *out0, int64_t capacity0,
                             int64_t *n_out0, int32_t *out_idx0, const double *xyz1, int64_t n1, int64_t point_num1, double *out1,
                             int64_t capacity1, int64_t *n_out1, int32_t *out_idx1, int rc[2]);

/* ---- (8f #3) octree down-sampler: PCL_octree::PCL_Octree_Simplification_WithOutNormal, Method_Octree.hpp:77-165 ----
 * resolution = mean distance of the first 1000 points to their kn-th nearest point (kn = 2 below 80000 points, else
 * 7 * (n / 80000) capped at 35); occupied voxels of a pcl::octree::OctreePointCloudSearch of that resolution (PCL
 * 1.8.1 bounding-cube rules, insertion order) in depth-first order; every voxel centre replaced by its nearest
 * cloud point (ties -> lowest index).  out_idx receives one point index per voxel (repeats possible, as in the
 * reference); *n_out the voxel count.  Needs n >= 1000.  PCL is absent from the reference tree: parity unpinned. */
int kss_downsample_octree(kss_ctx *ctx, const double *xyz, int64_t n, int32_t *out_idx, int64_t capacity,
                          int64_t *n_out, double *resolution_out /* may be NULL */);

/* ---- PCR_QM: registrationMeasure.hpp:47-98 -> out = {MSE, RMSE, MAE} ---- */
int kss_pcr_qm(kss_ctx *ctx, const double *aligned, int64_t na, const double *tmpl, int64_t nt,
               double out[3]);

/* ---- (a16) KSSICP_Registration on already down-sampled clouds, KSS_ICP.hpp:86-131 + :185-233 */
typedef struct {
    double  scale;
    double  angle[3];         /* chosen Euler angles */
    double  R[9], t[3];       /* composite similarity p' = scale*R*p + t */
    double  c_src[3], c_tgt[3]; /* pre-shape centroids of S', T' (x_middle_S.. = c_tgt, x_middle.. = c_tgt - c_src) */
    float   T_icp[16];
    double  E_d_init;         /* :93 */
    double  final_fitness;    /* :130 */
    int32_t used_angle_list;  /* :99 branch */
    int32_t angle_index;
    int32_t n_angle_list;
    int32_t icp_iterations;
    int32_t icp_converged;
    int32_t grid;             /* g */
} kss_register_result;
int kss_register(kss_ctx *ctx, const double *src_sub, int64_t nss, const double *tgt_sub, int64_t nts,
                 const double *src_full, int64_t nsf, double accurate, int iter,
                 double *point_align /* nsf*3, may be NULL */, kss_register_result *res);

/* ---- many full KSS registrations (configs C3 / C5 read as registrations, not bare ICPs): for every pair the whole
 * KSSICP_init + KSSICP_Registration sequence (KSS_ICP.hpp:53-131) -- pNumber = min(n_S, n_T) / 2 capped at sample_cap
 * (2000 in the reference, :57-63), AIVS down-sampling of both clouds (farthest-point sampling when a cloud cannot be
 * voxelised), kss_register.  A registration is a chain of small launches that leaves most of the GPU idle, so the pairs
 * are spread over `workers` host threads, each with its own context / stream on the same device (0 = pick a default);
 * every pair is handled by exactly one worker with the same code as the one-pair path, so results[i] does not depend
 * on the worker count.  src_off / tgt_off are point offsets (npairs + 1 entries) into packed double[n][3] arrays.
 * point_align_all (may be NULL) receives the aligned full-resolution sources, laid out like src_all. */
int kss_register_batch(kss_ctx *ctx, const double *src_all, const int64_t *src_off, const double *tgt_all,
                       const int64_t *tgt_off, int npairs, int64_t sample_cap, double accurate, int iter, int workers,
                       double *point_align_all, kss_register_result *results);

/* ---- (8e) RCCL-backed kss_allreduce_fn: user = &kss_rccl_link{ctx, ncclComm_t}; ncclAllReduce(sum, f64) on the
 * context's stream between a host->device and a device->host copy of the n doubles (160 B per ICP iteration:
 * latency bound, one collective per iteration) ---- */
typedef struct { kss_ctx *ctx; void *rccl_comm; } kss_rccl_link;
int kss_rccl_allreduce_sum(void *user /* kss_rccl_link* */, double *values, int n);

/* ---- (8e) gather of per-pair result records over RCCL (ncclComm_t passed as void*) ----
 * all must hold world_size * n_local records; every rank receives every record. */
int kss_gather_results(kss_ctx *ctx, void *rccl_comm, int world_size,
                       const kss_icp_result *local, int n_local, kss_icp_result *all);

#ifdef __cplusplus
}
#endif
#endif /* KSSICP_H_ */
