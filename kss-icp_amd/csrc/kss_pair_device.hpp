// kss_pair_device.hpp -- the device code of the pair metrics (point-to-plane, trimmed, robust, generalized, symmetric and robust
// symmetric ICP, similarity ICP, voxelized generalized ICP), for one pair (kss_pair.hip) and for many pairs per call (kss_pairb.hip):
//   p2l_source / trim_point_source   what one source adds to its lane's accumulators (plane / point metric),
//   gicp_source / symm_source        the same for generalized and for symmetric ICP,
//   vgicp_source                     the same for voxelized generalized ICP: the voxel is looked up from the source's position,
//   sim_point_source                 the same for similarity ICP (the point metric and the kept sources' sum of squares),
//   the metric functors              one small struct per metric: the uniform parameters of a pass and the call of its body,
//   pair_walk                        the ONE walk both forms run: a lane's sources in steps of the grid, the functor's body per
//                                    source, then block_sum and the row store (or, for a keys metric, one key per source),
//   p2l_rows_column_sum              the fixed-order column sums of the plane metric's rows,
//   trim_key / trim_resolve_counts   the candidate test and the resolution of one radix digit from a lane's eight bin counts.
// pair_rows_kernel<M, SRC> (kss_pair.hip) gives workgroup b of stream_blocks(n) the sources b * 256 + t + k * 256 * grid;
// pairb_rows_kernel<M, PERM> (kss_pairb.hip) gives workgroup b of a pair's stream_blocks(ns_p) the same sources of that pair.  A
// pair's bits are the same alone and inside a batch because both are this one walk over the same bodies.
#pragma once
#include "kss_device.hpp"
#include "kss_gicp.hpp"
#include "kss_robust.hpp"

namespace kss {

// ---- robust ICP: what the per-source bodies below do for a candidate ---------------------------------------
// PAIR_PLAIN   add it to the record unweighted (kss_icp_p2l, kss_icp_trimmed and their batches: the code they always ran);
// PAIR_ROBUST  count it ([29] / [17] += 1), weigh it with robust_weight_of and, when kept, add the weighted terms and count it
//              again ([31] / [19] += 1): counts are sums of ones in f64, exact in any order;
// PAIR_KEY     write its selection key to *ra.key (the caller's, preset to NaN: no candidate) and add nothing.
enum { PAIR_PLAIN = 0, PAIR_ROBUST = 1, PAIR_KEY = 2 };
struct RobustArg {
    int loss = 0;
    double c2 = 0.0;
    float* key = nullptr;
};

// ---- point-to-plane --------------------------------------------------------------------------------------
constexpr int P2L_THREADS = 256;

// Where the current source positions come from: SRC_F3 packed float triples in original order (kss_p2l_sums); SRC_F4 the
// NN pass's float4 output in original order (brute-force engine); SRC_F4_PERM the same in cell order, perm[i] = the slot of
// original source i.
enum { SRC_F3 = 0, SRC_F4 = 1, SRC_F4_PERM = 2 };

// Source i (an index into idx / d2_in / perm / src3; in a batch the global one) against the target tgt / nrm of nt points.
// TRIM (trimmed ICP): max_d2 is the pass's cut tau (-1: no candidate) and a correspondence is kept when 0 <= d2 <= tau; the
// body and the summation order are the same, so an overlap of 1 -- tau = the largest d2 within max_d2 -- gives the untrimmed
// record bit for bit.  MODE != PAIR_PLAIN (robust ICP, with TRIM: the candidates are 0 <= d2 <= max_d2): see above.
template <int SRC, bool TRIM, int MODE = PAIR_PLAIN>
__device__ __forceinline__ void p2l_source(double (&acc)[P2L_NSUMS], const float* __restrict__ src3, const float4* __restrict__ src4,
                                           const int32_t* __restrict__ perm, const int32_t* __restrict__ idx,
                                           const float* __restrict__ d2_in, const float* __restrict__ tgt,
                                           const float* __restrict__ nrm, int64_t i, int64_t nt, double max_d2,
                                           const RobustArg ra = RobustArg()) {
    static_assert(MODE == PAIR_PLAIN || TRIM, "the robust candidates are those of the trimmed test");
    const int64_t j = idx[i];
    if (j < 0 || j >= nt) return;   // (kss_p2l_sums_dev: an index outside the target contributes nothing)
    float sx, sy, sz;
    if constexpr (SRC == SRC_F3) {
        sx = src3[3 * i]; sy = src3[3 * i + 1]; sz = src3[3 * i + 2];
    } else {
        const float4 p = src4[SRC == SRC_F4_PERM ? (int64_t)perm[i] : i];
        sx = p.x; sy = p.y; sz = p.z;
    }
    const float qx = tgt[3 * j], qy = tgt[3 * j + 1], qz = tgt[3 * j + 2];
    const float nx = nrm[3 * j], ny = nrm[3 * j + 1], nz = nrm[3 * j + 2];
    const double d2 = (double)(d2_in ? d2_in[i] : dist2<false>(sx, sy, sz, qx, qy, qz));
    if constexpr (MODE == PAIR_PLAIN) acc[29] += d2;
    // PCL: `if (distance > max_dist_sqr) continue;`, and a correspondence whose normal is not finite is dropped
    if ((TRIM ? d2 >= 0.0 && d2 <= max_d2 : !(d2 > max_d2)) && isfinite(nx) && isfinite(ny) && isfinite(nz)) {
        // float, left to right, no fma (PCL computes these in float and widens)
        const float a = nz * sy - ny * sz;
        const float b = nx * sz - nz * sx;
        const float c = ny * sx - nx * sy;
        const float r = ((nx * qx + ny * qy) + nz * qz) - nx * sx - ny * sy - nz * sz;
        if constexpr (MODE == PAIR_KEY) {
            *ra.key = fabsf(r);
            return;
        }
        const double v[6] = {(double)a, (double)b, (double)c, (double)nx, (double)ny, (double)nz};
        const double rd = (double)r;
        if constexpr (MODE == PAIR_ROBUST) {
            acc[29] += 1.0;
            bool kept;
            const double w = robust_weight_of(ra.loss, rd * rd, ra.c2, kept);   // (the product of two widened floats is exact)
            if (!kept) return;
            double wv[6];
#pragma unroll
            for (int p = 0; p < 6; ++p) wv[p] = w * v[p];
            acc[0] += w;
            int k = 1;
#pragma unroll
            for (int p = 0; p < 6; ++p)
#pragma unroll
                for (int q = p; q < 6; ++q) acc[k++] += wv[p] * v[q];
#pragma unroll
            for (int p = 0; p < 6; ++p) acc[22 + p] += wv[p] * rd;
            acc[28] += w * d2;
            acc[30] += (w * rd) * rd;
            acc[31] += 1.0;
        } else {
            acc[0] += 1.0;
            int k = 1;
#pragma unroll
            for (int p = 0; p < 6; ++p)
#pragma unroll
                for (int q = p; q < 6; ++q) acc[k++] += v[p] * v[q];
#pragma unroll
            for (int p = 0; p < 6; ++p) acc[22 + p] += v[p] * rd;
            acc[28] += d2;
            acc[30] += rd * rd;
        }
    }
}

// ---- generalized ICP ------------------------------------------------------------------------------------
// What one kept correspondence adds to the record: its metric M (upper triangle), the source's widened position p, d = q - p and
// the pass's squared distance d2 for slot [28].  Shared by gicp_source (q a target point) and vgicp_source (q a voxel's mean).
__device__ __forceinline__ void gicp_accumulate(double (&acc)[P2L_NSUMS], const double (&M)[6], double px, double py, double pz, double d0,
                                                double d1, double dz, double d2) {
    // M as rows (symmetric)
    const double Mr[3][3] = {{M[0], M[1], M[2]}, {M[1], M[3], M[4]}, {M[2], M[4], M[5]}};
    double u[3], B[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a) u[a] = (Mr[a][0] * d0 + Mr[a][1] * d1) + Mr[a][2] * dz;
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        B[0][b] = py * Mr[2][b] - pz * Mr[1][b];
        B[1][b] = pz * Mr[0][b] - px * Mr[2][b];
        B[2][b] = px * Mr[1][b] - py * Mr[0][b];
    }
    acc[0] += 1.0;
    // row 0: UL00 UL01 UL02 B00 B01 B02; row 1: UL11 UL12 B10 B11 B12; row 2: UL22 B20 B21 B22; then M
    acc[1] += B[0][2] * py - B[0][1] * pz;
    acc[2] += B[0][0] * pz - B[0][2] * px;
    acc[3] += B[0][1] * px - B[0][0] * py;
    acc[4] += B[0][0]; acc[5] += B[0][1]; acc[6] += B[0][2];
    acc[7] += B[1][0] * pz - B[1][2] * px;
    acc[8] += B[1][1] * px - B[1][0] * py;
    acc[9] += B[1][0]; acc[10] += B[1][1]; acc[11] += B[1][2];
    acc[12] += B[2][1] * px - B[2][0] * py;
    acc[13] += B[2][0]; acc[14] += B[2][1]; acc[15] += B[2][2];
    acc[16] += M[0]; acc[17] += M[1]; acc[18] += M[2];
    acc[19] += M[3]; acc[20] += M[4];
    acc[21] += M[5];
    acc[22] += py * u[2] - pz * u[1];
    acc[23] += pz * u[0] - px * u[2];
    acc[24] += px * u[1] - py * u[0];
    acc[25] += u[0]; acc[26] += u[1]; acc[27] += u[2];
    acc[28] += d2;
    acc[30] += (d0 * u[0] + d1 * u[1]) + dz * u[2];
}

// Source i as in p2l_source, with the source's own normal sn[3 * i ..] (by ORIGINAL index; in a batch the global one) turned by Rn: the definition at
// kss_icp_gicp in include/kssicp.h.  The 6 x 6 block A^T M A of A = [ -[p]x | I ] is formed by blocks -- lower right M, upper
// right B = [p]x M, upper left B [p]x^T -- and not by a generic triple product: 54 f64 multiplications instead of 162.
template <int SRC>
__device__ __forceinline__ void gicp_source(double (&acc)[P2L_NSUMS], const float* __restrict__ src3, const float4* __restrict__ src4,
                                            const int32_t* __restrict__ perm, const int32_t* __restrict__ idx,
                                            const float* __restrict__ d2_in, const float* __restrict__ sn, const float* __restrict__ tgt,
                                            const float* __restrict__ nrm, int64_t i, int64_t nt, double max_d2, const GicpRot& Rn, double e) {
    const int64_t j = idx[i];
    if (j < 0 || j >= nt) return;
    float sx, sy, sz;
    if constexpr (SRC == SRC_F3) {
        sx = src3[3 * i]; sy = src3[3 * i + 1]; sz = src3[3 * i + 2];
    } else {
        const float4 p = src4[SRC == SRC_F4_PERM ? (int64_t)perm[i] : i];
        sx = p.x; sy = p.y; sz = p.z;
    }
    const float qx = tgt[3 * j], qy = tgt[3 * j + 1], qz = tgt[3 * j + 2];
    const float nx = nrm[3 * j], ny = nrm[3 * j + 1], nz = nrm[3 * j + 2];
    const float ux = sn[3 * i], uy = sn[3 * i + 1], uz = sn[3 * i + 2];
    const double d2 = (double)(d2_in ? d2_in[i] : dist2<false>(sx, sy, sz, qx, qy, qz));
    acc[29] += d2;
    if (!(d2 > max_d2) && isfinite(nx) && isfinite(ny) && isfinite(nz) && isfinite(ux) && isfinite(uy) && isfinite(uz)) {
        const double nq[3] = {(double)nx, (double)ny, (double)nz};
        const double us[3] = {(double)ux, (double)uy, (double)uz};
        double m[3], M[6];
#pragma unroll
        for (int k = 0; k < 3; ++k) m[k] = ((double)Rn.r[3 * k] * us[0] + (double)Rn.r[3 * k + 1] * us[1]) + (double)Rn.r[3 * k + 2] * us[2];
        if (!gicp_metric_of(nq, m, e, M)) return;
        const double px = (double)sx, py = (double)sy, pz = (double)sz;
        gicp_accumulate(acc, M, px, py, pz, (double)qx - px, (double)qy - py, (double)qz - pz, d2);
    }
}

// ---- voxelized generalized ICP ---------------------------------------------------------------------------
// The 7- and 27-voxel neighbourhoods (kss_vmap_set_neighbourhood): what a source at the moved position s with the
// lattice coordinates f adds when the map's setting is nb = 7 or 27 -- one correspondence per neighbour cell that is in the window
// and occupied, the centre first, then the others in ascending (o_z, o_y, o_x).  Two phases, so that no table read waits for an
// accumulation:
//   1  every table read of the neighbourhood, unrolled: up to 27 independent loads (a row of three x-neighbours is twelve
//      contiguous bytes), each kept in this lane's own column of an LDS array, and a bit per occupied neighbour -- bit 0 the
//      centre, bits 1 .. 26 the others in the definition's order;
//   2  a loop over the set bits, lowest first: the voxel index back from LDS, the record's ten doubles, and vgicp_correspondence,
//      the body vgicp_source runs on its one voxel, so a source whose only occupied neighbour is its own voxel adds setting 1's
//      terms in setting 1's order.  The loop is not unrolled: one body.
// A lane reads only what it wrote itself, in program order: no barrier.  The source's normal is tested, and m formed, once.
constexpr int VGICP_NB_MAX = 27;
// What ONE correspondence adds: the source at the widened position p, its turned normal m, against the voxel record rec =
// {N, mean x y z, S00 S01 S02 S11 S12 S22}.  The one body of both lookups -- vgicp_source's own voxel and every neighbour of
// vgicp_neighbours -- so the identity of the header (a source whose only occupied neighbour is its own voxel adds setting 1's terms)
// holds by construction.
__device__ __forceinline__ void vgicp_correspondence(double (&acc)[P2L_NSUMS], const double* __restrict__ rec, double px, double py, double pz,
                                                     const double (&m)[3], double max_d2, double e) {
    const double d0 = rec[1] - px, d1 = rec[2] - py, dz = rec[3] - pz;
    const double dd = (d0 * d0 + d1 * d1) + dz * dz;
    if (dd > max_d2) return;
    const double Q[6] = {rec[4], rec[5], rec[6], rec[7], rec[8], rec[9]};
    double M[6];
    if (!gicp_metric_of_g(Q, m, e, M)) return;
    gicp_accumulate(acc, M, px, py, pz, d0, d1, dz, dd);
}
__device__ __forceinline__ void vgicp_neighbours(double (&acc)[P2L_NSUMS], const float* __restrict__ sn, const VmapDev& v, int64_t i, float sx, float sy,
                                                 float sz, float fx, float fy, float fz, double max_d2, const GicpRot& Rn, double e, int nb) {
    __shared__ int32_t nbv[VGICP_NB_MAX][P2L_THREADS];
    // a lattice cell: |f_a| <= 2^24 on all axes, compared in float (a NaN has none); then the conversion to int is exact
    constexpr float LIM = 16777216.0f;
    if (!(fabsf(fx) <= LIM && fabsf(fy) <= LIM && fabsf(fz) <= LIM)) return;
    const float ux = sn[3 * i], uy = sn[3 * i + 1], uz = sn[3 * i + 2];
    // local cell of the source: |a|, |base| <= 2^24, so the difference and c + o are plain ints; a + o is in the window iff
    // 0 <= c + o < dims
    const int cx = (int)fx - v.base[0], cy = (int)fy - v.base[1], cz = (int)fz - v.base[2];
    const int64_t centre = ((int64_t)cz * v.dims[1] + cy) * v.dims[0] + cx;   // (read only behind its neighbour's window test)
    const int64_t sy_ = v.dims[0], sz_ = (int64_t)v.dims[1] * v.dims[0];
    const bool full = nb == 27;
    unsigned mask = 0;
#pragma unroll
    for (int k = 0; k < VGICP_NB_MAX; ++k) {
        const int ox = k % 3 - 1, oy = (k / 3) % 3 - 1, oz = k / 9 - 1;                  // ascending (o_z, o_y, o_x)
        const int bit = k == 13 ? 0 : (k < 13 ? k + 1 : k);                             // the centre first
        const bool axis = (ox != 0) + (oy != 0) + (oz != 0) <= 1;                        // one of the 7
        const int x = cx + ox, y = cy + oy, z = cz + oz;
        int32_t vox = -1;
        if ((axis || full) && x >= 0 && x < v.dims[0] && y >= 0 && y < v.dims[1] && z >= 0 && z < v.dims[2])
            vox = v.cell[centre + (oz * sz_ + oy * sy_ + ox)];
        if (axis || full) nbv[bit][threadIdx.x] = vox;   // (a slot is read only where its bit is set: at 7 the other 20 are not written)
        mask |= (vox >= 0 ? 1u : 0u) << bit;
    }
    if (mask == 0 || !(isfinite(ux) && isfinite(uy) && isfinite(uz))) return;
    const double px = (double)sx, py = (double)sy, pz = (double)sz;
    const double us[3] = {(double)ux, (double)uy, (double)uz};
    double m[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) m[k] = ((double)Rn.r[3 * k] * us[0] + (double)Rn.r[3 * k + 1] * us[1]) + (double)Rn.r[3 * k + 2] * us[2];
#pragma unroll 1
    while (mask) {
        const int bit = __ffs(mask) - 1;
        mask &= mask - 1;
        vgicp_correspondence(acc, v.rec + (int64_t)nbv[bit][threadIdx.x] * VMAP_NSTAT, px, py, pz, m, max_d2, e);
    }
}

// Source i against the voxel map v: the definition at kss_icp_vgicp in include/kssicp.h.  No idx is read: the voxel is looked up
// from the source's own position -- f_a = floorf((p_a - lo_a) * inv), the build's expression, compared in float so that a NaN
// has no voxel -- and the voxel's mean and average n n^T stand where gicp_source has q and nq nq^T.  MOVE: the position read
// from `in` is first moved by the float 3 x 4 T as transform_apply_f32_kernel moves it and stored to `out` (another array), so a
// pass needs no launch for the move.
template <bool MOVE, bool NEIGH = false>
__device__ __forceinline__ void vgicp_source(double (&acc)[P2L_NSUMS], const float* __restrict__ in, float* __restrict__ out, const float* __restrict__ sn,
                                             const VmapDev& v, const VmapMove& T, int64_t i, double max_d2, const GicpRot& Rn, double e, int nb = 1) {
    float sx = in[3 * i], sy = in[3 * i + 1], sz = in[3 * i + 2];
    if constexpr (MOVE) {
        const float x = sx, y = sy, z = sz;
        sx = ((T.m[0] * x + T.m[1] * y) + T.m[2] * z) + T.m[3];
        sy = ((T.m[4] * x + T.m[5] * y) + T.m[6] * z) + T.m[7];
        sz = ((T.m[8] * x + T.m[9] * y) + T.m[10] * z) + T.m[11];
        out[3 * i] = sx; out[3 * i + 1] = sy; out[3 * i + 2] = sz;
    }
    const float fx = floorf((sx - v.lo[0]) * v.inv), fy = floorf((sy - v.lo[1]) * v.inv), fz = floorf((sz - v.lo[2]) * v.inv);
    if constexpr (NEIGH) {   // (the move and its store are done: once per source, before any lookup)
        vgicp_neighbours(acc, sn, v, i, sx, sy, sz, fx, fy, fz, max_d2, Rn, e, nb);
        return;
    }
    // the window (kss_vmap_shift): base <= f < base + dims, both bounds exact in float; base = 0 gives 0 <= f < dims
    if (!(fx >= (float)v.base[0] && fx < (float)(v.base[0] + v.dims[0]) && fy >= (float)v.base[1] && fy < (float)(v.base[1] + v.dims[1]) &&
          fz >= (float)v.base[2] && fz < (float)(v.base[2] + v.dims[2]))) return;
    // (inside the window |f| <= 2^24, so the conversion to int is the conversion to int64; inside the table: the test above)
    const int cx = (int)fx - v.base[0], cy = (int)fy - v.base[1], cz = (int)fz - v.base[2];
    const int32_t vox = v.cell[((int64_t)cz * v.dims[1] + cy) * v.dims[0] + cx];
    if (vox < 0) return;
    const float ux = sn[3 * i], uy = sn[3 * i + 1], uz = sn[3 * i + 2];
    if (!(isfinite(ux) && isfinite(uy) && isfinite(uz))) return;
    const double us[3] = {(double)ux, (double)uy, (double)uz};
    double m[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) m[k] = ((double)Rn.r[3 * k] * us[0] + (double)Rn.r[3 * k + 1] * us[1]) + (double)Rn.r[3 * k + 2] * us[2];
    vgicp_correspondence(acc, v.rec + (int64_t)vox * VMAP_NSTAT, (double)sx, (double)sy, (double)sz, m, max_d2, e);
}

// ---- symmetric ICP --------------------------------------------------------------------------------------
// Source i as in gicp_source: the definition at kss_icp_symm in include/kssicp.h.  The plane metric's record with
// n = nq +- m in place of the target's normal and w = p + q in place of p; the 21 + 6 products of v v^T and v r directly.
// MODE != PAIR_PLAIN (robust symmetric ICP; the definition at kss_icp_symm_robust): the candidates are
// 0 <= d2 <= max_d2 as in p2l_source's robust form, x = r * r, the key is (float)fabs(r), and w * v[p] is formed inside the
// unrolled loops (v and w v are never both live as arrays).
template <int SRC, int MODE = PAIR_PLAIN>
__device__ __forceinline__ void symm_source(double (&acc)[P2L_NSUMS], const float* __restrict__ src3, const float4* __restrict__ src4,
                                            const int32_t* __restrict__ perm, const int32_t* __restrict__ idx,
                                            const float* __restrict__ d2_in, const float* __restrict__ sn, const float* __restrict__ tgt,
                                            const float* __restrict__ nrm, int64_t i, int64_t nt, double max_d2, const GicpRot& Rn, int align,
                                            const RobustArg ra = RobustArg()) {
    const int64_t j = idx[i];
    if (j < 0 || j >= nt) return;
    float sx, sy, sz;
    if constexpr (SRC == SRC_F3) {
        sx = src3[3 * i]; sy = src3[3 * i + 1]; sz = src3[3 * i + 2];
    } else {
        const float4 p = src4[SRC == SRC_F4_PERM ? (int64_t)perm[i] : i];
        sx = p.x; sy = p.y; sz = p.z;
    }
    const float qx = tgt[3 * j], qy = tgt[3 * j + 1], qz = tgt[3 * j + 2];
    const float nx = nrm[3 * j], ny = nrm[3 * j + 1], nz = nrm[3 * j + 2];
    const float ux = sn[3 * i], uy = sn[3 * i + 1], uz = sn[3 * i + 2];
    const double d2 = (double)(d2_in ? d2_in[i] : dist2<false>(sx, sy, sz, qx, qy, qz));
    if constexpr (MODE == PAIR_PLAIN) acc[29] += d2;
    if ((MODE == PAIR_PLAIN ? !(d2 > max_d2) : d2 >= 0.0 && d2 <= max_d2) && isfinite(nx) && isfinite(ny) && isfinite(nz) && isfinite(ux) &&
        isfinite(uy) && isfinite(uz)) {
        const double nq[3] = {(double)nx, (double)ny, (double)nz};
        const double us[3] = {(double)ux, (double)uy, (double)uz};
        double m[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) m[k] = ((double)Rn.r[3 * k] * us[0] + (double)Rn.r[3 * k + 1] * us[1]) + (double)Rn.r[3 * k + 2] * us[2];
        const double dot = (m[0] * nq[0] + m[1] * nq[1]) + m[2] * nq[2];
        const bool flip = align && dot < 0.0;
        const double n0 = flip ? nq[0] - m[0] : nq[0] + m[0];
        const double n1 = flip ? nq[1] - m[1] : nq[1] + m[1];
        const double n2 = flip ? nq[2] - m[2] : nq[2] + m[2];
        const double px = (double)sx, py = (double)sy, pz = (double)sz;
        const double qxd = (double)qx, qyd = (double)qy, qzd = (double)qz;
        const double w0 = px + qxd, w1 = py + qyd, w2 = pz + qzd;
        const double d0 = qxd - px, d1 = qyd - py, dz = qzd - pz;
        const double r = (d0 * n0 + d1 * n1) + dz * n2;
        if constexpr (MODE == PAIR_KEY) {
            *ra.key = (float)fabs(r);
            return;
        }
        double w = 1.0;
        if constexpr (MODE == PAIR_ROBUST) {   // the weight first: a source that is not kept forms no v, and the division's temporaries are gone before v is live
            acc[29] += 1.0;
            bool kept;
            w = robust_weight_of(ra.loss, r * r, ra.c2, kept);
            if (!kept) return;
        }
        const double v[6] = {w1 * n2 - w2 * n1, w2 * n0 - w0 * n2, w0 * n1 - w1 * n0, n0, n1, n2};
        if constexpr (MODE == PAIR_ROBUST) {
            acc[0] += w;
            int k = 1;
#pragma unroll
            for (int p = 0; p < 6; ++p) {
                const double wvp = w * v[p];
#pragma unroll
                for (int q = p; q < 6; ++q) acc[k++] += wvp * v[q];
                acc[22 + p] += wvp * r;
            }
            acc[28] += w * d2;
            acc[30] += (w * r) * r;
            acc[31] += 1.0;
        } else {
            acc[0] += 1.0;
            int k = 1;
#pragma unroll
            for (int p = 0; p < 6; ++p)
#pragma unroll
                for (int q = p; q < 6; ++q) acc[k++] += v[p] * v[q];
#pragma unroll
            for (int p = 0; p < 6; ++p) acc[22 + p] += v[p] * r;
            acc[28] += d2;
            acc[30] += r * r;
        }
    }
}

// Column c of the rows: lane (g, c) = (tid / 32, tid % 32) takes rows g, g + 8, g + 16, ... (32 lanes read one 256-byte
// row) into eight accumulators -- row g + 8 (8 m + u) goes to accumulator u while a whole round of eight fits, the tail to
// accumulator 0 -- added as ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7)); then the 8 group totals in group order.
// (Eight loads in flight per lane: with one accumulator the lane waits out one memory latency per row, 12 us at 391 rows.)
// The column total in lanes tid < P2L_NSUMS.  Needs blockDim.x == P2L_THREADS.
constexpr int P2L_GROUPS = P2L_THREADS / P2L_NSUMS;
__device__ __forceinline__ double p2l_rows_column_sum(const double* __restrict__ rows, int nrows, double (*shg)[P2L_NSUMS]) {
    const int g = threadIdx.x / P2L_NSUMS, c = threadIdx.x % P2L_NSUMS;
    constexpr int G = P2L_GROUPS;
    double a[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int k = g;
    for (; k + 7 * G < nrows; k += 8 * G) {
#pragma unroll
        for (int u = 0; u < 8; ++u) a[u] += rows[(int64_t)(k + u * G) * P2L_NSUMS + c];
    }
    for (; k < nrows; k += G) a[0] += rows[(int64_t)k * P2L_NSUMS + c];
    shg[g][c] = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
    __syncthreads();
    double v = 0.0;
    if (threadIdx.x < P2L_NSUMS)
        for (int gg = 0; gg < P2L_GROUPS; ++gg) v += shg[gg][threadIdx.x];
    return v;
}

// ---- trimmed ICP ----------------------------------------------------------------------------------------
constexpr int TRIM_BINS = 2048;                 // row width: the widest digit
constexpr int TRIM_HIST_THREADS = 256;
constexpr int TRIM_LANE_BINS = TRIM_BINS / TRIM_HIST_THREADS;   // bins per lane when a digit is resolved
constexpr int TRIM_THREADS = 256;
// digit d covers key bits [trim_shift(d), trim_shift(d) + trim_bits(d))
// (a key has its sign bit clear: 31 bits; the first digit is the exponent and three mantissa bits)
__device__ __host__ constexpr int trim_shift(int d) { return d == 0 ? 20 : d == 1 ? 10 : 0; }
__device__ __host__ constexpr int trim_bits(int d) { return d == 0 ? 11 : 10; }

// candidate test and key of one squared distance
__device__ __forceinline__ bool trim_key(float d2f, double max_d2, unsigned& key) {
    const double d = (double)d2f;
    key = d2f == 0.0f ? 0u : __float_as_uint(d2f);
    return d >= 0.0 && d <= max_d2;
}

// Resolves digit DIGIT from its bin counts, lane t holding the counts c[0..7] of the bins 8t .. 8t + 7: the state after it
// (prefix, rank inside the keys that carry it, m, k; after the last digit cut and kept) in *out (LDS), valid for every lane
// after the call.  *prev is the state before it (digit 0 has none: m is the total of the counts); prev and out must not
// alias.  Needs blockDim.x == TRIM_HIST_THREADS.
template <int DIGIT>
__device__ __forceinline__ void trim_resolve_counts(const unsigned (&c)[TRIM_LANE_BINS], double overlap,
                                                    const TrimState* __restrict__ prev, TrimState* out, unsigned* wave_tot) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    // inclusive scan of the lane totals over the workgroup (counts stay below 2^31: n is capped by the C-ABI)
    unsigned mine = 0u;
#pragma unroll
    for (int q = 0; q < TRIM_LANE_BINS; ++q) mine += c[q];
    unsigned inc = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned o = __shfl_up(inc, off, 64);
        if (lane >= off) inc += o;
    }
    if (lane == 63) wave_tot[wave] = inc;
    __syncthreads();
    unsigned base = 0u, total = 0u;
    for (int w = 0; w < TRIM_HIST_THREADS / 64; ++w) {
        if (w < wave) base += wave_tot[w];
        total += wave_tot[w];
    }
    const unsigned excl = base + inc - mine;   // keys of this digit below bin 8t
    long long m, k, rank;
    unsigned prefix;
    if constexpr (DIGIT == 0) {
        m = (long long)total;
        k = trim_rank_of(m, overlap);
        rank = k;
        prefix = 0u;
    } else {
        m = prev->m; k = prev->k; rank = prev->rank; prefix = prev->prefix;
    }
    if (t == 0) {   // no candidate (rank 0); otherwise overwritten below by the lane that holds the rank
        TrimState o;
        o.prefix = 0u; o.pad = 0u; o.rank = 0; o.m = m; o.k = k; o.cut = -1.0; o.kept = 0;
        *out = o;
    }
    __syncthreads();
    const unsigned rk = (unsigned)rank;
    if (rank > 0 && excl < rk && rk <= excl + mine) {   // exactly one lane: the counts of a digit add up to at least the rank
        unsigned below = excl, bin = 0u, cnt = 0u;
        bool found = false;
#pragma unroll
        for (int q = 0; q < TRIM_LANE_BINS; ++q) {
            if (!found) {
                if (rk <= below + c[q]) { found = true; bin = (unsigned)(TRIM_LANE_BINS * t + q); cnt = c[q]; }
                else below += c[q];
            }
        }
        TrimState o;
        o.prefix = (prefix << trim_bits(DIGIT)) | bin;
        o.pad = 0u;
        o.rank = (long long)(rk - below);
        o.m = m; o.k = k;
        o.cut = -1.0; o.kept = 0;
        if constexpr (DIGIT == 2) {
            o.cut = (double)__uint_as_float(o.prefix);   // tau
            o.kept = (k - o.rank) + (long long)cnt;      // the keys below tau + the whole tie at tau
        }
        *out = o;
    }
    __syncthreads();
}

// point metric: source i (as in p2l_source) on accumulate_corr's arithmetic, kept when 0 <= d2 <= cut.  MODE != PAIR_PLAIN
// (robust ICP): as above, cut = max_d2; F3 (kss_robust_sums): the sources are the packed float triples src3 and d2 is
// recomputed as kss_cov does.
template <bool PERM, int MODE = PAIR_PLAIN, bool F3 = false>
__device__ __forceinline__ void trim_point_source(double (&acc)[NSUMS], const float4* __restrict__ src4, const int32_t* __restrict__ perm,
                                                  const int32_t* __restrict__ idx, const float* __restrict__ d2_in,
                                                  const float* __restrict__ tgt, int64_t i, int64_t nt, double cut,
                                                  const float* __restrict__ src3 = nullptr, const RobustArg ra = RobustArg()) {
    static_assert(MODE != PAIR_PLAIN || !F3, "the unweighted form reads the NN pass's float4 output");
    const int64_t j = idx[i];
    if (j < 0 || j >= nt) return;
    if constexpr (MODE == PAIR_PLAIN) {
        const float d2f = d2_in[i];
        const double d2 = (double)d2f;
        if (!(d2 >= 0.0 && d2 <= cut)) return;
        const float4 p = src4[PERM ? (int64_t)perm[i] : i];
        accumulate_corr(acc, p.x, p.y, p.z, tgt[3 * j], tgt[3 * j + 1], tgt[3 * j + 2], d2f, cut);
    } else {
        float sx, sy, sz;
        if constexpr (F3) {
            sx = src3[3 * i]; sy = src3[3 * i + 1]; sz = src3[3 * i + 2];
        } else {
            const float4 p = src4[PERM ? (int64_t)perm[i] : i];
            sx = p.x; sy = p.y; sz = p.z;
        }
        const float qx = tgt[3 * j], qy = tgt[3 * j + 1], qz = tgt[3 * j + 2];
        const float d2f = F3 ? dist2<false>(sx, sy, sz, qx, qy, qz) : d2_in[i];
        const double d2 = (double)d2f;
        if (!(d2 >= 0.0 && d2 <= cut)) return;
        if constexpr (MODE == PAIR_KEY) {
            *ra.key = d2f;
            return;
        }
        acc[17] += 1.0;
        bool kept;
        const double w = robust_weight_of(ra.loss, d2, ra.c2, kept);
        if (!kept) return;
        const double p[3] = {(double)sx, (double)sy, (double)sz};
        const double q[3] = {(double)qx, (double)qy, (double)qz};
        double ws[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) ws[k] = w * p[k];
        acc[0] += w;
#pragma unroll
        for (int k = 0; k < 3; ++k) { acc[1 + k] += ws[k]; acc[4 + k] += w * q[k]; }
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int l = 0; l < 3; ++l) acc[7 + 3 * k + l] += ws[k] * q[l];
        acc[16] += w * d2;
        acc[19] += 1.0;
    }
}

// ---- similarity ICP ---------------------------------------------------------------------------------------
// Source i as in trim_point_source's unweighted form: slots [0..16] are that record bit for bit (accumulate_corr's terms in its
// order), and [17] += |p|^2 of the kept source -- f64 on the widened floats, the squares exact, nothing fused -- from the p
// already in registers for the cross terms.  [18], [19] are not touched.  SRC_F3 (kss_sim_sums): the sources are the packed
// float triples and d2 is recomputed as kss_cov does, lim = max_d2; otherwise lim = the pass's cut tau (-1: no candidate).
template <int SRC>
__device__ __forceinline__ void sim_point_source(double (&acc)[NSUMS], const float* __restrict__ src3, const float4* __restrict__ src4,
                                                 const int32_t* __restrict__ perm, const int32_t* __restrict__ idx,
                                                 const float* __restrict__ d2_in, const float* __restrict__ tgt, int64_t i, int64_t nt,
                                                 double lim) {
    const int64_t j = idx[i];
    if (j < 0 || j >= nt) return;
    float sx, sy, sz, d2f;
    if constexpr (SRC == SRC_F3) {
        sx = src3[3 * i]; sy = src3[3 * i + 1]; sz = src3[3 * i + 2];
        d2f = dist2<false>(sx, sy, sz, tgt[3 * j], tgt[3 * j + 1], tgt[3 * j + 2]);
    } else {
        d2f = d2_in[i];
    }
    const double d2 = (double)d2f;
    if (!(d2 >= 0.0 && d2 <= lim)) return;
    if constexpr (SRC != SRC_F3) {
        const float4 p4 = src4[SRC == SRC_F4_PERM ? (int64_t)perm[i] : i];
        sx = p4.x; sy = p4.y; sz = p4.z;
    }
    const double p[3] = {(double)sx, (double)sy, (double)sz};
    const double q[3] = {(double)tgt[3 * j], (double)tgt[3 * j + 1], (double)tgt[3 * j + 2]};
    acc[0] += 1.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) { acc[1 + k] += p[k]; acc[4 + k] += q[k]; }
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int l = 0; l < 3; ++l) acc[7 + 3 * k + l] += p[k] * q[l];
    acc[16] += d2;
    acc[17] += (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2];
}

// ---- the metric functors and the walk ----------------------------------------------------------------------
// c2 of a robust pass, derived by every workgroup that needs it from the selection's last TrimState (sel: not read with a fixed
// scale): one f64 product or two, the same bits everywhere
__device__ __forceinline__ double robust_pass_c2(const RobustScale& rs, bool plane, const TrimState* __restrict__ sel) {
    if (!rs.autoscale) return rs.c2;
    const double med = sel->cut;   // the median key widened (-1: no candidate)
    return med >= 0.0 ? robust_scale2_of(plane, rs.K, med, rs.min2) : 0.0;
}

// A metric M carries the uniform parameters of one pass of one pair.  It is built on the host from the values of a single pair
// (and travels into pair_rows_kernel by value) or on the device from the per-pair tables at pair p (pairb_rows_kernel); begin()
// then reads what the pass left in device memory (the cut, the median key), once per workgroup.  NC: the columns of its rows;
// KEYS: it writes one selection key per source and no rows; F3: it has a form for packed float triples (PairSrc::src3).
// source<SRC>(acc, s, tgt, nrm, i, nt, key) is the body's call, unchanged.
template <bool TRIM>
struct PlaneMetric {   // plane metric, untrimmed (lim = max_d2) or trimmed (lim = the pass's cut)
    static constexpr int NC = P2L_NSUMS;
    static constexpr bool KEYS = false, F3 = true;
    const double* cut;
    double lim;
    PlaneMetric(double max_d2, const double* cut_) : cut(cut_), lim(max_d2) {}
    __device__ PlaneMetric(const PairbArgs& a, int p) : cut(&a.ts[p].cut), lim(a.s.max_d2) {}
    __device__ void begin() { if constexpr (TRIM) lim = *cut; }   // tau of this pass (-1: no candidate), written by the selection
    template <int SRC>
    __device__ __forceinline__ void source(double (&acc)[NC], const PairSrc& s, const float* tgt, const float* nrm, int64_t i, int64_t nt, float*) const {
        p2l_source<SRC, TRIM>(acc, s.src3, s.src4, s.perm, s.idx, s.d2, tgt, nrm, i, nt, lim);
    }
};
struct PointTrimMetric {   // point metric over the correspondences at or below the pass's cut
    static constexpr int NC = NSUMS;
    static constexpr bool KEYS = false, F3 = false;
    const double* cut;
    double lim = 0.0;
    explicit PointTrimMetric(const double* cut_) : cut(cut_) {}
    __device__ PointTrimMetric(const PairbArgs& a, int p) : cut(&a.ts[p].cut) {}
    __device__ void begin() { lim = *cut; }
    template <int SRC>
    __device__ __forceinline__ void source(double (&acc)[NC], const PairSrc& s, const float* tgt, const float*, int64_t i, int64_t nt, float*) const {
        trim_point_source<SRC == SRC_F4_PERM>(acc, s.src4, s.perm, s.idx, s.d2, tgt, i, nt, lim);
    }
};
struct SimMetric {   // similarity step: the point metric's record and the kept sources' sum of squares; cut null: lim = max_d2 (packed triples)
    static constexpr int NC = NSUMS;
    static constexpr bool KEYS = false, F3 = true;
    const double* cut;
    double lim;
    SimMetric(double max_d2, const double* cut_) : cut(cut_), lim(max_d2) {}
    __device__ SimMetric(const PairbArgs& a, int p) : cut(&a.ts[p].cut), lim(0.0) {}
    __device__ void begin() { if (cut) lim = *cut; }   // tau of this pass (-1: no candidate), written by the selection
    template <int SRC>
    __device__ __forceinline__ void source(double (&acc)[NC], const PairSrc& s, const float* tgt, const float*, int64_t i, int64_t nt, float*) const {
        sim_point_source<SRC>(acc, s.src3, s.src4, s.perm, s.idx, s.d2, tgt, i, nt, lim);
    }
};
// the scale of a robust pass: the pair's RobustScale and where its selection left the median key
struct RobustPass {
    RobustScale rs;
    const TrimState* sel = nullptr;
    RobustArg ra;
    __host__ __device__ RobustPass() {}
    __host__ __device__ RobustPass(const RobustScale& rs_, const TrimState* sel_) : rs(rs_), sel(sel_) {}
    __device__ RobustPass(const PairbArgs& a, int p) : rs(a.rs[p]), sel(a.ts + p) {}
    __device__ void begin(bool plane) { ra.loss = rs.loss; ra.c2 = robust_pass_c2(rs, plane, sel); }
};
template <int MODE>
struct PlaneRobustMetric {   // plane metric weighted (PAIR_ROBUST) or its keys |r| (PAIR_KEY)
    static constexpr int NC = P2L_NSUMS;
    static constexpr bool KEYS = MODE == PAIR_KEY, F3 = true;
    RobustPass rp;
    PlaneRobustMetric() {}
    PlaneRobustMetric(const RobustScale& rs, const TrimState* sel) : rp(rs, sel) {}
    __device__ PlaneRobustMetric(const PairbArgs& a, int p) : rp(a, p) {}
    __device__ void begin() { if constexpr (!KEYS) rp.begin(true); }
    template <int SRC>
    __device__ __forceinline__ void source(double (&acc)[NC], const PairSrc& s, const float* tgt, const float* nrm, int64_t i, int64_t nt, float* key) const {
        RobustArg ra = rp.ra;
        ra.key = key;
        p2l_source<SRC, true, MODE>(acc, s.src3, s.src4, s.perm, s.idx, s.d2, tgt, nrm, i, nt, s.max_d2, ra);
    }
};
template <int MODE>
struct PointRobustMetric {   // point metric weighted, or its keys d2 (packed float triples: kss_robust_sums; the loops select over the NN pass's d2)
    static constexpr int NC = NSUMS;
    static constexpr bool KEYS = MODE == PAIR_KEY, F3 = true;
    RobustPass rp;
    PointRobustMetric() {}
    PointRobustMetric(const RobustScale& rs, const TrimState* sel) : rp(rs, sel) {}
    __device__ PointRobustMetric(const PairbArgs& a, int p) : rp(a, p) {}
    __device__ void begin() { if constexpr (!KEYS) rp.begin(false); }
    template <int SRC>
    __device__ __forceinline__ void source(double (&acc)[NC], const PairSrc& s, const float* tgt, const float*, int64_t i, int64_t nt, float* key) const {
        RobustArg ra = rp.ra;
        ra.key = key;
        trim_point_source<SRC == SRC_F4_PERM, MODE, SRC == SRC_F3>(acc, s.src4, s.perm, s.idx, s.d2, tgt, i, nt, s.max_d2, s.src3, ra);
    }
};
struct GicpMetric {   // generalized: the rotation applied to the source normals and e = 1 - epsilon
    static constexpr int NC = P2L_NSUMS;
    static constexpr bool KEYS = false, F3 = true;
    GicpRot Rn;
    double e;
    GicpMetric(const GicpRot& Rn_, double e_) : Rn(Rn_), e(e_) {}
    __device__ GicpMetric(const PairbArgs& a, int p) {   // pass[p] is the same for every lane of the workgroup: one uniform load
        const PairPass pp = a.pass[p];
#pragma unroll
        for (int k = 0; k < 9; ++k) Rn.r[k] = pp.r[k];
        e = pp.e;
    }
    __device__ void begin() {}
    template <int SRC>
    __device__ __forceinline__ void source(double (&acc)[NC], const PairSrc& s, const float* tgt, const float* nrm, int64_t i, int64_t nt, float*) const {
        gicp_source<SRC>(acc, s.src3, s.src4, s.perm, s.idx, s.d2, s.sn, tgt, nrm, i, nt, s.max_d2, Rn, e);
    }
};
template <bool NEIGH>
struct VgicpNb { static constexpr int nb = 1; };          // the map's neighbourhood setting: a member only where it is read
template <>
struct VgicpNb<true> { int nb = 7; };
template <bool MOVE, bool NEIGH = false>
struct VgicpMetric : VgicpNb<NEIGH> {   // voxelized generalized: the map, GicpMetric's rotation and e, and (MOVE) the step the sources take on the way in
    static constexpr int NC = P2L_NSUMS;
    static constexpr bool KEYS = false, F3 = true;
    VmapDev v;
    VmapMove T;
    const float* in;   // packed float triples by original index: the positions before the move
    float* out;        // MOVE: where the moved positions go (not `in`)
    GicpRot Rn;
    double e;
    VgicpMetric(const VmapDev& v_, const VmapMove& T_, const float* in_, float* out_, const GicpRot& Rn_, double e_)
        : v(v_), T(T_), in(in_), out(out_), Rn(Rn_), e(e_) {}
    __device__ VgicpMetric(const VgicpbArgs& a, const VgicpbPass& pp) : v(a.v), in(a.in), out(a.out), e(pp.e) {   // (pp: the scan's entry, uniform)
#pragma unroll
        for (int k = 0; k < 12; ++k) T.m[k] = pp.t[k];
#pragma unroll
        for (int k = 0; k < 9; ++k) Rn.r[k] = pp.r[k];
        if constexpr (NEIGH) this->nb = a.nb;
    }
    __device__ void begin() {}
    template <int SRC>
    __device__ __forceinline__ void source(double (&acc)[NC], const PairSrc& s, const float*, const float*, int64_t i, int64_t, float*) const {
        static_assert(SRC == SRC_F3, "the voxel lookup reads packed float triples");
        vgicp_source<MOVE, NEIGH>(acc, in, out, s.sn, v, T, i, s.max_d2, Rn, e, this->nb);
    }
};
template <int MODE>
struct SymmMetric {   // symmetric: that rotation and align_normals; unweighted, weighted, or the weighted form's keys |r|
    static constexpr int NC = P2L_NSUMS;
    static constexpr bool KEYS = MODE == PAIR_KEY, F3 = true;
    GicpRot Rn;
    int align;
    RobustPass rp;
    SymmMetric(const GicpRot& Rn_, int align_) : Rn(Rn_), align(align_) {}
    SymmMetric(const GicpRot& Rn_, int align_, const RobustScale& rs, const TrimState* sel) : Rn(Rn_), align(align_), rp(rs, sel) {}
    __device__ SymmMetric(const PairbArgs& a, int p) {
        const PairPass pp = a.pass[p];
#pragma unroll
        for (int k = 0; k < 9; ++k) Rn.r[k] = pp.r[k];
        align = pp.align;
        if constexpr (MODE == PAIR_ROBUST) rp = RobustPass(a, p);
    }
    __device__ void begin() { if constexpr (MODE == PAIR_ROBUST) rp.begin(true); }
    template <int SRC>
    __device__ __forceinline__ void source(double (&acc)[NC], const PairSrc& s, const float* tgt, const float* nrm, int64_t i, int64_t nt, float* key) const {
        RobustArg ra = rp.ra;
        ra.key = key;
        symm_source<SRC, MODE>(acc, s.src3, s.src4, s.perm, s.idx, s.d2, s.sn, tgt, nrm, i, nt, s.max_d2, Rn, align, ra);
    }
};

// The walk: this lane's sources base + first, base + first + step, ... below base + n against the target tgt / nrm of nt points.
// Rows metric: the accumulators from zero, block_sum, row blockIdx.x of rows.  Keys metric: keys[source] = its key, preset to the
// quiet NaN (no candidate); no accumulator is read and nothing is summed.  Needs blockDim.x == P2L_THREADS.
template <class M, int SRC>
__device__ __forceinline__ void pair_walk(const M& m, const PairSrc& s, const float* tgt, const float* nrm, int64_t base, int64_t first, int64_t n,
                                          int64_t step, int64_t nt, double* __restrict__ rows, float* __restrict__ keys) {
    constexpr int NC = M::NC;
    double acc[NC];
    if constexpr (M::KEYS) {
        for (int64_t i = first; i < n; i += step) {
            float key = __uint_as_float(0x7fc00000u);
            m.template source<SRC>(acc, s, tgt, nrm, base + i, nt, &key);
            keys[base + i] = key;
        }
    } else {
        __shared__ double sh[P2L_THREADS / 64][NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) acc[c] = 0.0;
        for (int64_t i = first; i < n; i += step) m.template source<SRC>(acc, s, tgt, nrm, base + i, nt, nullptr);
        const double r = block_sum<NC>(acc, sh);
        if (threadIdx.x < NC) rows[(int64_t)blockIdx.x * NC + threadIdx.x] = r;
    }
}

}  // namespace kss
