// Scene-level bundle adjustment (CosyPose stage 3) and the reprojected symmetric distance it aligns with.
// Reference: cosypose/multiview/bundle_adjustment.py:164-222, lib3d/symmetric_distances.py:94-121, lib3d/camera_geometry.py:4-15,
// lib3d/transform_ops.py:54-64, lib3d/rotations.py:6-21.
//
// The reference gets the Jacobian of the reprojections by replicating every parameter once per residual and calling autograd, forms the
// dense (residuals x n) matrix and inverts J^T J + lambda I on the CPU.  Here every residual (candidate, point, x|y) depends on 18
// parameters only (the 9-D pose of its object and of its view), so:
//   align      one workgroup per candidate: TCO = TCW[view] TWO[obj] from the 9-D states, best symmetry of the candidate against it
//   linearise  one workgroup per candidate: analytic Jacobian rows, errors, and the candidate's 18x18 block of J^T J and 18 of J^T e
//   accumulate one workgroup per 9x9 block of A: the candidates of that (object, view) pair summed IN CANDIDATE ORDER (no atomics)
//   solve      one workgroup: Cholesky of A + lambda I (symmetric positive definite for lambda > 0), two triangular solves
// All of the bundle adjustment is float64 (DESIGN.md "Bundle adjustment": the problem is too ill-conditioned for float32); contraction
// is off so that a value does not depend on which multiply-adds the compiler chose to fuse.  Every sum runs in a fixed order: two runs
// on the same inputs give the same bits.
#include <stdlib.h>
#include <string.h>

#include "cosy_common.h"
#include "reduce_device.h"

#pragma clang fp contract(off)

namespace cosy {

namespace {

constexpr int BA_ROWS = 256;         // residual rows staged in LDS per pass = threads of a linearise workgroup
constexpr int BA_W = 19;             // 9 object derivatives, 9 view derivatives, the error
constexpr int BA_TRI = 171;          // upper triangle of the 18x18 block
constexpr int BA_BLK = BA_TRI + 18;  // + J^T e
constexpr int BA_MAX_N = 1152;       // 9 * (objects + views <= 128)
constexpr int BA_SOLVE_THREADS = 1024;

template <typename T> __device__ __forceinline__ T t_sqrt(T v);
template <> __device__ __forceinline__ float t_sqrt<float>(float v) { return sqrtf(v); }
template <> __device__ __forceinline__ double t_sqrt<double>(double v) { return sqrt(v); }

template <typename T>
__device__ __forceinline__ void mat4_mul(const T* A, const T* B, T* C) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            T acc = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) acc += A[i * 4 + k] * B[k * 4 + j];
            C[i * 4 + j] = acc;
        }
}

// P = K @ T[:3]  (3x4), camera_geometry.py:12
template <typename T>
__device__ __forceinline__ void proj_matrix(const T* K, const T* M, T* Pm) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) Pm[i * 4 + j] = (K[i * 3] * M[j] + K[i * 3 + 1] * M[4 + j]) + K[i * 3 + 2] * M[8 + j];
}

// project_points: no z clamp
template <typename T>
__device__ __forceinline__ void project(const T* Pm, T x, T y, T z, T& u, T& v) {
    const T s0 = ((Pm[0] * x + Pm[1] * y) + Pm[2] * z) + Pm[3];
    const T s1 = ((Pm[4] * x + Pm[5] * y) + Pm[6] * z) + Pm[7];
    const T s2 = ((Pm[8] * x + Pm[9] * y) + Pm[10] * z) + Pm[11];
    u = s0 / s2; v = s1 / s2;
}

// Over the ns symmetries S_k of the object: mean over its P points of |project(K, t1 S_k, p) - project(K, t2, p)| in pixels; strict <,
// first wins.  Called by all 256 threads of the workgroup; every thread returns the same index and distance.
template <typename T>
__device__ int reprojected_best_symmetry(const T* t1, const T* t2, const T* K, const T* __restrict__ p, const T* __restrict__ sym, int ns,
                                         int P, T* red, T& best_d) {
    T P2[12];
    proj_matrix(K, t2, P2);
    int best = -1;
    best_d = 0;
    for (int s = 0; s < ns; ++s) {
        T sm[16], M[16], P1[12];
#pragma unroll
        for (int i = 0; i < 16; ++i) sm[i] = sym[(size_t)s * 16 + i];
        mat4_mul(t1, sm, M);
        proj_matrix(K, M, P1);
        T acc = 0;
        for (int i = threadIdx.x; i < P; i += 256) {
            const T x = p[i * 3], y = p[i * 3 + 1], z = p[i * 3 + 2];
            T u1, v1, u2, v2;
            project(P1, x, y, z, u1, v1);
            project(P2, x, y, z, u2, v2);
            const T du = u1 - u2, dv = v1 - v2;
            acc += t_sqrt(du * du + dv * dv);
        }
        const T d = block_sum256(acc, red) / (T)P;
        if (best < 0 || d < best_d) { best = s; best_d = d; }
    }
    return best;
}

__global__ __launch_bounds__(256) void symmetric_distance_reprojected_kernel(const float* __restrict__ T1, const float* __restrict__ T2,
                                                                             const float* __restrict__ K, const int* __restrict__ obj,
                                                                             const float* __restrict__ pts, const float* __restrict__ sym,
                                                                             const int* __restrict__ n_sym, int n_obj, int P, int S,
                                                                             float* __restrict__ min_dists, int* __restrict__ best_sym,
                                                                             float* __restrict__ S12) {
    __shared__ float red[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int o = obj ? obj[b] : b;
    // an object id outside the tables, or an object without a symmetry (the identity counts as one): nothing is read out of bounds and
    // the item is marked -- distance NaN, index -1, S12 zero -- instead of being left unwritten
    if (o < 0 || o >= n_obj || (n_sym && n_sym[o] <= 0)) {
        if (tid == 0) { min_dists[b] = __builtin_nanf(""); best_sym[b] = -1; }
        if (tid < 16) S12[(size_t)b * 16 + tid] = 0.f;
        return;
    }
    float t1[16], t2[16], k[9];
#pragma unroll
    for (int i = 0; i < 16; ++i) { t1[i] = T1[(size_t)b * 16 + i]; t2[i] = T2[(size_t)b * 16 + i]; }
#pragma unroll
    for (int i = 0; i < 9; ++i) k[i] = K[(size_t)b * 9 + i];
    const int ns = n_sym ? min(n_sym[o], S) : S;
    float d;
    const int best = reprojected_best_symmetry<float>(t1, t2, k, pts + (size_t)o * P * 3, sym + (size_t)o * S * 16, ns, P, red, d);
    if (tid == 0) { min_dists[b] = d; best_sym[b] = best; }
    if (tid < 16 && best >= 0) S12[(size_t)b * 16 + tid] = sym[((size_t)o * S + best) * 16 + tid];
}

__device__ __forceinline__ void cross3(const double* a, const double* b, double* c) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// compute_transform_from_pose9d: R = [x y z] (columns) from ortho6d (x = a1/|a1|, z = (x X a2)/|.|, y = z X x), t = a[6:9]
__device__ __forceinline__ void pose9d_to_T(const double* a, double* T) {
    const double n = sqrt(dot3(a, a));
    const double x[3] = {a[0] / n, a[1] / n, a[2] / n};
    double z[3], y[3];
    cross3(x, a + 3, z);
    const double nz = sqrt(dot3(z, z));
    z[0] /= nz; z[1] /= nz; z[2] /= nz;
    cross3(z, x, y);
#pragma unroll
    for (int i = 0; i < 3; ++i) { T[i * 4] = x[i]; T[i * 4 + 1] = y[i]; T[i * 4 + 2] = z[i]; T[i * 4 + 3] = a[6 + i]; }
    T[12] = 0.; T[13] = 0.; T[14] = 0.; T[15] = 1.;
}

// dR/da_k (row-major 3x3) of the ortho6d rotation, k = 0..5, by the chain rule through normalise / cross / normalise / cross
__device__ void ortho6d_derivative(const double* a, int k, double* dR) {
    const double n = sqrt(dot3(a, a));
    const double x[3] = {a[0] / n, a[1] / n, a[2] / n};
    double da1[3] = {0., 0., 0.}, da2[3] = {0., 0., 0.};
    if (k < 3) da1[k] = 1.; else da2[k - 3] = 1.;
    const double xd = dot3(x, da1);
    const double dx[3] = {(da1[0] - x[0] * xd) / n, (da1[1] - x[1] * xd) / n, (da1[2] - x[2] * xd) / n};
    double c[3], z[3], t0[3], t1[3], dc[3];
    cross3(x, a + 3, c);
    const double nc = sqrt(dot3(c, c));
    z[0] = c[0] / nc; z[1] = c[1] / nc; z[2] = c[2] / nc;
    cross3(dx, a + 3, t0);
    cross3(x, da2, t1);
    dc[0] = t0[0] + t1[0]; dc[1] = t0[1] + t1[1]; dc[2] = t0[2] + t1[2];
    const double zd = dot3(z, dc);
    const double dz[3] = {(dc[0] - z[0] * zd) / nc, (dc[1] - z[1] * zd) / nc, (dc[2] - z[2] * zd) / nc};
    cross3(dz, x, t0);
    cross3(z, dx, t1);
#pragma unroll
    for (int i = 0; i < 3; ++i) { dR[i * 3] = dx[i]; dR[i * 3 + 1] = t0[i] + t1[i]; dR[i * 3 + 2] = dz[i]; }
}

// ids: cand_obj (n_cand) | cand_view (n_cand) | cand_mesh (n_cand) | obj_mesh (n_obj), validated by cosy_ba_upload_ids.  A candidate
// whose ids are nevertheless outside their tables is skipped (nothing read or written out of bounds).
__device__ __forceinline__ bool cand_ids(const int* __restrict__ ids, int c, int n_cand, int n_obj, int n_views, int n_mesh, int& o, int& v,
                                         int& m_cand, int& m_obj) {
    o = ids[c]; v = ids[n_cand + c]; m_cand = ids[2 * n_cand + c];
    if (o < 0 || o >= n_obj || v < 0 || v >= n_views || m_cand < 0 || m_cand >= n_mesh) return false;
    m_obj = ids[3 * n_cand + o];
    return m_obj >= 0 && m_obj < n_mesh;
}

// The alignment of candidate c (object row o, view row v, mesh m; all checked by the caller), shared by the single-problem and the
// batched kernel so that both compute the same bits.  dists / best_sym may be null.
__device__ __forceinline__ void ba_align_body(const double* __restrict__ TWO_9d, const double* __restrict__ TCW_9d,
                                              const double* __restrict__ cand_TCO, const double* __restrict__ K,
                                              const double* __restrict__ pts, const double* __restrict__ sym,
                                              const int* __restrict__ n_sym, int c, int o, int v, int m, int P, int S,
                                              double* __restrict__ dists, int* __restrict__ best_sym, double* __restrict__ aligned,
                                              double* red) {
    const int tid = threadIdx.x;
    double a[9], Two[16], Tcw[16], Tco[16], t1[16], k[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) a[i] = TWO_9d[(size_t)o * 9 + i];
    pose9d_to_T(a, Two);
#pragma unroll
    for (int i = 0; i < 9; ++i) a[i] = TCW_9d[(size_t)v * 9 + i];
    pose9d_to_T(a, Tcw);
    mat4_mul(Tcw, Two, Tco);
#pragma unroll
    for (int i = 0; i < 16; ++i) t1[i] = cand_TCO[(size_t)c * 16 + i];
#pragma unroll
    for (int i = 0; i < 9; ++i) k[i] = K[(size_t)v * 9 + i];
    const int ns = min(n_sym[m], S);
    if (ns <= 0) {   // a mesh without a symmetry (the identity counts as one): marked with NaNs, which the loss then shows
        if (tid == 0) {
            if (dists) dists[c] = __builtin_nan("");
            if (best_sym) best_sym[c] = -1;
        }
        if (tid < 16) aligned[(size_t)c * 16 + tid] = __builtin_nan("");
        return;
    }
    double d;
    const double* sm = sym + (size_t)m * S * 16;
    const int best = reprojected_best_symmetry<double>(t1, Tco, k, pts + (size_t)m * P * 3, sm, ns, P, red, d);
    if (tid == 0) {
        if (dists) dists[c] = d;
        if (best_sym) best_sym[c] = best;
    }
    if (tid < 16 && best >= 0) {   // TCO_cand_aligned = cand_TCO @ S
        const int i = tid >> 2, j = tid & 3;
        double acc = 0.;
#pragma unroll
        for (int q = 0; q < 4; ++q) acc += t1[i * 4 + q] * sm[(size_t)best * 16 + q * 4 + j];
        aligned[(size_t)c * 16 + tid] = acc;
    }
}

__global__ __launch_bounds__(256) void ba_align_kernel(const double* __restrict__ TWO_9d, const double* __restrict__ TCW_9d,
                                                       const double* __restrict__ cand_TCO, const double* __restrict__ K,
                                                       const int* __restrict__ ids, const double* __restrict__ pts,
                                                       const double* __restrict__ sym, const int* __restrict__ n_sym, int n_cand, int n_obj,
                                                       int n_views, int n_mesh, int P, int S, double* __restrict__ dists,
                                                       int* __restrict__ best_sym, double* __restrict__ aligned) {
    __shared__ double red[4];
    const int c = blockIdx.x;
    int o, v, m, mo;
    if (!cand_ids(ids, c, n_cand, n_obj, n_views, n_mesh, o, v, m, mo)) return;
    ba_align_body(TWO_9d, TCW_9d, cand_TCO, K, pts, sym, n_sym, c, o, v, m, P, S, dists, best_sym, aligned, red);
}

// One workgroup per candidate.  Thread t of a pass owns residual row r = pass*256 + t: point r/2, coordinate r%2 (the reference's order,
// bundle_adjustment.py:93-110).  The rows of a pass are staged in LDS, then thread t < 189 adds the pass' contribution to its entry of
// the upper triangle of J_c^T J_c (171) or of J_c^T e_c (18), rows in order.
// The body is shared by the single-problem and the batched kernel (the same bits from both); `ok` = the candidate's ids are inside
// their tables (o, v: object and view row, mo: the object's mesh).  errors, J_obj, J_view may be null.  rows: BA_ROWS * BA_W doubles of
// LDS, dRo / dRc: 54 each, red: 4.
__device__ __forceinline__ void ba_linearize_body(const double* __restrict__ TWO_9d, const double* __restrict__ TCW_9d,
                                                  const double* __restrict__ aligned, const double* __restrict__ K,
                                                  const double* __restrict__ pts, bool ok, int c, int o, int v, int mo, int P,
                                                  double threshold, double* __restrict__ errors, double* __restrict__ J_obj,
                                                  double* __restrict__ J_view, double* __restrict__ blk, double* __restrict__ loss_part,
                                                  double* rows, double* dRo, double* dRc, double* red) {
    const int tid = threadIdx.x;
    // entry of the block this thread sums
    int ei = 0, ej = 18;
    if (tid < BA_TRI) {
        int rem = tid;
        while (rem >= 18 - ei) { rem -= 18 - ei; ++ei; }
        ej = ei + rem;
    } else if (tid < BA_BLK) {
        ei = tid - BA_TRI;
    }
    if (!ok) {   // uniform over the workgroup
        if (tid < BA_BLK) blk[(size_t)c * BA_BLK + tid] = 0.;
        if (tid == 0) loss_part[c] = 0.;
        return;
    }
    double ao[9], ac[9], Two[16], Tcw[16], Tca[16], k[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) { ao[i] = TWO_9d[(size_t)o * 9 + i]; ac[i] = TCW_9d[(size_t)v * 9 + i]; k[i] = K[(size_t)v * 9 + i]; }
    pose9d_to_T(ao, Two);
    pose9d_to_T(ac, Tcw);
#pragma unroll
    for (int i = 0; i < 16; ++i) Tca[i] = aligned[(size_t)c * 16 + i];
    if (tid < 6) ortho6d_derivative(ao, tid, dRo + tid * 9);
    else if (tid < 12) ortho6d_derivative(ac, tid - 6, dRc + (tid - 6) * 9);
    double Pa[12];
    proj_matrix(k, Tca, Pa);
    const double* p = pts + (size_t)mo * P * 3;
    const int n_rows = 2 * P;
    double acc = 0., loss_acc = 0.;
    for (int base = 0; base < n_rows; base += BA_ROWS) {
        __syncthreads();   // dRo / dRc written; rows of the previous pass consumed
        const int r = base + tid;
        double* row = rows + tid * BA_W;
        if (r < n_rows) {
            const int xy = r & 1;
            const double px = p[(r >> 1) * 3], py = p[(r >> 1) * 3 + 1], pz = p[(r >> 1) * 3 + 2];
            const double pp[3] = {px, py, pz};
            double q[3], pc[3], s[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) q[i] = ((Two[i * 4] * px + Two[i * 4 + 1] * py) + Two[i * 4 + 2] * pz) + Two[i * 4 + 3];
#pragma unroll
            for (int i = 0; i < 3; ++i) pc[i] = ((Tcw[i * 4] * q[0] + Tcw[i * 4 + 1] * q[1]) + Tcw[i * 4 + 2] * q[2]) + Tcw[i * 4 + 3];
#pragma unroll
            for (int i = 0; i < 3; ++i) s[i] = (k[i * 3] * pc[0] + k[i * 3 + 1] * pc[1]) + k[i * 3 + 2] * pc[2];
            const double yhat = s[xy] / s[2];
            double u, w;
            project(Pa, px, py, pz, u, w);
            const double e = (xy ? w : u) - yhat;
            // d yhat / d pc, then through TCW to the world point q
            double g[3], gw[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) g[i] = (k[xy * 3 + i] - yhat * k[6 + i]) / s[2];
#pragma unroll
            for (int i = 0; i < 3; ++i) gw[i] = (Tcw[i] * g[0] + Tcw[4 + i] * g[1]) + Tcw[8 + i] * g[2];
#pragma unroll
            for (int kk = 0; kk < 6; ++kk) {
                const double* d = dRo + kk * 9;
                double dq[3];
#pragma unroll
                for (int i = 0; i < 3; ++i) dq[i] = (d[i * 3] * pp[0] + d[i * 3 + 1] * pp[1]) + d[i * 3 + 2] * pp[2];
                row[kk] = dot3(gw, dq);
                const double* dc = dRc + kk * 9;
#pragma unroll
                for (int i = 0; i < 3; ++i) dq[i] = (dc[i * 3] * q[0] + dc[i * 3 + 1] * q[1]) + dc[i * 3 + 2] * q[2];
                row[9 + kk] = dot3(g, dq);
            }
#pragma unroll
            for (int i = 0; i < 3; ++i) { row[6 + i] = gw[i]; row[15 + i] = g[i]; }
            row[18] = e;
            const size_t gr = (size_t)c * n_rows + r;
            if (errors) errors[gr] = e;
            if (J_obj)
#pragma unroll
                for (int i = 0; i < 9; ++i) J_obj[gr * 9 + i] = row[i];
            if (J_view)
#pragma unroll
                for (int i = 0; i < 9; ++i) J_view[gr * 9 + i] = row[9 + i];
            const double e2 = e * e;
            // torch.min(residuals, threshold): the clamp enters the loss only, and a NaN residual stays NaN (NaN > threshold is false)
            loss_acc += e2 > threshold ? threshold : e2;
        } else {
#pragma unroll
            for (int i = 0; i < BA_W; ++i) row[i] = 0.;
        }
        __syncthreads();
        if (tid < BA_BLK) {
            const int nr = min(BA_ROWS, n_rows - base);
            for (int rr = 0; rr < nr; ++rr) acc += rows[rr * BA_W + ei] * rows[rr * BA_W + ej];
        }
    }
    if (tid < BA_BLK) blk[(size_t)c * BA_BLK + tid] = acc;
    loss_acc = block_sum256(loss_acc, red);
    if (tid == 0) loss_part[c] = loss_acc;
}

__global__ __launch_bounds__(BA_ROWS) void ba_linearize_kernel(const double* __restrict__ TWO_9d, const double* __restrict__ TCW_9d,
                                                               const double* __restrict__ aligned, const double* __restrict__ K,
                                                               const int* __restrict__ ids, const double* __restrict__ pts, int n_cand,
                                                               int n_obj, int n_views, int n_mesh, int P, double threshold,
                                                               double* __restrict__ errors, double* __restrict__ J_obj,
                                                               double* __restrict__ J_view, double* __restrict__ blk,
                                                               double* __restrict__ loss_part) {
    __shared__ double rows[BA_ROWS * BA_W];
    __shared__ double dRo[6 * 9], dRc[6 * 9];
    __shared__ double red[4];
    const int c = blockIdx.x;
    int o, v, m, mo;
    const bool ok = cand_ids(ids, c, n_cand, n_obj, n_views, n_mesh, o, v, m, mo);
    ba_linearize_body(TWO_9d, TCW_9d, aligned, K, pts, ok, c, o, v, mo, P, threshold, errors, J_obj, J_view, blk, loss_part, rows, dRo, dRc,
                      red);
}

__device__ __forceinline__ int tri_index(int i, int j) {   // i <= j < 18
    return i * 18 - (i * (i - 1)) / 2 + (j - i);
}

// A (n,n) and b (n), n = 9 (n_obj + n_views), objects first: the workgroup of block (bi, bj) writes that 9x9 block -- zeros included, so A
// needs no clearing -- as the sum over the candidates c0 <= c < c1 of that block IN CANDIDATE ORDER; column 0's workgroups also write b,
// workgroup (0,0) the loss.  A candidate's object / view row is cand_obj[c] - o_base / cand_view[c] - v_base.  Shared by the
// single-problem and the batched kernel.
__device__ __forceinline__ void ba_accumulate_body(const double* __restrict__ blk, const double* __restrict__ loss_part,
                                                   const int* __restrict__ cand_obj, const int* __restrict__ cand_view, int c0, int c1,
                                                   int o_base, int v_base, int n_obj, int n_views, int P, int bi, int bj,
                                                   double* __restrict__ A, double* __restrict__ b, double* __restrict__ loss) {
    const int tid = threadIdx.x;
    const int n = 9 * (n_obj + n_views);
    const bool io = bi < n_obj, jo = bj < n_obj;
    const int r = tid / 9, cc = tid % 9;
    if (tid < 81) {
        double acc = 0.;
        if (io != jo || bi == bj) {
            const int want_o = io ? bi : (jo ? bj : -1), want_v = !io ? bi - n_obj : (!jo ? bj - n_obj : -1);
            int hi, hj;   // entry of the candidate's 18x18 block
            if (io && jo) { hi = r; hj = cc; }
            else if (!io && !jo) { hi = 9 + r; hj = 9 + cc; }
            else if (io) { hi = r; hj = 9 + cc; }
            else { hi = cc; hj = 9 + r; }
            const int e = hi <= hj ? tri_index(hi, hj) : tri_index(hj, hi);
            for (int c = c0; c < c1; ++c) {
                const int o = cand_obj[c] - o_base, v = cand_view[c] - v_base;
                if ((want_o < 0 || o == want_o) && (want_v < 0 || v == want_v)) acc += blk[(size_t)c * BA_BLK + e];
            }
        }
        A[(size_t)(bi * 9 + r) * n + bj * 9 + cc] = acc;
    }
    if (bj == 0 && tid >= 96 && tid < 105) {
        const int t = tid - 96;
        double acc = 0.;
        for (int c = c0; c < c1; ++c) {
            const int o = cand_obj[c] - o_base, v = cand_view[c] - v_base;
            if (io ? o == bi : v == bi - n_obj) acc += blk[(size_t)c * BA_BLK + BA_TRI + (io ? t : 9 + t)];
        }
        b[bi * 9 + t] = acc;
    }
    if (bi == 0 && bj == 0 && tid == 127) {
        double acc = 0.;
        for (int c = c0; c < c1; ++c) acc += loss_part[c];
        *loss = acc / ((double)(c1 - c0) * (double)(2 * P));
    }
}

__global__ __launch_bounds__(128) void ba_accumulate_kernel(const double* __restrict__ blk, const double* __restrict__ loss_part,
                                                            const int* __restrict__ ids, int n_cand, int n_obj, int n_views, int P,
                                                            double* __restrict__ A, double* __restrict__ b, double* __restrict__ loss) {
    ba_accumulate_body(blk, loss_part, ids, ids + n_cand, 0, n_cand, 0, 0, n_obj, n_views, P, blockIdx.y, blockIdx.x, A, b, loss);
}

// h = (A + lambda I)^-1 b: right-looking Cholesky of the lower triangle in `L` (n*n doubles of workspace), then L y = b, L^T h = y.
// One workgroup of BA_SOLVE_THREADS; column k (col), the right-hand side (vec) and the diagonal (dg) live in LDS, BA_MAX_N doubles
// each.  h is left in vec, visible to every thread on return.  A non-positive pivot gives NaNs in h (the caller's loss test rejects).
// Shared by the single-problem and the batched kernel.
__device__ __forceinline__ void ba_solve_body(const double* __restrict__ A, const double* __restrict__ b, int n, double lambda,
                                              double* __restrict__ L, double* col, double* vec, double* dg) {
    const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
    for (int i = ty; i < n; i += 32)
        for (int j = tx; j <= i; j += 32) L[(size_t)i * n + j] = A[(size_t)i * n + j] + (i == j ? lambda : 0.);
    for (int i = tid; i < n; i += BA_SOLVE_THREADS) vec[i] = b[i];
    __syncthreads();
    for (int k = 0; k < n; ++k) {
        const double d = sqrt(L[(size_t)k * n + k]);
        if (tid == 0) dg[k] = d;
        for (int i = k + 1 + tid; i < n; i += BA_SOLVE_THREADS) {
            const double v = L[(size_t)i * n + k] / d;
            L[(size_t)i * n + k] = v;
            col[i] = v;
        }
        __syncthreads();
        for (int i = k + 1 + ty; i < n; i += 32) {
            const double li = col[i];
            for (int j = k + 1 + tx; j <= i; j += 32) L[(size_t)i * n + j] -= li * col[j];
        }
        __syncthreads();
    }
    for (int k = 0; k < n; ++k) {          // L y = b
        if (tid == 0) vec[k] /= dg[k];
        __syncthreads();
        const double yk = vec[k];
        for (int i = k + 1 + tid; i < n; i += BA_SOLVE_THREADS) vec[i] -= L[(size_t)i * n + k] * yk;
        __syncthreads();
    }
    for (int k = n - 1; k >= 0; --k) {     // L^T h = y
        if (tid == 0) vec[k] /= dg[k];
        __syncthreads();
        const double hk = vec[k];
        for (int i = tid; i < k; i += BA_SOLVE_THREADS) vec[i] -= L[(size_t)k * n + i] * hk;
        __syncthreads();
    }
}

__global__ __launch_bounds__(BA_SOLVE_THREADS) void ba_solve_kernel(const double* __restrict__ A, const double* __restrict__ b, int n,
                                                                    double lambda, double* __restrict__ L, double* __restrict__ h) {
    __shared__ double col[BA_MAX_N], vec[BA_MAX_N], dg[BA_MAX_N];
    ba_solve_body(A, b, n, lambda, L, col, vec, dg);
    for (int i = threadIdx.x; i < n; i += BA_SOLVE_THREADS) h[i] = vec[i];
}

// ---- the batch: G problems through the same launches ------------------------------------------------------------------------------
// The device table written by cosy_ba_batch_upload: int32 cand_obj | cand_view | cand_mesh | cand_prob (n_cand each; object and view
// rows are GLOBAL) | obj_mesh (n_obj) | cand_off | obj_off | view_off (G+1 each), then, 8-byte aligned, A_off (G+1) int64.
struct BaTab {
    const int *cand_obj, *cand_view, *cand_mesh, *cand_prob, *obj_mesh, *cand_off, *obj_off, *view_off;
    const long long* A_off;
};

inline size_t ba_tab_ints(int G, int n_cand, int n_obj) {
    const size_t n = 4 * (size_t)n_cand + (size_t)n_obj + 3 * ((size_t)G + 1);
    return (n + 1) & ~(size_t)1;
}

inline BaTab ba_tab(const void* table, int G, int n_cand, int n_obj) {
    const int* t = (const int*)table;
    BaTab r;
    r.cand_obj = t;
    r.cand_view = t + (size_t)n_cand;
    r.cand_mesh = t + 2 * (size_t)n_cand;
    r.cand_prob = t + 3 * (size_t)n_cand;
    r.obj_mesh = t + 4 * (size_t)n_cand;
    r.cand_off = r.obj_mesh + (size_t)n_obj;
    r.obj_off = r.cand_off + ((size_t)G + 1);
    r.view_off = r.obj_off + ((size_t)G + 1);
    r.A_off = (const long long*)(t + ba_tab_ints(G, n_cand, n_obj));
    return r;
}

// candidate c of the batch: its object / view row inside ITS problem's rows, its meshes inside the table (cosy_ba_batch_upload checked
// them; a candidate that is outside nevertheless is skipped as in the single problem)
__device__ __forceinline__ bool ba_batch_cand_ids(const BaTab& t, int c, int g, int n_mesh, int& o, int& v, int& m, int& mo) {
    o = t.cand_obj[c]; v = t.cand_view[c]; m = t.cand_mesh[c];
    if (o < t.obj_off[g] || o >= t.obj_off[g + 1] || v < t.view_off[g] || v >= t.view_off[g + 1] || m < 0 || m >= n_mesh) return false;
    mo = t.obj_mesh[o];
    return mo >= 0 && mo < n_mesh;
}

// does problem g take part in this linearisation?  which = 0: the current state, not needed after an accepted step
__device__ __forceinline__ bool ba_batch_idle(const cosy_ba_ctrl_t* __restrict__ ctrl, int g, int which) {
    return ctrl[g].finished || (which == 0 && ctrl[g].prev_update);
}

__global__ __launch_bounds__(256) void ba_batch_align_kernel(BaTab t, const cosy_ba_ctrl_t* __restrict__ ctrl, int which, int G,
                                                             const double* __restrict__ TWO_9d, const double* __restrict__ TCW_9d,
                                                             const double* __restrict__ cand_TCO, const double* __restrict__ K,
                                                             const double* __restrict__ pts, const double* __restrict__ sym,
                                                             const int* __restrict__ n_sym, int n_mesh, int P, int S,
                                                             double* __restrict__ aligned) {
    __shared__ double red[4];
    const int c = blockIdx.x;
    const int g = t.cand_prob[c];
    if (g < 0 || g >= G || ba_batch_idle(ctrl, g, which)) return;
    int o, v, m, mo;
    if (!ba_batch_cand_ids(t, c, g, n_mesh, o, v, m, mo)) return;
    ba_align_body(TWO_9d, TCW_9d, cand_TCO, K, pts, sym, n_sym, c, o, v, m, P, S, nullptr, nullptr, aligned, red);
}

__global__ __launch_bounds__(BA_ROWS) void ba_batch_linearize_kernel(BaTab t, const cosy_ba_ctrl_t* __restrict__ ctrl, int which, int G,
                                                                     const double* __restrict__ TWO_9d, const double* __restrict__ TCW_9d,
                                                                     const double* __restrict__ aligned, const double* __restrict__ K,
                                                                     const double* __restrict__ pts, int n_mesh, int P, double threshold,
                                                                     double* __restrict__ blk, double* __restrict__ loss_part) {
    __shared__ double rows[BA_ROWS * BA_W];
    __shared__ double dRo[6 * 9], dRc[6 * 9];
    __shared__ double red[4];
    const int c = blockIdx.x;
    const int g = t.cand_prob[c];
    if (g < 0 || g >= G || ba_batch_idle(ctrl, g, which)) return;
    int o, v, m, mo;
    const bool ok = ba_batch_cand_ids(t, c, g, n_mesh, o, v, m, mo);
    ba_linearize_body(TWO_9d, TCW_9d, aligned, K, pts, ok, c, o, v, mo, P, threshold, nullptr, nullptr, nullptr, blk, loss_part, rows, dRo,
                      dRc, red);
}

// grid (max_blocks^2, G): workgroup (x, g) owns block (x / blocks_g, x % blocks_g) of problem g's A
__global__ __launch_bounds__(128) void ba_batch_accumulate_kernel(BaTab t, cosy_ba_ctrl_t* __restrict__ ctrl, int which,
                                                                  const double* __restrict__ blk, const double* __restrict__ loss_part,
                                                                  int P, double* __restrict__ A, double* __restrict__ b) {
    const int g = blockIdx.y;
    if (ba_batch_idle(ctrl, g, which)) return;
    const int o0 = t.obj_off[g], v0 = t.view_off[g];
    const int no = t.obj_off[g + 1] - o0, nv = t.view_off[g + 1] - v0, nb = no + nv;
    if ((int)blockIdx.x >= nb * nb) return;
    const int bi = blockIdx.x / nb, bj = blockIdx.x % nb;
    ba_accumulate_body(blk, loss_part, t.cand_obj, t.cand_view, t.cand_off[g], t.cand_off[g + 1], o0, v0, no, nv, P, bi, bj,
                       A + (size_t)t.A_off[g], b + 9 * ((size_t)o0 + (size_t)v0), which ? &ctrl[g].next_loss : &ctrl[g].loss);
}

__global__ __launch_bounds__(BA_SOLVE_THREADS) void ba_batch_solve_step_kernel(BaTab t, const cosy_ba_ctrl_t* __restrict__ ctrl,
                                                                               const double* __restrict__ A, const double* __restrict__ b,
                                                                               double* __restrict__ L, const double* __restrict__ TWO_9d,
                                                                               const double* __restrict__ TCW_9d,
                                                                               double* __restrict__ TWO_9d_updated,
                                                                               double* __restrict__ TCW_9d_updated, int optimize_cameras) {
    __shared__ double col[BA_MAX_N], vec[BA_MAX_N], dg[BA_MAX_N];
    const int g = blockIdx.x;
    if (ctrl[g].finished) return;
    const int o0 = t.obj_off[g], v0 = t.view_off[g];
    const int no = t.obj_off[g + 1] - o0, nv = t.view_off[g + 1] - v0;
    const int n = 9 * (no + nv);
    if (n > BA_MAX_N) return;
    const size_t a0 = (size_t)t.A_off[g];
    ba_solve_body(A + a0, b + 9 * ((size_t)o0 + (size_t)v0), n, ctrl[g].lambda, L + a0, col, vec, dg);
    const size_t po = 9 * (size_t)o0, pv = 9 * (size_t)v0;
    for (int i = threadIdx.x; i < n; i += BA_SOLVE_THREADS) {
        if (i < 9 * no) {
            TWO_9d_updated[po + i] = TWO_9d[po + i] + vec[i];
        } else {
            const int j = i - 9 * no;
            TCW_9d_updated[pv + j] = optimize_cameras ? TCW_9d[pv + j] + vec[i] : TCW_9d[pv + j];
        }
    }
}

__global__ __launch_bounds__(256) void ba_batch_record_kernel(BaTab t, cosy_ba_ctrl_t* __restrict__ ctrl, int iteration, int n_hist_rows,
                                                              int n_obj, int n_views, const double* __restrict__ TWO_9d,
                                                              const double* __restrict__ TCW_9d, int* __restrict__ hist_iteration,
                                                              double* __restrict__ hist_lambda, double* __restrict__ hist_loss,
                                                              double* __restrict__ hist_TWO_9d, double* __restrict__ hist_TCW_9d) {
    const int g = blockIdx.x, tid = threadIdx.x;
    const cosy_ba_ctrl_t r = ctrl[g];
    if (r.finished) return;    // uniform: the record is written below, after every thread has read it
    __syncthreads();
    const int k = r.n_hist;
    if (k < 0 || k >= n_hist_rows) return;
    if (hist_TWO_9d) {
        const size_t o0 = 9 * (size_t)t.obj_off[g], v0 = 9 * (size_t)t.view_off[g];
        const int no = 9 * (t.obj_off[g + 1] - t.obj_off[g]), nv = 9 * (t.view_off[g + 1] - t.view_off[g]);
        double* ho = hist_TWO_9d + (size_t)k * n_obj * 9 + o0;
        double* hv = hist_TCW_9d + (size_t)k * n_views * 9 + v0;
        for (int i = tid; i < no; i += 256) ho[i] = TWO_9d[o0 + i];
        for (int i = tid; i < nv; i += 256) hv[i] = TCW_9d[v0 + i];
    }
    if (tid == 0) {
        const size_t row = (size_t)g * n_hist_rows + k;
        hist_iteration[row] = iteration;
        hist_lambda[row] = r.lambda;
        hist_loss[row] = r.loss;
        ctrl[g].n_hist = k + 1;
        if (r.done) ctrl[g].finished = 1;
    }
}

// the reference's comparisons in the reference's order (bundle_adjustment.py:263-276 there): a NaN rho fails both and is rejected
__global__ __launch_bounds__(256) void ba_batch_decide_kernel(BaTab t, cosy_ba_ctrl_t* __restrict__ ctrl, double L_down, double L_up,
                                                              double eps, double* __restrict__ TWO_9d, double* __restrict__ TCW_9d,
                                                              const double* __restrict__ TWO_9d_updated,
                                                              const double* __restrict__ TCW_9d_updated) {
    const int g = blockIdx.x, tid = threadIdx.x;
    const cosy_ba_ctrl_t r = ctrl[g];
    if (r.finished) return;    // uniform, as in the record kernel
    __syncthreads();
    const double rho = r.loss - r.next_loss;
    if (fabs(rho) < eps) {
        if (tid == 0) ctrl[g].done = 1;
    } else if (rho > eps) {
        if (TWO_9d) {
            const size_t o0 = 9 * (size_t)t.obj_off[g], v0 = 9 * (size_t)t.view_off[g];
            const int no = 9 * (t.obj_off[g + 1] - t.obj_off[g]), nv = 9 * (t.view_off[g + 1] - t.view_off[g]);
            for (int i = tid; i < no; i += 256) TWO_9d[o0 + i] = TWO_9d_updated[o0 + i];
            for (int i = tid; i < nv; i += 256) TCW_9d[v0 + i] = TCW_9d_updated[v0 + i];
        }
        if (tid == 0) {
            const double l = r.lambda / L_down;
            ctrl[g].loss = r.next_loss;
            ctrl[g].lambda = 1e-7 > l ? 1e-7 : l;      // max(lambda / L_down, 1e-7)
            ctrl[g].prev_update = 1;
        }
    } else {
        if (tid == 0) {
            const double l = r.lambda * L_up;
            ctrl[g].lambda = 1e7 < l ? 1e7 : l;        // min(lambda * L_up, 1e7)
            ctrl[g].prev_update = 0;
        }
    }
}

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace

}  // namespace cosy

using namespace cosy;

extern "C" {

int cosy_symmetric_distance_reprojected(const float* T1, const float* T2, const float* K, const int* obj_id, const float* pts_table,
                                        const float* sym_table, const int* n_sym, int B, int n_obj, int P, int S, float* min_dists,
                                        int* best_sym, float* S12, cosy_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    COSY_REQUIRE(B >= 0 && P > 0 && S > 0, "cosy_symmetric_distance_reprojected: B=%d P=%d S=%d", B, P, S);
    if (B == 0) return COSY_OK;
    COSY_REQUIRE(n_obj > 0 && (obj_id || n_obj >= B), "cosy_symmetric_distance_reprojected: n_obj=%d table rows for B=%d%s", n_obj, B,
                 obj_id ? "" : " per-sample items");
    COSY_REQUIRE(T1 && T2 && K && pts_table && sym_table && min_dists && best_sym && S12, "cosy_symmetric_distance_reprojected: null pointer");
    hipLaunchKernelGGL(symmetric_distance_reprojected_kernel, dim3(B), dim3(256), 0, s, T1, T2, K, obj_id, pts_table, sym_table, n_sym, n_obj, P,
                       S, min_dists, best_sym, S12);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

#define BA_REQUIRE_SIZES(name)                                                                                                       \
    do {                                                                                                                             \
        COSY_REQUIRE(n_cand > 0 && P > 0 && n_obj > 0 && n_views > 0, name ": n_cand=%d P=%d n_obj=%d n_views=%d", n_cand, P, n_obj, \
                     n_views);                                                                                                       \
        if (n_obj + n_views > BA_MAX_N / 9) {                                                                                        \
            cosy::set_error(name ": n_obj + n_views = %d > %d", n_obj + n_views, BA_MAX_N / 9);                                      \
            return COSY_ESIZE;                                                                                                       \
        }                                                                                                                            \
    } while (0)

size_t cosy_ba_workspace_bytes(int n_cand, int P, int n_obj, int n_views) {
    if (n_cand <= 0 || P <= 0 || n_obj <= 0 || n_views <= 0 || n_obj + n_views > BA_MAX_N / 9) return 0;
    // cosy_ba_linearize: the candidates' blocks and loss parts; cosy_ba_solve: the factor L (n*n), ON TOP of them -- the blocks are
    // consumed by the accumulation before a solve can run in stream order
    const size_t n = 9 * (size_t)(n_obj + n_views);
    const size_t lin = align256((size_t)n_cand * BA_BLK * sizeof(double)) + align256((size_t)n_cand * sizeof(double));
    const size_t sol = align256(n * n * sizeof(double));
    return lin > sol ? lin : sol;
}

int cosy_ba_upload_ids(const int* host_cand_obj, const int* host_cand_view, const int* host_cand_mesh, const int* host_obj_mesh, int n_cand,
                       int n_obj, int n_views, int n_mesh, int* ids, cosy_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    COSY_REQUIRE(n_cand > 0 && n_obj > 0 && n_views > 0 && n_mesh > 0, "cosy_ba_upload_ids: n_cand=%d n_obj=%d n_views=%d n_mesh=%d", n_cand,
                 n_obj, n_views, n_mesh);
    COSY_REQUIRE(host_cand_obj && host_cand_view && host_cand_mesh && host_obj_mesh && ids, "cosy_ba_upload_ids: null pointer");
    for (int c = 0; c < n_cand; ++c) {
        COSY_REQUIRE(host_cand_obj[c] >= 0 && host_cand_obj[c] < n_obj, "cosy_ba_upload_ids: candidate %d: object id %d outside [0, %d)", c,
                     host_cand_obj[c], n_obj);
        COSY_REQUIRE(host_cand_view[c] >= 0 && host_cand_view[c] < n_views, "cosy_ba_upload_ids: candidate %d: view id %d outside [0, %d)", c,
                     host_cand_view[c], n_views);
        COSY_REQUIRE(host_cand_mesh[c] >= 0 && host_cand_mesh[c] < n_mesh, "cosy_ba_upload_ids: candidate %d: mesh id %d outside [0, %d)", c,
                     host_cand_mesh[c], n_mesh);
    }
    for (int o = 0; o < n_obj; ++o)
        COSY_REQUIRE(host_obj_mesh[o] >= 0 && host_obj_mesh[o] < n_mesh, "cosy_ba_upload_ids: object %d: mesh id %d outside [0, %d)", o,
                     host_obj_mesh[o], n_mesh);
    const size_t nb = (size_t)n_cand * sizeof(int);
    COSY_CHECK_HIP(hipMemcpyAsync(ids, host_cand_obj, nb, hipMemcpyHostToDevice, s));
    COSY_CHECK_HIP(hipMemcpyAsync(ids + n_cand, host_cand_view, nb, hipMemcpyHostToDevice, s));
    COSY_CHECK_HIP(hipMemcpyAsync(ids + 2 * (size_t)n_cand, host_cand_mesh, nb, hipMemcpyHostToDevice, s));
    COSY_CHECK_HIP(hipMemcpyAsync(ids + 3 * (size_t)n_cand, host_obj_mesh, (size_t)n_obj * sizeof(int), hipMemcpyHostToDevice, s));
    return COSY_OK;
}

int cosy_ba_align(const double* TWO_9d, const double* TCW_9d, const double* cand_TCO, const double* K, const int* ids, const double* pts_table,
                  const double* sym_table, const int* n_sym, int n_cand, int n_obj, int n_views, int n_mesh, int P, int S, double* dists,
                  int* best_sym, double* TCO_cand_aligned, cosy_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    BA_REQUIRE_SIZES("cosy_ba_align");
    COSY_REQUIRE(n_mesh > 0 && S > 0, "cosy_ba_align: n_mesh=%d S=%d", n_mesh, S);
    COSY_REQUIRE(TWO_9d && TCW_9d && cand_TCO && K && ids && pts_table && sym_table && n_sym && dists && best_sym && TCO_cand_aligned,
                 "cosy_ba_align: null pointer");
    hipLaunchKernelGGL(ba_align_kernel, dim3(n_cand), dim3(256), 0, s, TWO_9d, TCW_9d, cand_TCO, K, ids, pts_table, sym_table, n_sym, n_cand,
                       n_obj, n_views, n_mesh, P, S, dists, best_sym, TCO_cand_aligned);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

int cosy_ba_linearize(const double* TWO_9d, const double* TCW_9d, const double* TCO_cand_aligned, const double* K, const int* ids,
                      const double* pts_table, int n_cand, int n_obj, int n_views, int n_mesh, int P, double residuals_threshold,
                      double* errors, double* loss, double* A, double* b, double* J_obj, double* J_view, void* workspace,
                      cosy_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    BA_REQUIRE_SIZES("cosy_ba_linearize");
    COSY_REQUIRE(n_mesh > 0, "cosy_ba_linearize: n_mesh=%d", n_mesh);
    COSY_REQUIRE(TWO_9d && TCW_9d && TCO_cand_aligned && K && ids && pts_table && errors && loss && A && b && workspace,
                 "cosy_ba_linearize: null pointer");
    double* blk = (double*)workspace;
    double* loss_part = (double*)((char*)workspace + align256((size_t)n_cand * BA_BLK * sizeof(double)));
    hipLaunchKernelGGL(ba_linearize_kernel, dim3(n_cand), dim3(BA_ROWS), 0, s, TWO_9d, TCW_9d, TCO_cand_aligned, K, ids, pts_table, n_cand,
                       n_obj, n_views, n_mesh, P, residuals_threshold, errors, J_obj, J_view, blk, loss_part);
    COSY_CHECK_HIP(hipGetLastError());
    const int nb = n_obj + n_views;
    hipLaunchKernelGGL(ba_accumulate_kernel, dim3(nb, nb), dim3(128), 0, s, blk, loss_part, ids, n_cand, n_obj, n_views, P, A, b, loss);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

int cosy_ba_solve(const double* A, const double* b, int n, double lambda, double* h, void* workspace, cosy_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    COSY_REQUIRE(n > 0, "cosy_ba_solve: n=%d", n);
    COSY_REQUIRE(lambda > 0., "cosy_ba_solve: lambda=%g must be positive (A + lambda I is factored by Cholesky)", lambda);
    if (n > BA_MAX_N) {
        cosy::set_error("cosy_ba_solve: n=%d > %d", n, BA_MAX_N);
        return COSY_ESIZE;
    }
    COSY_REQUIRE(A && b && h && workspace, "cosy_ba_solve: null pointer");
    hipLaunchKernelGGL(ba_solve_kernel, dim3(1), dim3(BA_SOLVE_THREADS), 0, s, A, b, n, lambda, (double*)workspace, h);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

// ---- the batch ----
namespace {

struct BaBatchWs { double *blk, *loss_part, *aligned, *A, *L, *b; };

inline size_t ba_batch_ws_layout(int n_cand, int n_blocks, long long a_total, char* base, BaBatchWs* ws) {
    const size_t sizes[6] = {(size_t)n_cand * BA_BLK, (size_t)n_cand, (size_t)n_cand * 16, (size_t)a_total, (size_t)a_total,
                             (size_t)n_blocks * 9};
    double** out[6] = {ws ? &ws->blk : nullptr, ws ? &ws->loss_part : nullptr, ws ? &ws->aligned : nullptr, ws ? &ws->A : nullptr,
                       ws ? &ws->L : nullptr, ws ? &ws->b : nullptr};
    size_t off = 0;
    for (int i = 0; i < 6; ++i) {
        if (ws) *out[i] = (double*)(base + off);
        off += align256(sizes[i] * sizeof(double));
    }
    return off;
}

int ba_batch_check(const cosy_ba_batch_t* b, const char* name) {
    COSY_REQUIRE(b, "%s: null batch", name);
    COSY_REQUIRE(b->G > 0 && b->G <= COSY_MAX_GRID_Y && b->n_cand >= b->G && b->n_obj >= b->G && b->n_views >= b->G,
                 "%s: G=%d n_cand=%d n_obj=%d n_views=%d (every problem has a candidate, an object and a view; G <= %d)", name, b->G,
                 b->n_cand, b->n_obj, b->n_views, COSY_MAX_GRID_Y);
    COSY_REQUIRE(b->n_mesh > 0 && b->P > 0 && b->S > 0 && b->n_hist_rows > 0, "%s: n_mesh=%d P=%d S=%d n_hist_rows=%d", name, b->n_mesh,
                 b->P, b->S, b->n_hist_rows);
    if (b->max_blocks > BA_MAX_N / 9) {
        cosy::set_error("%s: max_blocks = %d > %d", name, b->max_blocks, BA_MAX_N / 9);
        return COSY_ESIZE;
    }
    COSY_REQUIRE(b->max_blocks >= 2 && b->a_total >= 324LL * b->G, "%s: max_blocks=%d a_total=%lld", name, b->max_blocks, b->a_total);
    COSY_REQUIRE(b->L_down > 0. && b->L_up > 0., "%s: L_down=%g L_up=%g must be positive", name, b->L_down, b->L_up);
    COSY_REQUIRE(b->table && b->cand_TCO && b->K && b->pts_table && b->sym_table && b->n_sym && b->TWO_9d && b->TCW_9d &&
                     b->TWO_9d_updated && b->TCW_9d_updated && b->ctrl && b->hist_iteration && b->hist_lambda && b->hist_loss &&
                     b->workspace,
                 "%s: null pointer", name);
    COSY_REQUIRE(!b->hist_TWO_9d == !b->hist_TCW_9d, "%s: hist_TWO_9d and hist_TCW_9d go together", name);
    return COSY_OK;
}

int ba_batch_linearize_launch(const cosy_ba_batch_t* b, int which, hipStream_t s) {
    const BaTab t = ba_tab(b->table, b->G, b->n_cand, b->n_obj);
    BaBatchWs ws;
    ba_batch_ws_layout(b->n_cand, b->n_obj + b->n_views, b->a_total, (char*)b->workspace, &ws);
    const double* TWO = which ? b->TWO_9d_updated : b->TWO_9d;
    const double* TCW = which ? b->TCW_9d_updated : b->TCW_9d;
    hipLaunchKernelGGL(ba_batch_align_kernel, dim3(b->n_cand), dim3(256), 0, s, t, b->ctrl, which, b->G, TWO, TCW, b->cand_TCO, b->K,
                       b->pts_table, b->sym_table, b->n_sym, b->n_mesh, b->P, b->S, ws.aligned);
    COSY_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(ba_batch_linearize_kernel, dim3(b->n_cand), dim3(BA_ROWS), 0, s, t, b->ctrl, which, b->G, TWO, TCW, ws.aligned, b->K,
                       b->pts_table, b->n_mesh, b->P, b->residuals_threshold, ws.blk, ws.loss_part);
    COSY_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(ba_batch_accumulate_kernel, dim3(b->max_blocks * b->max_blocks, b->G), dim3(128), 0, s, t, b->ctrl, which, ws.blk,
                       ws.loss_part, b->P, ws.A, ws.b);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

int ba_batch_solve_step_launch(const cosy_ba_batch_t* b, hipStream_t s) {
    const BaTab t = ba_tab(b->table, b->G, b->n_cand, b->n_obj);
    BaBatchWs ws;
    ba_batch_ws_layout(b->n_cand, b->n_obj + b->n_views, b->a_total, (char*)b->workspace, &ws);
    hipLaunchKernelGGL(ba_batch_solve_step_kernel, dim3(b->G), dim3(BA_SOLVE_THREADS), 0, s, t, b->ctrl, ws.A, ws.b, ws.L, b->TWO_9d,
                       b->TCW_9d, b->TWO_9d_updated, b->TCW_9d_updated, b->optimize_cameras);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

}  // namespace

size_t cosy_ba_batch_table_bytes(int G, int n_cand, int n_obj) {
    if (G <= 0 || n_cand <= 0 || n_obj <= 0) return 0;
    return ba_tab_ints(G, n_cand, n_obj) * sizeof(int) + ((size_t)G + 1) * sizeof(long long);
}

size_t cosy_ba_batch_workspace_bytes(int n_cand, int n_blocks, long long a_total) {
    if (n_cand <= 0 || n_blocks <= 0 || a_total <= 0) return 0;
    return ba_batch_ws_layout(n_cand, n_blocks, a_total, nullptr, nullptr);
}

int cosy_ba_batch_upload(const int* host_cand_obj, const int* host_cand_view, const int* host_cand_mesh, const int* host_obj_mesh,
                         const int* host_cand_off, const int* host_obj_off, const int* host_view_off, int G, int n_mesh, void* table,
                         long long* a_total, int* max_blocks, cosy_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    COSY_REQUIRE(G > 0 && G <= COSY_MAX_GRID_Y && n_mesh > 0, "cosy_ba_batch_upload: G=%d (1 .. %d) n_mesh=%d", G, COSY_MAX_GRID_Y, n_mesh);
    COSY_REQUIRE(host_cand_obj && host_cand_view && host_cand_mesh && host_obj_mesh && host_cand_off && host_obj_off && host_view_off &&
                     table && a_total && max_blocks,
                 "cosy_ba_batch_upload: null pointer");
    COSY_REQUIRE(host_cand_off[0] == 0 && host_obj_off[0] == 0 && host_view_off[0] == 0, "cosy_ba_batch_upload: offsets start at %d, %d, %d",
                 host_cand_off[0], host_obj_off[0], host_view_off[0]);
    long long a_sum = 0;
    int blocks_max = 0;
    for (int g = 0; g < G; ++g) {
        const long long nc = (long long)host_cand_off[g + 1] - host_cand_off[g], no = (long long)host_obj_off[g + 1] - host_obj_off[g],
                        nv = (long long)host_view_off[g + 1] - host_view_off[g];
        COSY_REQUIRE(nc > 0 && no > 0 && nv > 0, "cosy_ba_batch_upload: problem %d: %lld candidates, %lld objects, %lld views", g, nc, no, nv);
        if (no + nv > BA_MAX_N / 9) {
            cosy::set_error("cosy_ba_batch_upload: problem %d: n_obj + n_views = %lld > %d", g, no + nv, BA_MAX_N / 9);
            return COSY_ESIZE;
        }
        a_sum += 81 * (no + nv) * (no + nv);
        if (no + nv > blocks_max) blocks_max = (int)(no + nv);
    }
    const int n_cand = host_cand_off[G], n_obj = host_obj_off[G];
    for (int g = 0; g < G; ++g)
        for (int c = host_cand_off[g]; c < host_cand_off[g + 1]; ++c) {
            COSY_REQUIRE(host_cand_obj[c] >= host_obj_off[g] && host_cand_obj[c] < host_obj_off[g + 1],
                         "cosy_ba_batch_upload: problem %d, candidate %d: object row %d outside [%d, %d)", g, c, host_cand_obj[c],
                         host_obj_off[g], host_obj_off[g + 1]);
            COSY_REQUIRE(host_cand_view[c] >= host_view_off[g] && host_cand_view[c] < host_view_off[g + 1],
                         "cosy_ba_batch_upload: problem %d, candidate %d: view row %d outside [%d, %d)", g, c, host_cand_view[c],
                         host_view_off[g], host_view_off[g + 1]);
            COSY_REQUIRE(host_cand_mesh[c] >= 0 && host_cand_mesh[c] < n_mesh,
                         "cosy_ba_batch_upload: problem %d, candidate %d: mesh id %d outside [0, %d)", g, c, host_cand_mesh[c], n_mesh);
        }
    for (int o = 0; o < n_obj; ++o)
        COSY_REQUIRE(host_obj_mesh[o] >= 0 && host_obj_mesh[o] < n_mesh, "cosy_ba_batch_upload: object %d: mesh id %d outside [0, %d)", o,
                     host_obj_mesh[o], n_mesh);
    // the whole table in one host block, one copy
    const size_t n_ints = ba_tab_ints(G, n_cand, n_obj), bytes = cosy_ba_batch_table_bytes(G, n_cand, n_obj);
    int* host = (int*)calloc(1, bytes);
    COSY_REQUIRE(host, "cosy_ba_batch_upload: out of host memory (%zu bytes)", bytes);
    int* w = host;
    memcpy(w, host_cand_obj, (size_t)n_cand * sizeof(int)); w += n_cand;
    memcpy(w, host_cand_view, (size_t)n_cand * sizeof(int)); w += n_cand;
    memcpy(w, host_cand_mesh, (size_t)n_cand * sizeof(int)); w += n_cand;
    for (int g = 0; g < G; ++g)
        for (int c = host_cand_off[g]; c < host_cand_off[g + 1]; ++c) w[c] = g;
    w += n_cand;
    memcpy(w, host_obj_mesh, (size_t)n_obj * sizeof(int)); w += n_obj;
    memcpy(w, host_cand_off, ((size_t)G + 1) * sizeof(int)); w += G + 1;
    memcpy(w, host_obj_off, ((size_t)G + 1) * sizeof(int)); w += G + 1;
    memcpy(w, host_view_off, ((size_t)G + 1) * sizeof(int));
    long long* a_off = (long long*)(host + n_ints);
    a_off[0] = 0;
    for (int g = 0; g < G; ++g) {
        const long long nb = ((long long)host_obj_off[g + 1] - host_obj_off[g]) + ((long long)host_view_off[g + 1] - host_view_off[g]);
        a_off[g + 1] = a_off[g] + 81 * nb * nb;
    }
    hipError_t e = hipMemcpyAsync(table, host, bytes, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);     // `host` is freed below
    free(host);
    COSY_CHECK_HIP(e);
    *a_total = a_sum;
    *max_blocks = blocks_max;
    return COSY_OK;
}

int cosy_ba_batch_linearize(const cosy_ba_batch_t* batch, int which, cosy_stream_t stream) {
    const int rc = ba_batch_check(batch, "cosy_ba_batch_linearize");
    if (rc != COSY_OK) return rc;
    COSY_REQUIRE(which == 0 || which == 1, "cosy_ba_batch_linearize: which=%d", which);
    return ba_batch_linearize_launch(batch, which, (hipStream_t)stream);
}

int cosy_ba_batch_solve_step(const cosy_ba_batch_t* batch, cosy_stream_t stream) {
    const int rc = ba_batch_check(batch, "cosy_ba_batch_solve_step");
    if (rc != COSY_OK) return rc;
    return ba_batch_solve_step_launch(batch, (hipStream_t)stream);
}

int cosy_ba_batch_record(cosy_ba_ctrl_t* ctrl, int G, int iteration, int n_hist_rows, const void* table, int n_cand, int n_obj,
                         int n_views, const double* TWO_9d, const double* TCW_9d, int* hist_iteration, double* hist_lambda,
                         double* hist_loss, double* hist_TWO_9d, double* hist_TCW_9d, cosy_stream_t stream) {
    COSY_REQUIRE(G > 0 && iteration >= 0 && n_hist_rows > 0, "cosy_ba_batch_record: G=%d iteration=%d n_hist_rows=%d", G, iteration,
                 n_hist_rows);
    COSY_REQUIRE(ctrl && hist_iteration && hist_lambda && hist_loss, "cosy_ba_batch_record: null pointer");
    COSY_REQUIRE(!hist_TWO_9d == !hist_TCW_9d, "cosy_ba_batch_record: hist_TWO_9d and hist_TCW_9d go together");
    BaTab t = {};
    if (hist_TWO_9d) {
        COSY_REQUIRE(table && TWO_9d && TCW_9d && n_cand > 0 && n_obj > 0 && n_views > 0,
                     "cosy_ba_batch_record: a state history needs the table and the states (n_cand=%d n_obj=%d n_views=%d)", n_cand, n_obj,
                     n_views);
        t = ba_tab(table, G, n_cand, n_obj);
    }
    hipLaunchKernelGGL(ba_batch_record_kernel, dim3(G), dim3(256), 0, (hipStream_t)stream, t, ctrl, iteration, n_hist_rows, n_obj, n_views,
                       TWO_9d, TCW_9d, hist_iteration, hist_lambda, hist_loss, hist_TWO_9d, hist_TCW_9d);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

int cosy_ba_batch_decide(cosy_ba_ctrl_t* ctrl, int G, double L_down, double L_up, double eps, const void* table, int n_cand, int n_obj,
                         double* TWO_9d, double* TCW_9d, const double* TWO_9d_updated, const double* TCW_9d_updated,
                         cosy_stream_t stream) {
    COSY_REQUIRE(G > 0 && L_down > 0. && L_up > 0., "cosy_ba_batch_decide: G=%d L_down=%g L_up=%g", G, L_down, L_up);
    COSY_REQUIRE(ctrl, "cosy_ba_batch_decide: null ctrl");
    BaTab t = {};
    if (TWO_9d || TCW_9d || TWO_9d_updated || TCW_9d_updated) {
        COSY_REQUIRE(table && TWO_9d && TCW_9d && TWO_9d_updated && TCW_9d_updated && n_cand > 0 && n_obj > 0,
                     "cosy_ba_batch_decide: the states go together with the table (n_cand=%d n_obj=%d)", n_cand, n_obj);
        t = ba_tab(table, G, n_cand, n_obj);
    }
    hipLaunchKernelGGL(ba_batch_decide_kernel, dim3(G), dim3(256), 0, (hipStream_t)stream, t, ctrl, L_down, L_up, eps, TWO_9d, TCW_9d,
                       TWO_9d_updated, TCW_9d_updated);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

int cosy_ba_batch_iterate(const cosy_ba_batch_t* batch, int n_first, int n_count, cosy_stream_t stream) {
    const int rc = ba_batch_check(batch, "cosy_ba_batch_iterate");
    if (rc != COSY_OK) return rc;
    COSY_REQUIRE(n_first >= 0 && n_count >= 0, "cosy_ba_batch_iterate: n_first=%d n_count=%d", n_first, n_count);
    const cosy_ba_batch_t* b = batch;
    for (int n = n_first; n < n_first + n_count; ++n) {
        int r = ba_batch_linearize_launch(b, 0, (hipStream_t)stream);
        if (r != COSY_OK) return r;
        r = cosy_ba_batch_record(b->ctrl, b->G, n, b->n_hist_rows, b->table, b->n_cand, b->n_obj, b->n_views, b->TWO_9d, b->TCW_9d,
                                 b->hist_iteration, b->hist_lambda, b->hist_loss, b->hist_TWO_9d, b->hist_TCW_9d, stream);
        if (r != COSY_OK) return r;
        r = ba_batch_solve_step_launch(b, (hipStream_t)stream);
        if (r != COSY_OK) return r;
        r = ba_batch_linearize_launch(b, 1, (hipStream_t)stream);
        if (r != COSY_OK) return r;
        r = cosy_ba_batch_decide(b->ctrl, b->G, b->L_down, b->L_up, b->eps, b->table, b->n_cand, b->n_obj, b->TWO_9d, b->TCW_9d,
                                 b->TWO_9d_updated, b->TCW_9d_updated, stream);
        if (r != COSY_OK) return r;
    }
    return COSY_OK;
}

}  // extern "C"
