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

__global__ __launch_bounds__(256) void ba_align_kernel(const double* __restrict__ TWO_9d, const double* __restrict__ TCW_9d,
                                                       const double* __restrict__ cand_TCO, const double* __restrict__ K,
                                                       const int* __restrict__ ids, const double* __restrict__ pts,
                                                       const double* __restrict__ sym, const int* __restrict__ n_sym, int n_cand, int n_obj,
                                                       int n_views, int n_mesh, int P, int S, double* __restrict__ dists,
                                                       int* __restrict__ best_sym, double* __restrict__ aligned) {
    __shared__ double red[4];
    const int c = blockIdx.x, tid = threadIdx.x;
    int o, v, m, mo;
    if (!cand_ids(ids, c, n_cand, n_obj, n_views, n_mesh, o, v, m, mo)) return;
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
        if (tid == 0) { dists[c] = __builtin_nan(""); best_sym[c] = -1; }
        if (tid < 16) aligned[(size_t)c * 16 + tid] = __builtin_nan("");
        return;
    }
    double d;
    const double* sm = sym + (size_t)m * S * 16;
    const int best = reprojected_best_symmetry<double>(t1, Tco, k, pts + (size_t)m * P * 3, sm, ns, P, red, d);
    if (tid == 0) { dists[c] = d; best_sym[c] = best; }
    if (tid < 16 && best >= 0) {   // TCO_cand_aligned = cand_TCO @ S
        const int i = tid >> 2, j = tid & 3;
        double acc = 0.;
#pragma unroll
        for (int q = 0; q < 4; ++q) acc += t1[i * 4 + q] * sm[(size_t)best * 16 + q * 4 + j];
        aligned[(size_t)c * 16 + tid] = acc;
    }
}

// One workgroup per candidate.  Thread t of a pass owns residual row r = pass*256 + t: point r/2, coordinate r%2 (the reference's order,
// bundle_adjustment.py:93-110).  The rows of a pass are staged in LDS, then thread t < 189 adds the pass' contribution to its entry of
// the upper triangle of J_c^T J_c (171) or of J_c^T e_c (18), rows in order.
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
    const int c = blockIdx.x, tid = threadIdx.x;
    int o, v, m, mo;
    const bool ok = cand_ids(ids, c, n_cand, n_obj, n_views, n_mesh, o, v, m, mo);
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
            errors[gr] = e;
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

__device__ __forceinline__ int tri_index(int i, int j) {   // i <= j < 18
    return i * 18 - (i * (i - 1)) / 2 + (j - i);
}

// A (n,n) and b (n), n = 9 (n_obj + n_views), objects first: workgroup (bj, bi) writes the 9x9 block (bi, bj) -- zeros included, so A
// needs no clearing -- as the sum over the candidates of that block IN CANDIDATE ORDER; column 0's workgroups also write b, workgroup
// (0,0) the loss.
__global__ __launch_bounds__(128) void ba_accumulate_kernel(const double* __restrict__ blk, const double* __restrict__ loss_part,
                                                            const int* __restrict__ ids, int n_cand, int n_obj, int n_views, int P,
                                                            double* __restrict__ A, double* __restrict__ b, double* __restrict__ loss) {
    const int bi = blockIdx.y, bj = blockIdx.x, tid = threadIdx.x;
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
            for (int c = 0; c < n_cand; ++c) {
                const int o = ids[c], v = ids[n_cand + c];
                if ((want_o < 0 || o == want_o) && (want_v < 0 || v == want_v)) acc += blk[(size_t)c * BA_BLK + e];
            }
        }
        A[(size_t)(bi * 9 + r) * n + bj * 9 + cc] = acc;
    }
    if (bj == 0 && tid >= 96 && tid < 105) {
        const int t = tid - 96;
        double acc = 0.;
        for (int c = 0; c < n_cand; ++c) {
            const int o = ids[c], v = ids[n_cand + c];
            if (io ? o == bi : v == bi - n_obj) acc += blk[(size_t)c * BA_BLK + BA_TRI + (io ? t : 9 + t)];
        }
        b[bi * 9 + t] = acc;
    }
    if (bi == 0 && bj == 0 && tid == 127) {
        double acc = 0.;
        for (int c = 0; c < n_cand; ++c) acc += loss_part[c];
        *loss = acc / ((double)n_cand * (double)(2 * P));
    }
}

// h = (A + lambda I)^-1 b: right-looking Cholesky of the lower triangle in `L` (n*n doubles of workspace), then L y = b, L^T h = y.
// One workgroup; column k and the right-hand side live in LDS.  A non-positive pivot gives NaNs in h (the caller's loss test rejects).
__global__ __launch_bounds__(BA_SOLVE_THREADS) void ba_solve_kernel(const double* __restrict__ A, const double* __restrict__ b, int n,
                                                                    double lambda, double* __restrict__ L, double* __restrict__ h) {
    __shared__ double col[BA_MAX_N], vec[BA_MAX_N], dg[BA_MAX_N];
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
    for (int i = tid; i < n; i += BA_SOLVE_THREADS) h[i] = vec[i];
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

}  // extern "C"
