// Multi-view candidate matching (CosyPose stage 2): RANSAC over pairs of tentative matches, float32.
// Reference: cosypose/multiview/ransac.py:19-88 (camera-pose hypotheses, scoring), csrc/cosypose_cext.cpp:107-216 (inliers, best
// hypothesis per view pair).
//
// The reference expands every (hypothesis, tentative match) pair on the host, materialises one 4x4 and one distance per pair, copies
// the distances to the host and does the inlier bookkeeping in C++.  Here three launches do it and per hypothesis two numbers leave
// the chip:
//   ransac_hypotheses_kernel  one lane per (seed, symmetry of label_gd); the lanes of a seed walk the symmetries of label_ab together
//   ransac_score_kernel       one workgroup per hypothesis: a thread per tentative match of its view pair scores it, the inliers are
//                             ordered by (distance, list position) with a bitonic sort in LDS, one thread walks them greedily
//   ransac_best_kernel        one workgroup per view pair: best hypothesis, then the same walk again for the winner alone, this time
//                             writing the matches
// The distance is symmetric_distance_batched_fast (kernels_dist.hip, mode 1: best symmetry by the mean SQUARED distance over the
// padded table, result = the mean distance of that symmetry), every tie decided as the reference does: strict <, first index wins.
// Every sum has a fixed order and nothing is accumulated with atomics: two runs give the same bits.  Ids outside their tables are
// rejected by the Python layer before upload; the kernels skip them (such a match is no inlier, such a seed gives best_sym = -1).
//
// LDS of the two sorting kernels (dynamic): 8 bytes per sort slot (slots = the longest tentative-match list rounded up to a power
// of two, at least 128) + one bit per slot for each of the two "candidate already used" sets.  4096 matches (RANSAC_MAX_TM) are
// 33 KB; a scene whose longest list has 140 (25 objects, 8 views) takes 2 KB, so that the residency of ransac_score_kernel is
// bounded by waves, not by LDS.
#include "cosy_common.h"
#include "dist_device.h"

#pragma clang fp contract(off)

namespace cosy {

namespace {

constexpr int RANSAC_MAX_TM = 4096;     // tentative matches per ordered view pair (cosy_ransac_max_tmatches)
constexpr int RANSAC_THREADS = 128;     // ransac_score_kernel / ransac_best_kernel: the production scene averages 111 matches per hypothesis
constexpr unsigned long long KEY_NONE = ~0ull;

// Sort key of an inlier: (distance, list position).  The distance goes through the usual order-preserving float -> unsigned map
// (negative: all bits flipped, otherwise: sign bit set), so that given distances below zero (the public find_ransac_inliers takes
// any float) sort before the positive ones as the reference's `<` puts them; -0 is keyed as +0, which `<` ties with it, so that
// the list position decides.  NaN never gets here (it fails dist <= thr); +inf maps to 0xff800000, below KEY_NONE.
__device__ __forceinline__ unsigned long long sort_key(float dist, int i) {
    const unsigned u = __float_as_uint(dist + 0.f);
    const unsigned m = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)m << 32) | (unsigned)i;
}
__device__ __forceinline__ float key_dist(unsigned long long key) {
    const unsigned m = (unsigned)(key >> 32);
    return __uint_as_float((m & 0x80000000u) ? (m ^ 0x80000000u) : ~m);
}

struct RansacScene {
    const float* poses;      // (n_cand,4,4) TCO of every candidate
    const int* cand_mesh;    // (n_cand) row of the candidate's label in the tables
    const float* pts;        // (n_mesh,P,3)
    const float* sym;        // (n_mesh,S,4,4), identity-padded
    const int* n_sym;        // (n_mesh)
    int n_cand, n_mesh, P, S;
};

__device__ __forceinline__ void load16(const float* p, float* T) {
#pragma unroll
    for (int i = 0; i < 16; ++i) T[i] = p[i];
}
// invert_T (lib3d/transform_ops.py:24-32): R^T, -R^T t
__device__ __forceinline__ void invert_T(const float* T, float* O) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) O[i * 4 + j] = T[j * 4 + i];
        O[i * 4 + 3] = -((T[0 * 4 + i] * T[3] + T[1 * 4 + i] * T[7]) + T[2 * 4 + i] * T[11]);
    }
    O[12] = T[12]; O[13] = T[13]; O[14] = T[14]; O[15] = T[15];
}
// sums over the P points of |A p - B p|^2 and |A p - B p|, points in table order
__device__ __forceinline__ void point_sums(const float* A, const float* Bm, const float* __restrict__ p, int P, float& sum_sq, float& sum_n) {
    sum_sq = 0.f; sum_n = 0.f;
    for (int i = 0; i < P; ++i) {
        const float x = p[i * 3], y = p[i * 3 + 1], z = p[i * 3 + 2];
        float q1[3], q2[3];
        xform_pt(A, x, y, z, q1);
        xform_pt(Bm, x, y, z, q2);
        const float dx = q1[0] - q2[0], dy = q1[1] - q2[1], dz = q1[2] - q2[2];
        const float sq = (dx * dx + dy * dy) + dz * dz;
        sum_sq += sq;
        sum_n += sqrtf(sq);
    }
}
// symmetric_distance_batched_fast of one item by one thread
__device__ __forceinline__ float fast_distance(const float* T1, const float* T2, const float* __restrict__ p, const float* __restrict__ sym, int P, int S) {
    float best_c = 0.f, best_d = 0.f;
    for (int k = 0; k < S; ++k) {
        float sm[16], M[16], sum_sq, sum_n;
        load16(sym + (size_t)k * 16, sm);
        mat4_mul(T1, sm, M);
        point_sums(M, T2, p, P, sum_sq, sum_n);
        const float c = sum_sq / (float)P;
        if (k == 0 || c < best_c) { best_c = c; best_d = sum_n / (float)P; }
    }
    return best_d;
}

// ---- hypotheses: ransac.py:19-47 ------------------------------------------------------------------------------------------------
// G = lanes per seed (power of two >= S, <= 64).  Lane k of a seed holds TC1Og S_gd[k]; for each symmetry s of label_ab all of them
// form T2 = ((TC1Oa S_ab[s]) inv(TC2Ob)) TC2Od (the reference's association), lane k sums its symmetry's point distances, and a
// xor-shuffle argmin over the G lanes (smaller mean squared distance, then lower k) leaves the distance of s in every lane.
__global__ __launch_bounds__(256) void ransac_hypotheses_kernel(RansacScene sc, const int* __restrict__ seeds, int H, int G,
                                                                float* __restrict__ TC1C2, int* __restrict__ best_sym, float* __restrict__ gap,
                                                                float* __restrict__ sym_dists) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const long h = t / G;
    const int k = (int)(t % G);
    int a = -1, b = -1, g = -1, d = -1;
    if (h < H) { a = seeds[h * 4]; b = seeds[h * 4 + 1]; g = seeds[h * 4 + 2]; d = seeds[h * 4 + 3]; }
    const unsigned nc = (unsigned)sc.n_cand;
    bool valid = h < H && (unsigned)a < nc && (unsigned)b < nc && (unsigned)g < nc && (unsigned)d < nc;
    int m_ab = 0, m_gd = 0;
    if (valid) {
        m_ab = sc.cand_mesh[a]; m_gd = sc.cand_mesh[g];
        valid = (unsigned)m_ab < (unsigned)sc.n_mesh && (unsigned)m_gd < (unsigned)sc.n_mesh;
    }
    if (!valid) { a = b = g = d = 0; m_ab = m_gd = 0; }        // keeps the lane in step with the shuffles; nothing of it is stored
    float Ta[16], TbInv[16], Td[16], A[16];
    {
        float Tb[16], Tg[16], sm[16];
        load16(sc.poses + (size_t)a * 16, Ta);
        load16(sc.poses + (size_t)b * 16, Tb);
        load16(sc.poses + (size_t)g * 16, Tg);
        load16(sc.poses + (size_t)d * 16, Td);
        invert_T(Tb, TbInv);
        load16(sc.sym + ((size_t)m_gd * sc.S + (k < sc.S ? k : 0)) * 16, sm);
        mat4_mul(Tg, sm, A);
    }
    const float* p = sc.pts + (size_t)m_gd * sc.P * 3;
    const int ns_ab = min(max(sc.n_sym[m_ab], 1), sc.S);
    const float inf = __builtin_inff();
    int best = -1;
    float min1 = inf, min2 = inf;
    for (int s = 0; s < sc.S; ++s) {            // uniform trip count: every lane of the wave takes part in every shuffle
        const int ss = s < ns_ab ? s : 0;
        float sm[16], M1[16], M2[16], T2[16];
        load16(sc.sym + ((size_t)m_ab * sc.S + ss) * 16, sm);
        mat4_mul(Ta, sm, M1);
        mat4_mul(M1, TbInv, M2);
        mat4_mul(M2, Td, T2);
        float c = inf, dist = inf;
        int kk = G;
        if (k < sc.S) {
            float sum_sq, sum_n;
            point_sums(A, T2, p, sc.P, sum_sq, sum_n);
            c = sum_sq / (float)sc.P; dist = sum_n / (float)sc.P; kk = k;
        }
        for (int o = G >> 1; o > 0; o >>= 1) {
            const float c2 = __shfl_xor(c, o);
            const float d2 = __shfl_xor(dist, o);
            const int k2 = __shfl_xor(kk, o);
            if (c2 < c || (c2 == c && k2 < kk)) { c = c2; dist = d2; kk = k2; }
        }
        if (s < ns_ab) {
            if (sym_dists && valid && k == 0) sym_dists[h * sc.S + s] = dist;
            if (best < 0 || dist < min1) { min2 = min1; min1 = dist; best = s; }      // scatter_argmin: strict <, the first minimum stays
            else if (dist < min2) min2 = dist;
        } else if (sym_dists && valid && k == 0) {
            sym_dists[h * sc.S + s] = inf;
        }
    }
    if (k != 0 || h >= H) return;
    if (!valid) {
        best_sym[h] = -1; gap[h] = inf;
        for (int i = 0; i < 16; ++i) TC1C2[h * 16 + i] = 0.f;
        return;
    }
    float sm[16], M1[16], out[16];
    load16(sc.sym + ((size_t)m_ab * sc.S + best) * 16, sm);
    mat4_mul(Ta, sm, M1);
    mat4_mul(M1, TbInv, out);
    for (int i = 0; i < 16; ++i) TC1C2[h * 16 + i] = out[i];
    best_sym[h] = best;
    gap[h] = min2 - min1;
}

// ---- score + inliers of one hypothesis by one workgroup: ransac.py:67-88, cosypose_cext.cpp:156-185 ------------------------------
// tm: (n_tm,4) int32 per tentative match: cand1, cand2, and their ranks among the cand1s / cand2s of the view pair (what the two
// "already used" bit sets are indexed by).  The matches of view pair p are tm[pair_off[p] .. pair_off[p+1]).
struct Walk { int n_inliers; float dists_sum; };

template <bool WRITE>
__device__ __forceinline__ Walk score_and_walk(const RansacScene& sc, const float* __restrict__ Th, const int4* __restrict__ tm, int n_tm, int slots,
                                               float thr, const float* __restrict__ dists_in, float* __restrict__ dists_out,
                                               unsigned long long* keys, unsigned* used1, unsigned* used2, int* out_c1, int* out_c2) {
    const int tid = threadIdx.x;
    float T[16];
    if (!dists_in) load16(Th, T);         // with given distances the poses are not read (and may be absent)
    for (int i = tid; i < slots; i += RANSAC_THREADS) {
        unsigned long long key = KEY_NONE;
        if (i < n_tm) {
            const int4 m = tm[i];
            float dist = __builtin_inff();
            if (dists_in) {
                dist = dists_in[i];
            } else if ((unsigned)m.x < (unsigned)sc.n_cand && (unsigned)m.y < (unsigned)sc.n_cand) {
                const int o = sc.cand_mesh[m.x];
                if ((unsigned)o < (unsigned)sc.n_mesh) {
                    float T1[16], Tb[16], T2[16];
                    load16(sc.poses + (size_t)m.x * 16, T1);
                    load16(sc.poses + (size_t)m.y * 16, Tb);
                    mat4_mul(T, Tb, T2);
                    dist = fast_distance(T1, T2, sc.pts + (size_t)o * sc.P * 3, sc.sym + (size_t)o * sc.S * 16, sc.P, sc.S);
                }
            }
            if (dists_out) dists_out[i] = dist;
            const bool ok = (unsigned)m.z < (unsigned)n_tm && (unsigned)m.w < (unsigned)n_tm;
            if (ok && dist <= thr) key = sort_key(dist, i);
        }
        keys[i] = key;
    }
    for (int i = tid; i < (slots >> 5); i += RANSAC_THREADS) { used1[i] = 0u; used2[i] = 0u; }
    __syncthreads();
    // bitonic sort, ascending: (distance, list position) = the reference's stable_sort by distance; the non-inliers (KEY_NONE) go last
    for (int kk = 2; kk <= slots; kk <<= 1)
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < slots; i += RANSAC_THREADS) {
                const int l = i ^ j;
                if (l > i) {
                    const unsigned long long x = keys[i], y = keys[l];
                    if ((x > y) == ((i & kk) == 0)) { keys[i] = y; keys[l] = x; }
                }
            }
            __syncthreads();
        }
    Walk w = {0, 0.f};
    if (tid == 0) {
        for (int i = 0; i < n_tm; ++i) {
            const unsigned long long key = keys[i];
            if (key == KEY_NONE) break;
            const int4 m = tm[(unsigned)key];
            const unsigned b1 = 1u << (m.z & 31), b2 = 1u << (m.w & 31);
            if ((used1[m.z >> 5] & b1) || (used2[m.w >> 5] & b2)) continue;
            used1[m.z >> 5] |= b1; used2[m.w >> 5] |= b2;
            if (WRITE) { out_c1[w.n_inliers] = m.x; out_c2[w.n_inliers] = m.y; }
            w.dists_sum += dists_in ? dists_in[(unsigned)key] : key_dist(key);      // the stored distance where there is one
            w.n_inliers += 1;
        }
    }
    return w;       // in thread 0
}

__device__ __forceinline__ int sort_slots(int n_tm) {
    int s = RANSAC_THREADS;
    while (s < n_tm) s <<= 1;
    return s;
}

__global__ __launch_bounds__(RANSAC_THREADS) void ransac_score_kernel(RansacScene sc, const float* __restrict__ TC1C2, const int* __restrict__ hyp_pair,
                                                                      int n_pairs, const int* __restrict__ pair_off, const int4* __restrict__ tm, float thr,
                                                                      const long long* __restrict__ hyp_dist_off, const float* __restrict__ dists_in,
                                                                      float* __restrict__ dists_out, int* __restrict__ n_inliers,
                                                                      float* __restrict__ dists_sum) {
    extern __shared__ unsigned long long lds_keys[];
    const int h = blockIdx.x;
    const int p = hyp_pair[h];
    if ((unsigned)p >= (unsigned)n_pairs) {         // uniform over the workgroup
        if (threadIdx.x == 0) { n_inliers[h] = 0; dists_sum[h] = 0.f; }
        return;
    }
    const int first = pair_off[p], n_tm = pair_off[p + 1] - first;
    const int slots = sort_slots(n_tm);
    unsigned* used1 = (unsigned*)(lds_keys + slots);
    unsigned* used2 = used1 + (slots >> 5);
    const long long off = hyp_dist_off ? hyp_dist_off[h] : 0;
    const Walk w = score_and_walk<false>(sc, TC1C2 + (size_t)h * 16, tm + first, n_tm, slots, thr, dists_in ? dists_in + off : nullptr,
                                         dists_out ? dists_out + off : nullptr, lds_keys, used1, used2, nullptr, nullptr);
    if (threadIdx.x == 0) { n_inliers[h] = w.n_inliers; dists_sum[h] = w.dists_sum; }
}

// ---- best hypothesis per view pair: cosypose_cext.cpp:187-210 -------------------------------------------------------------------
// The hypotheses of pair p are pair_hyps[pair_hyp_off[p] .. pair_hyp_off[p+1]), ascending.  Most inliers, then the smaller sum, then
// the lower id (= the first kept under the reference's strict comparisons); at least n_min_inliers.  skip_zero = the reference's
// `hypothesis_id > 0`: hypothesis 0 is never reported.  The winner's matches go to match_c1/c2[pair_off[p] ...], their number to
// n_matches[p].
__global__ __launch_bounds__(RANSAC_THREADS) void ransac_best_kernel(RansacScene sc, const float* __restrict__ TC1C2, int H, const int* __restrict__ n_inliers,
                                                                     const float* __restrict__ dists_sum, const int* __restrict__ pair_hyp_off,
                                                                     const int* __restrict__ pair_hyps, const int* __restrict__ pair_off,
                                                                     const int4* __restrict__ tm, float thr, int n_min_inliers, int skip_zero,
                                                                     const long long* __restrict__ hyp_dist_off, const float* __restrict__ dists_in,
                                                                     int* __restrict__ best_hyp, int* __restrict__ n_matches, int* __restrict__ match_c1,
                                                                     int* __restrict__ match_c2) {
    extern __shared__ unsigned long long lds_keys[];
    __shared__ int red_n[RANSAC_THREADS], red_h[RANSAC_THREADS];
    __shared__ float red_d[RANSAC_THREADS];
    const int p = blockIdx.x, tid = threadIdx.x;
    int bn = -1, bh = -1;
    float bd = 0.f;
    for (int i = pair_hyp_off[p] + tid; i < pair_hyp_off[p + 1]; i += RANSAC_THREADS) {       // ascending ids per thread: strict comparisons keep the first
        const int h = pair_hyps[i];
        if ((unsigned)h >= (unsigned)H) continue;
        const int n = n_inliers[h];
        const float ds = dists_sum[h];
        if (n >= n_min_inliers && (bh < 0 || n > bn || (n == bn && ds < bd))) { bn = n; bd = ds; bh = h; }
    }
    red_n[tid] = bn; red_d[tid] = bd; red_h[tid] = bh;
    __syncthreads();
    if (tid == 0) {
        for (int i = 1; i < RANSAC_THREADS; ++i) {
            const int n = red_n[i], h = red_h[i];
            const float ds = red_d[i];
            if (h >= 0 && (bh < 0 || n > bn || (n == bn && (ds < bd || (ds == bd && h < bh))))) { bn = n; bd = ds; bh = h; }
        }
        if (bh < 0 || (skip_zero && bh == 0)) bh = -1;
        red_h[0] = bh;
    }
    __syncthreads();
    bh = red_h[0];
    if (bh < 0) {
        if (tid == 0) { best_hyp[p] = -1; n_matches[p] = 0; }
        return;
    }
    const int first = pair_off[p], n_tm = pair_off[p + 1] - first;
    const int slots = sort_slots(n_tm);
    unsigned* used1 = (unsigned*)(lds_keys + slots);
    unsigned* used2 = used1 + (slots >> 5);
    const Walk w = score_and_walk<true>(sc, TC1C2 + (size_t)bh * 16, tm + first, n_tm, slots, thr,
                                        dists_in ? dists_in + hyp_dist_off[bh] : nullptr, nullptr, lds_keys, used1, used2, match_c1 + first,
                                        match_c2 + first);
    if (tid == 0) { best_hyp[p] = bh; n_matches[p] = w.n_inliers; }
}

int check_scene(const char* who, const float* cand_poses, const int* cand_mesh, const float* pts_table, const float* sym_table, int n_cand,
                int n_mesh, int P, int S) {
    COSY_REQUIRE(n_cand > 0 && n_mesh > 0 && P > 0 && S > 0, "%s: n_cand=%d n_mesh=%d P=%d S=%d", who, n_cand, n_mesh, P, S);
    COSY_REQUIRE(cand_poses && cand_mesh && pts_table && sym_table, "%s: null pointer", who);
    return COSY_OK;
}

size_t sort_lds_bytes(int max_tm) {
    int slots = RANSAC_THREADS;
    while (slots < max_tm) slots <<= 1;
    return (size_t)slots * 8 + 2 * (size_t)(slots / 32) * 4;
}

}  // namespace

}  // namespace cosy

using namespace cosy;

extern "C" {

int cosy_ransac_max_tmatches(void) { return RANSAC_MAX_TM; }

int cosy_ransac_hypotheses(const float* cand_poses, const int* cand_mesh, const float* pts_table, const float* sym_table, const int* n_sym,
                           int n_cand, int n_mesh, int P, int S, const int* seeds, int H, float* TC1C2, int* best_sym, float* gap,
                           float* sym_dists, cosy_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    COSY_REQUIRE(H >= 0, "cosy_ransac_hypotheses: H=%d", H);
    if (H == 0) return COSY_OK;
    if (int rc = check_scene("cosy_ransac_hypotheses", cand_poses, cand_mesh, pts_table, sym_table, n_cand, n_mesh, P, S)) return rc;
    COSY_REQUIRE(n_sym && seeds && TC1C2 && best_sym && gap, "cosy_ransac_hypotheses: null pointer");
    if (S > 64) {
        set_error("cosy_ransac_hypotheses: S=%d symmetries > 64 (one wave's lanes)", S);
        return COSY_ESIZE;
    }
    int G = 1;
    while (G < S) G <<= 1;
    const RansacScene sc = {cand_poses, cand_mesh, pts_table, sym_table, n_sym, n_cand, n_mesh, P, S};
    hipLaunchKernelGGL(ransac_hypotheses_kernel, dim3(cdiv((long)H * G, 256)), dim3(256), 0, s, sc, seeds, H, G, TC1C2, best_sym, gap, sym_dists);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

int cosy_ransac_score(const float* cand_poses, const int* cand_mesh, const float* pts_table, const float* sym_table, int n_cand, int n_mesh,
                      int P, int S, const float* TC1C2, const int* hyp_pair, int H, const int* pair_off, const int* tmatches, int n_pairs,
                      int max_tm, float dist_threshold, const long long* hyp_dist_off, const float* dists_in, float* dists_out,
                      int* n_inliers, float* dists_sum, cosy_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    COSY_REQUIRE(H >= 0 && n_pairs >= 0 && max_tm >= 0, "cosy_ransac_score: H=%d n_pairs=%d max_tm=%d", H, n_pairs, max_tm);
    if (max_tm > RANSAC_MAX_TM) {
        set_error("cosy_ransac_score: %d tentative matches in one view pair > %d", max_tm, RANSAC_MAX_TM);
        return COSY_ESIZE;
    }
    if (H == 0) return COSY_OK;
    if (!dists_in) {
        if (int rc = check_scene("cosy_ransac_score", cand_poses, cand_mesh, pts_table, sym_table, n_cand, n_mesh, P, S)) return rc;
        COSY_REQUIRE(TC1C2, "cosy_ransac_score: null pointer");
    }
    COSY_REQUIRE(hyp_pair && pair_off && tmatches && n_inliers && dists_sum, "cosy_ransac_score: null pointer");
    COSY_REQUIRE(hyp_dist_off || (!dists_in && !dists_out), "cosy_ransac_score: a distance table needs hyp_dist_off");
    const RansacScene sc = {cand_poses, cand_mesh, pts_table, sym_table, nullptr, n_cand, n_mesh, P, S};
    hipLaunchKernelGGL(ransac_score_kernel, dim3(H), dim3(RANSAC_THREADS), sort_lds_bytes(max_tm), s, sc, TC1C2, hyp_pair, n_pairs, pair_off,
                       (const int4*)tmatches, dist_threshold, hyp_dist_off, dists_in, dists_out, n_inliers, dists_sum);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

int cosy_ransac_best(const float* cand_poses, const int* cand_mesh, const float* pts_table, const float* sym_table, int n_cand, int n_mesh,
                     int P, int S, const float* TC1C2, int H, const int* n_inliers, const float* dists_sum, const int* pair_hyp_off,
                     const int* pair_hyps, const int* pair_off, const int* tmatches, int n_pairs, int max_tm, float dist_threshold,
                     int n_min_inliers, int skip_hypothesis_0, const long long* hyp_dist_off, const float* dists_in, int* best_hyp,
                     int* n_matches, int* match_cand1, int* match_cand2, cosy_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    COSY_REQUIRE(H >= 0 && n_pairs >= 0 && max_tm >= 0, "cosy_ransac_best: H=%d n_pairs=%d max_tm=%d", H, n_pairs, max_tm);
    if (max_tm > RANSAC_MAX_TM) {
        set_error("cosy_ransac_best: %d tentative matches in one view pair > %d", max_tm, RANSAC_MAX_TM);
        return COSY_ESIZE;
    }
    if (n_pairs == 0) return COSY_OK;
    if (!dists_in) {
        if (int rc = check_scene("cosy_ransac_best", cand_poses, cand_mesh, pts_table, sym_table, n_cand, n_mesh, P, S)) return rc;
        COSY_REQUIRE(TC1C2, "cosy_ransac_best: null pointer");
    }
    COSY_REQUIRE(n_inliers && dists_sum && pair_hyp_off && pair_hyps && pair_off && tmatches && best_hyp && n_matches && match_cand1 &&
                     match_cand2, "cosy_ransac_best: null pointer");
    COSY_REQUIRE(hyp_dist_off || !dists_in, "cosy_ransac_best: a distance table needs hyp_dist_off");
    const RansacScene sc = {cand_poses, cand_mesh, pts_table, sym_table, nullptr, n_cand, n_mesh, P, S};
    hipLaunchKernelGGL(ransac_best_kernel, dim3(n_pairs), dim3(RANSAC_THREADS), sort_lds_bytes(max_tm), s, sc, TC1C2, H, n_inliers, dists_sum,
                       pair_hyp_off, pair_hyps, pair_off, (const int4*)tmatches, dist_threshold, n_min_inliers, skip_hypothesis_0 ? 1 : 0,
                       hyp_dist_off, dists_in, best_hyp, n_matches, match_cand1, match_cand2);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

}  // extern "C"
