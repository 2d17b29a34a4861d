// Training side of the detector: what torchvision 0.4.2 does between the heads' raw outputs and the five losses of Mask R-CNN (Matcher,
// BalancedPositiveNegativeSampler, BoxCoder.encode, RegionProposalNetwork.compute_loss, RoIHeads.select_training_samples, fastrcnn_loss,
// project_masks_on_boxes, maskrcnn_loss).  DESIGN.md section 23 states the contract; tests/dettrain_ref.py is the CPU twin.
//
//   dt_best_kernel       best[g] = max_j IoU[g,j] for allow_low_quality_matches: the image's ground truths in LDS, one candidate per thread
//                        (an anchor formed from its index, or a row of boxes), per ground truth a wave maximum over the IoU's bits, one LDS
//                        atomicMax per wave, one global atomicMax per workgroup and ground truth.  IoUs are >= +0, so bits order as values.
//   dt_match_kernel      the same IoUs again (the same bits): value and lowest argmax, the thresholds, the low-quality restore, the labels
//   dt_sample_kernel     ONE workgroup per image: radix select (four passes of 8 bits, per-wave LDS histograms) of the n_pos-th smallest key
//                        among the positives and of the n_neg-th among the negatives in the same passes, then ONE ordered compaction: sampled
//                        candidates in ascending index (ties at a cut: lower index first), and the sampled positives on their own
//   dt_rpn_loss_kernel   one thread per sampled anchor: label, encode (det_device.h's box_encode), both loss terms, both gradients into the NCHW planes
//   dt_roi_cands_kernel  proposals + ground truths -> the RoI side's candidates (padded rows)
//   dt_roi_gather_kernel the sampled rows: boxes, labels, clamped matched index, regression targets; the positives on their own
//   dt_count_kernel      N = rows with a label in [0, C)
//   dt_fastrcnn_kernel   one wave per row: softmax, cross-entropy term, smooth-L1 term, both gradient rows in full
//   dt_mask_kernel       one workgroup per positive RoI: the valid sample range of every bin of both axes in LDS, the M x M targets from
//                        the uint8 mask with the adaptive grid, BCE against mask_logits[r, label], the gradient row in full
//   dt_reduce_kernel     one workgroup per loss: the float64 sum of its terms in a fixed order, divided and rounded once
// Integer atomics only.  float32 with one rounding per operation: contraction is off (the pragma below and build.FILE_FLAGS).
#include <math.h>
#include "cosy_common.h"
#include "det_device.h"
#include "reduce_device.h"

#pragma clang fp contract(off)

namespace cosy {
namespace {

constexpr int DT_THREADS = 256;
constexpr int DT_SEL_THREADS = 1024;
constexpr int DT_SEL_WAVES = DT_SEL_THREADS / 64;

// where the candidates of the matcher come from: anchors formed from their index (boxes == nullptr) or N padded rows of boxes per image
struct Cands {
    const float* boxes;
    const int* counts;
    int N, L, A;
};

// anchor j of an image: the walk over the levels to its level and its index there, then anchor_box (det_device.h), the box rpn_decode_kernel decodes
__device__ __forceinline__ Box dt_anchor(const RpnLevels& lv, int L, int A, int j, int* level, int* index) {
    int l = 0, first = 0;
    for (; l < L - 1; ++l) {
        const int n = A * lv.H[l] * lv.W[l];
        if (j < first + n) break;
        first += n;
    }
    *level = l; *index = j - first;
    return anchor_box(lv, l, j - first, A);
}

// candidate j of image b; false: a padding row (or past the end), which takes no part
__device__ __forceinline__ bool dt_candidate(const RpnLevels& lv, const Cands& cd, int b, int j, Box* c) {
    if (j >= cd.N) return false;
    if (cd.boxes) {
        if (cd.counts && j >= cd.counts[b]) return false;
        *c = load_box(cd.boxes, (size_t)b * cd.N + j);
        return true;
    }
    int l, idx;
    *c = dt_anchor(lv, cd.L, cd.A, j, &l, &idx);
    return true;
}

// the matcher's IoU: box_iou(gt, candidate); NaN (0/0), a negative value (an inverted box) and -0 count as +0, so the bits order as the values
__device__ __forceinline__ float dt_iou(const Box& gt, const Box& c) {
    const float v = box_iou(gt, c);
    return v > 0.f ? v : 0.f;
}

// ground truths of image b into LDS; returns their number
__device__ __forceinline__ int dt_load_gt(const float* __restrict__ gt, const int* __restrict__ gt_off, int b, Box* s_gt, int* first) {
    const int g0 = gt_off[b];
    int G = gt_off[b + 1] - g0;
    G = G < 0 ? 0 : G > COSY_DT_MAX_GT ? COSY_DT_MAX_GT : G;
    for (int g = threadIdx.x; g < G; g += blockDim.x) s_gt[g] = load_box(gt, (size_t)g0 + g);
    *first = g0;
    return G;
}

__global__ __launch_bounds__(DT_THREADS) void dt_best_kernel(RpnLevels lv, Cands cd, const float* __restrict__ gt, const int* __restrict__ gt_off,
                                                             unsigned* __restrict__ best) {
    __shared__ Box s_gt[COSY_DT_MAX_GT];
    __shared__ unsigned s_best[COSY_DT_MAX_GT];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    int g0;
    const int G = dt_load_gt(gt, gt_off, b, s_gt, &g0);
    for (int g = tid; g < G; g += DT_THREADS) s_best[g] = 0u;
    __syncthreads();
    Box c = {0.f, 0.f, 0.f, 0.f};
    const bool real = dt_candidate(lv, cd, b, blockIdx.x * DT_THREADS + tid, &c);
    for (int g = 0; g < G; ++g) {                                  // (uniform: every lane takes part in the wave maximum)
        const unsigned bits = real ? __float_as_uint(dt_iou(s_gt[g], c)) : 0u;
        const unsigned m = wave_max(bits);
        if (lane == 0 && m > 0u) atomicMax(&s_best[g], m);
    }
    __syncthreads();
    for (int g = tid; g < G; g += DT_THREADS)
        if (s_best[g] > 0u) atomicMax(&best[g0 + g], s_best[g]);
}

__global__ __launch_bounds__(DT_THREADS) void dt_match_kernel(RpnLevels lv, Cands cd, const float* __restrict__ gt, const int* __restrict__ gt_off,
                                                              const int* __restrict__ gt_labels, const unsigned* __restrict__ best, float high,
                                                              float low, int* __restrict__ matched, float* __restrict__ matched_iou,
                                                              int* __restrict__ labels) {
    __shared__ Box s_gt[COSY_DT_MAX_GT];
    __shared__ unsigned s_best[COSY_DT_MAX_GT];
    const int b = blockIdx.y, tid = threadIdx.x, j = blockIdx.x * DT_THREADS + tid;
    int g0;
    const int G = dt_load_gt(gt, gt_off, b, s_gt, &g0);
    if (best)
        for (int g = tid; g < G; g += DT_THREADS) s_best[g] = best[g0 + g];
    __syncthreads();
    if (j >= cd.N) return;
    Box c = {0.f, 0.f, 0.f, 0.f};
    int m = -3;                                                    // a padding row
    float val = 0.f;
    if (dt_candidate(lv, cd, b, j, &c)) {
        int arg = 0;
        bool restore = false;
        val = -1.f;
        for (int g = 0; g < G; ++g) {
            const float v = dt_iou(s_gt[g], c);
            if (v > val) { val = v; arg = g; }                     // equal IoUs: the lowest g
            if (best && __float_as_uint(v) == s_best[g]) restore = true;
        }
        if (G == 0) val = 0.f;
        m = G == 0 ? -1 : val < low ? -1 : val < high ? -2 : arg;
        if (restore) m = arg;                                      // its ORIGINAL argmax, not the ground truth whose best it is
    }
    const size_t at = (size_t)b * cd.N + j;
    matched[at] = m;
    matched_iou[at] = val;
    if (labels) labels[at] = m >= 0 ? (gt_labels ? gt_labels[g0 + m] : 1) : m == -1 ? 0 : -1;
}

// ---- sampler ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DT_SEL_THREADS) void dt_sample_kernel(const int* __restrict__ labels, const int* __restrict__ keys, int N, int bs,
                                                                   int want_pos, int* __restrict__ samp_idx, int* __restrict__ samp_count,
                                                                   int* __restrict__ pos_idx, int* __restrict__ pos_count) {
    __shared__ unsigned hist[2][DT_SEL_WAVES][256];
    __shared__ unsigned w_tie[2][DT_SEL_WAVES], w_sel[2][DT_SEL_WAVES];
    __shared__ unsigned s_prefix[2], s_need[2];
    __shared__ int s_k[2];
    const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int* lab = labels + (size_t)b * N;
    const unsigned* key = (const unsigned*)keys + (size_t)b * N;
    unsigned prefix[2] = {0u, 0u}, need[2] = {0u, 0u};
    int k[2] = {0, 0};
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        for (int i = tid; i < 2 * DT_SEL_WAVES * 256; i += DT_SEL_THREADS) (&hist[0][0][0])[i] = 0u;
        __syncthreads();
        for (int i = tid; i < N; i += DT_SEL_THREADS) {
            const int y = lab[i];
            if (y < 0) continue;
            const int c = y >= 1 ? 0 : 1;                          // class 0: positives, class 1: negatives
            const unsigned u = key[i];
            if (pass > 0 && ((u >> (shift + 8)) != prefix[c] || k[c] == 0)) continue;
            atomicAdd(&hist[c][wave][(u >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid < 512) {
            const int c = tid >> 8, q = tid & 255;
            unsigned t = 0u;
            for (int w = 0; w < DT_SEL_WAVES; ++w) t += hist[c][w][q];
            hist[c][0][q] = t;
        }
        __syncthreads();
        if (tid == 0) {
            if (pass == 0) {                                       // every positive and every negative is in the first histograms
                unsigned P = 0u, Nn = 0u;
                for (int q = 0; q < 256; ++q) { P += hist[0][0][q]; Nn += hist[1][0][q]; }
                const int n_pos = (int)(P < (unsigned)want_pos ? P : (unsigned)want_pos);
                const unsigned room = (unsigned)(bs - n_pos);
                s_k[0] = n_pos;
                s_k[1] = (int)(Nn < room ? Nn : room);
                s_need[0] = (unsigned)s_k[0]; s_need[1] = (unsigned)s_k[1];
            }
            for (int c = 0; c < 2; ++c) {
                if (s_k[c] == 0) { s_prefix[c] = 0u; continue; }
                unsigned cum = 0u;
                const unsigned want = s_need[c];
                int digit = 255;
                for (int q = 0; q < 256; ++q) {                    // ascending: the smallest keys are taken
                    const unsigned n = hist[c][0][q];
                    if (cum + n >= want) { digit = q; break; }
                    cum += n;
                }
                s_need[c] = want - cum;                            // how many of the keys with this prefix are still wanted
                s_prefix[c] = (prefix[c] << 8) | (unsigned)digit;
            }
        }
        __syncthreads();
        for (int c = 0; c < 2; ++c) { prefix[c] = s_prefix[c]; need[c] = s_need[c]; k[c] = s_k[c]; }
    }
    const int total = k[0] + k[1];
    if (tid == 0) { samp_count[b] = total; pos_count[b] = k[0]; }
    // prefix[c] is the k[c]-th smallest key of class c: every key below it is taken, and the need[c] lowest-index candidates at it
    int* out = samp_idx + (size_t)b * bs;
    int* out_pos = pos_idx + (size_t)b * want_pos;
    unsigned base_tie[2] = {0u, 0u}, base_sel[2] = {0u, 0u};      // base_sel[0]: all sampled so far, [1]: the positives among them
    for (int start = 0; start < N && total > 0; start += DT_SEL_THREADS) {
        const int i = start + tid;
        int c = -1;
        bool below = false, tie = false;
        if (i < N) {
            const int y = lab[i];
            c = y < 0 ? -1 : y >= 1 ? 0 : 1;
            if (c >= 0 && k[c] > 0) {
                const unsigned u = key[i];
                below = u < prefix[c]; tie = u == prefix[c];
            }
        }
        const unsigned long long bt0 = __ballot(tie && c == 0), bt1 = __ballot(tie && c == 1);
        if (lane == 0) { w_tie[0][wave] = (unsigned)__popcll(bt0); w_tie[1][wave] = (unsigned)__popcll(bt1); }
        __syncthreads();
        unsigned off[2] = {0u, 0u}, tot[2] = {0u, 0u};
        for (int w = 0; w < DT_SEL_WAVES; ++w)
            for (int q = 0; q < 2; ++q) {
                const unsigned n = w_tie[q][w];
                if (w < wave) off[q] += n;
                tot[q] += n;
            }
        const unsigned long long lower = (1ULL << lane) - 1ULL;
        bool take = below;
        if (tie) take = base_tie[c] + off[c] + (unsigned)__popcll((c == 0 ? bt0 : bt1) & lower) < need[c];
        const unsigned long long bs_all = __ballot(take), bs_pos = __ballot(take && c == 0);
        if (lane == 0) { w_sel[0][wave] = (unsigned)__popcll(bs_all); w_sel[1][wave] = (unsigned)__popcll(bs_pos); }
        __syncthreads();
        unsigned soff[2] = {0u, 0u}, stot[2] = {0u, 0u};
        for (int w = 0; w < DT_SEL_WAVES; ++w)
            for (int q = 0; q < 2; ++q) {
                const unsigned n = w_sel[q][w];
                if (w < wave) soff[q] += n;
                stot[q] += n;
            }
        if (take) {
            const unsigned p = base_sel[0] + soff[0] + (unsigned)__popcll(bs_all & lower);
            if (p < (unsigned)bs) out[p] = i;
            if (c == 0) {
                const unsigned pp = base_sel[1] + soff[1] + (unsigned)__popcll(bs_pos & lower);
                if (pp < (unsigned)want_pos) out_pos[pp] = i;
            }
        }
        for (int q = 0; q < 2; ++q) { base_tie[q] += tot[q]; base_sel[q] += stot[q]; }
        if (base_sel[0] >= (unsigned)total) break;                 // (uniform)
    }
}

// ---- the loss terms (the encode is box_encode of det_device.h, next to the decode it inverts) ---------------------------------------------
// smooth-L1 of torch (beta = 0: plain L1) and its derivative
__device__ __forceinline__ float smooth_l1(float x, float beta) {
    const float ax = fabsf(x);
    return ax < beta ? __fdiv_rn(__fmul_rn(__fmul_rn(0.5f, x), x), beta) : __fsub_rn(ax, __fmul_rn(0.5f, beta));
}
__device__ __forceinline__ float smooth_l1_grad(float x, float beta) {
    return fabsf(x) < beta ? __fdiv_rn(x, beta) : x > 0.f ? 1.f : x < 0.f ? -1.f : 0.f;
}
// binary cross-entropy with logits in the stable form, and the sigmoid without overflow
__device__ __forceinline__ float bce_logits(float x, float y) {
    return __fadd_rn(__fsub_rn(x > 0.f ? x : 0.f, __fmul_rn(x, y)), log1pf(expf(-fabsf(x))));
}
__device__ __forceinline__ float sigmoid(float x) {
    const float e = expf(-fabsf(x));
    return x >= 0.f ? __fdiv_rn(1.f, __fadd_rn(1.f, e)) : __fdiv_rn(e, __fadd_rn(1.f, e));
}

// sum of counts[0 .. n) clamped to [0, cap]
__device__ __forceinline__ int dt_total(const int* __restrict__ counts, int n, int cap) {
    int t = 0;
    for (int i = 0; i < n; ++i) { const int c = counts[i]; t += c < 0 ? 0 : c > cap ? cap : c; }
    return t;
}

__global__ __launch_bounds__(DT_THREADS) void dt_encode_kernel(const float* __restrict__ ref, const float* __restrict__ boxes, long n, float wx, float wy,
                                                               float ww, float wh, float* __restrict__ out) {
    const long at = (long)blockIdx.x * DT_THREADS + threadIdx.x;
    if (at >= n) return;
    float t[4];
    box_encode(load_box(ref, at), load_box(boxes, at), wx, wy, ww, wh, t);
    for (int c = 0; c < 4; ++c) out[4 * at + c] = t[c];
}

// the gradient tensors of the RPN head's outputs, level by level (the layouts of RpnLevels::objectness / deltas)
struct RpnGrads { float* objectness[COSY_RPN_MAX_LEVELS]; float* deltas[COSY_RPN_MAX_LEVELS]; };

__global__ __launch_bounds__(DT_THREADS) void dt_rpn_loss_kernel(RpnLevels lv, RpnGrads gr, int L, int A, int B, int N, int bs,
                                                                 const int* __restrict__ samp_idx, const int* __restrict__ samp_count,
                                                                 const int* __restrict__ matched, const float* __restrict__ gt,
                                                                 const int* __restrict__ gt_off, double* __restrict__ terms) {
    const long at = (long)blockIdx.x * DT_THREADS + threadIdx.x;
    if (at >= (long)B * bs) return;
    const int b = (int)(at / bs), s = (int)(at - (long)b * bs);
    const float n_s = (float)dt_total(samp_count, B, bs);
    double t_obj = 0., t_box = 0.;
    const int j = s < samp_count[b] ? samp_idx[at] : -1;
    if (j >= 0 && j < N) {                                         // an index read from memory: checked before it addresses anything
        const int m = matched[(size_t)b * N + j];
        const int g0 = gt_off[b], G = gt_off[b + 1] - g0;
        if (m >= -1 && m < G) {
            int l, idx;
            const Box anc = dt_anchor(lv, L, A, j, &l, &idx);
            const int HW = lv.H[l] * lv.W[l], pos = idx / A, a = idx - pos * A;
            const size_t o_at = ((size_t)b * A + a) * HW + pos;
            const float y = m >= 0 ? 1.f : 0.f, x = lv.objectness[l][o_at];
            t_obj = (double)bce_logits(x, y);
            gr.objectness[l][o_at] = __fdiv_rn(__fsub_rn(sigmoid(x), y), n_s);
            if (m >= 0) {
                float t[4];
                box_encode(load_box(gt, (size_t)g0 + m), anc, 1.f, 1.f, 1.f, 1.f, t);
                for (int c = 0; c < 4; ++c) {
                    const size_t d_at = ((size_t)b * 4 * A + 4 * a + c) * HW + pos;
                    const float diff = __fsub_rn(lv.deltas[l][d_at], t[c]);
                    t_box += (double)smooth_l1(diff, 0.f);
                    gr.deltas[l][d_at] = __fdiv_rn(smooth_l1_grad(diff, 0.f), n_s);
                }
            }
        }
    }
    terms[at] = t_obj;
    terms[(size_t)B * bs + at] = t_box;
}

// out[k] = float(sum of terms[k][0 .. n) / denominator), 0 when the denominator is 0; the denominator: mult x (the clamped sum of `counts`, or
// `fixed` without counts).  Thread t adds the terms t, t + 256, ... in that order, then block_sum256: the same bits on every call.
__global__ __launch_bounds__(DT_THREADS) void dt_reduce_kernel(const double* __restrict__ terms, long n, const int* __restrict__ counts, int n_counts,
                                                               int cap, long fixed, long mult, float* __restrict__ out) {
    __shared__ double scratch[4];
    const double* t = terms + (size_t)blockIdx.x * n;
    double acc = 0.;
    for (long i = threadIdx.x; i < n; i += DT_THREADS) acc += t[i];
    const double sum = block_sum256(acc, scratch);
    const long denom = mult * (counts ? (long)dt_total(counts, n_counts, cap) : fixed);
    if (threadIdx.x == 0) out[blockIdx.x] = denom > 0 ? (float)(sum / (double)denom) : 0.f;
}

// ---- RoI training samples ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DT_THREADS) void dt_roi_cands_kernel(const float* __restrict__ proposals, const int* __restrict__ counts, int post,
                                                                  const float* __restrict__ gt, const int* __restrict__ gt_off, int B, int rows,
                                                                  float* __restrict__ cand, int* __restrict__ cand_count) {
    const long at = (long)blockIdx.x * DT_THREADS + threadIdx.x;
    if (at >= (long)B * rows) return;
    const int b = (int)(at / rows), j = (int)(at - (long)b * rows);
    int n = counts[b];
    n = n < 0 ? 0 : n > post ? post : n;
    const int g0 = gt_off[b];
    int G = gt_off[b + 1] - g0;
    G = G < 0 ? 0 : G > rows - post ? rows - post : G;
    Box v = {0.f, 0.f, 0.f, 0.f};
    if (j < n) v = load_box(proposals, (size_t)b * post + j);
    else if (j < n + G) v = load_box(gt, (size_t)g0 + j - n);
    store_box(cand, at, v);
    if (j == 0) cand_count[b] = n + G;
}

__global__ __launch_bounds__(DT_THREADS) void dt_roi_gather_kernel(const float* __restrict__ cand, int rows, const int* __restrict__ matched,
                                                                   const int* __restrict__ labels, const int* __restrict__ samp_idx,
                                                                   const int* __restrict__ samp_count, const int* __restrict__ pos_idx,
                                                                   const int* __restrict__ pos_count, const float* __restrict__ gt,
                                                                   const int* __restrict__ gt_off, int B, int bs, int want_pos, float wx, float wy,
                                                                   float ww, float wh, float* __restrict__ out_boxes, int* __restrict__ out_labels,
                                                                   int* __restrict__ out_matched, float* __restrict__ out_targets,
                                                                   float* __restrict__ pos_boxes, int* __restrict__ pos_labels,
                                                                   int* __restrict__ pos_matched) {
    const long at = (long)blockIdx.x * DT_THREADS + threadIdx.x;
    const int per = bs + want_pos;
    if (at >= (long)B * per) return;
    const int b = (int)(at / per), s = (int)(at - (long)b * per);
    const bool all = s < bs;
    const int r = all ? s : s - bs;
    const int cnt = all ? samp_count[b] : pos_count[b];
    const int j = r < cnt ? (all ? samp_idx[(size_t)b * bs + r] : pos_idx[(size_t)b * want_pos + r]) : -1;
    const int g0 = gt_off[b], G = gt_off[b + 1] - g0;
    Box v = {0.f, 0.f, 0.f, 0.f};
    float t[4] = {0.f, 0.f, 0.f, 0.f};
    int label = -1, m = 0;
    if (j >= 0 && j < rows) {                                      // an index read from memory: checked before it addresses anything
        const size_t c_at = (size_t)b * rows + j;
        const int raw = matched[c_at];
        m = raw < 0 ? 0 : raw;                                     // the CLAMPED index, as torchvision keeps it
        if (m < G) {
            v = load_box(cand, c_at);
            label = labels[c_at];
            if (all) box_encode(load_box(gt, (size_t)g0 + m), v, wx, wy, ww, wh, t);
        } else m = 0;
    }
    if (all) {
        const size_t o = (size_t)b * bs + r;
        store_box(out_boxes, o, v);
        for (int c = 0; c < 4; ++c) out_targets[4 * o + c] = t[c];
        out_labels[o] = label; out_matched[o] = m;
    } else {
        const size_t o = (size_t)b * want_pos + r;
        store_box(pos_boxes, o, v);
        pos_labels[o] = label; pos_matched[o] = m;
    }
}

// ---- Fast R-CNN loss ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DT_THREADS) void dt_count_kernel(const int* __restrict__ labels, int R, int C, int* __restrict__ n_real) {
    __shared__ int scratch[4];
    int n = 0;
    for (int r = threadIdx.x; r < R; r += DT_THREADS) n += labels[r] >= 0 && labels[r] < C;
    n = block_sum256(n, scratch);
    if (threadIdx.x == 0) *n_real = n;
}

__global__ __launch_bounds__(DT_THREADS) void dt_fastrcnn_kernel(const float* __restrict__ logits, const float* __restrict__ box_regression,
                                                                 const int* __restrict__ labels, const float* __restrict__ targets, int R, int C,
                                                                 const int* __restrict__ n_real, float* __restrict__ grad_logits,
                                                                 float* __restrict__ grad_box, double* __restrict__ terms) {
    const int r = blockIdx.x * (DT_THREADS / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= R) return;                                            // (a wave as a whole)
    const int label = labels[r];
    const float n = (float)*n_real;
    const float* z = logits + (size_t)r * C;
    float* gz = grad_logits + (size_t)r * C;
    float* gb = grad_box + (size_t)r * 4 * C;
    for (int c = lane; c < 4 * C; c += 64)                        // every entry but the four the label's smooth-L1 writes below
        if (!(label > 0 && (c >> 2) == label)) gb[c] = 0.f;
    if (label < 0 || label >= C) {                                 // padding: neither summed nor counted
        for (int c = lane; c < C; c += 64) gz[c] = 0.f;
        if (lane == 0) { terms[r] = 0.; terms[(size_t)R + r] = 0.; }
        return;
    }
    float mx = -INFINITY;
    for (int c = lane; c < C; c += 64) mx = fmaxf(mx, z[c]);
    mx = wave_max(mx);
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s = __fadd_rn(s, expf(__fsub_rn(z[c], mx)));
    s = wave_sum(s);
    for (int c = lane; c < C; c += 64) {
        const float p = __fdiv_rn(expf(__fsub_rn(z[c], mx)), s);
        gz[c] = __fdiv_rn(c == label ? __fsub_rn(p, 1.f) : p, n);
    }
    float l1 = 0.f;
    if (label > 0 && lane < 4) {
        const size_t at = (size_t)r * 4 * C + 4 * label + lane;
        const float diff = __fsub_rn(box_regression[at], targets[4 * (size_t)r + lane]);
        l1 = smooth_l1(diff, 1.f);
        grad_box[at] = __fdiv_rn(smooth_l1_grad(diff, 1.f), n);
    }
    const float a0 = __shfl(l1, 0, 64), a1 = __shfl(l1, 1, 64), a2 = __shfl(l1, 2, 64), a3 = __shfl(l1, 3, 64);
    if (lane == 0) {
        terms[r] = (double)__fsub_rn(logf(s), __fsub_rn(z[label], mx));
        terms[(size_t)R + r] = (((double)a0 + (double)a1) + (double)a2) + (double)a3;
    }
}

// ---- mask targets and loss ---------------------------------------------------------------------------------------------------------------
// the adaptive grid of one axis: size = max(extent, 1), bin = size / M, g = ceil(bin) capped at COSY_DT_MAX_GRID (NaN: 1)
__device__ __forceinline__ void dt_axis(float lo, float hi, int M, float* bin, int* g) {
    const float ext = __fsub_rn(hi, lo);
    const float size = ext > 1.f ? ext : 1.f;
    *bin = __fdiv_rn(size, (float)M);
    const float gf = ceilf(*bin);
    *g = gf >= 1.f ? (gf > (float)COSY_DT_MAX_GRID ? COSY_DT_MAX_GRID : (int)gf) : 1;
}

__global__ __launch_bounds__(DT_THREADS) void dt_mask_kernel(const long long* __restrict__ mask_ptr, const int* __restrict__ mask_dims, int B,
                                                             const float* __restrict__ boxes, const int* __restrict__ labels,
                                                             const int* __restrict__ matched, const int* __restrict__ pos_count, int rows, int R,
                                                             const float* __restrict__ logits, int C, int M, float* __restrict__ grad,
                                                             float* __restrict__ targets_out, double* __restrict__ partial) {
    __shared__ int s_first[2][COSY_DT_MAX_M], s_last[2][COSY_DT_MAX_M];
    __shared__ double scratch[4];
    const int r = blockIdx.x, tid = threadIdx.x, MM = M * M;
    // everything up to the ranges is uniform over the workgroup
    const int img = r / rows;
    bool real = img < B && (!pos_count || r - img * rows < pos_count[img]);
    const int g_idx = matched[r], label = labels ? labels[r] : 0;
    int H = 0, W = 0;
    if (real) {
        H = mask_dims[3 * img + 1]; W = mask_dims[3 * img + 2];
        real = g_idx >= 0 && g_idx < mask_dims[3 * img] && H >= 1 && W >= 1 && (long)H * W < (1L << 30) && (!logits || (label >= 0 && label < C));
    }
    if (grad)                                                      // the whole gradient row: zeros outside the label's channel
        for (int o = tid; o < C * MM; o += DT_THREADS)
            if (!real || o / MM != label) grad[(size_t)r * C * MM + o] = 0.f;
    if (!real) {
        if (targets_out)
            for (int o = tid; o < MM; o += DT_THREADS) targets_out[(size_t)r * MM + o] = 0.f;
        if (partial && tid == 0) partial[r] = 0.;
        return;
    }
    const Box roi = load_box(boxes, r);
    float bin_h, bin_w;
    int gh, gw;
    dt_axis(roi.y1, roi.y2, M, &bin_h, &gh);
    dt_axis(roi.x1, roi.x2, M, &bin_w, &gw);
    for (int q = tid; q < 2 * M; q += DT_THREADS) {                // the first and last sample of every bin that lies inside [-1, size]
        const int axis = q / M, p = q - axis * M, g = axis ? gw : gh;
        int first = g, last = -1;
        for (int i = 0; i < g; ++i)
            if (msroi_tap(axis ? roi.x1 : roi.y1, axis ? bin_w : bin_h, p, i, g, axis ? W : H).lo >= 0) { first = i < first ? i : first; last = i; }
        s_first[axis][p] = first; s_last[axis][p] = last;
    }
    __syncthreads();
    const unsigned char* mask = (const unsigned char*)mask_ptr[img] + (size_t)g_idx * H * W;
    const float count = __fmul_rn((float)gh, (float)gw);
    const float denom = (float)((long)(pos_count ? dt_total(pos_count, B, rows) : R) * MM);
    double acc_loss = 0.;
    for (int o = tid; o < MM; o += DT_THREADS) {
        const int ph = o / M, pw = o - ph * M;
        float acc = 0.f;
        for (int iy = s_first[0][ph]; iy <= s_last[0][ph]; ++iy) {
            const Tap ty = msroi_tap(roi.y1, bin_h, ph, iy, gh, H);
            if (ty.lo < 0) continue;
            for (int ix = s_first[1][pw]; ix <= s_last[1][pw]; ++ix) {
                const Tap tx = msroi_tap(roi.x1, bin_w, pw, ix, gw, W);
                if (tx.lo < 0) continue;
                const float w1 = __fmul_rn(ty.wh, tx.wh), w2 = __fmul_rn(ty.wh, tx.wl), w3 = __fmul_rn(ty.wl, tx.wh), w4 = __fmul_rn(ty.wl, tx.wl);
                float v = __fmul_rn(w1, (float)mask[ty.lo * W + tx.lo]);
                v = __fadd_rn(v, __fmul_rn(w2, (float)mask[ty.lo * W + tx.hi]));
                v = __fadd_rn(v, __fmul_rn(w3, (float)mask[ty.hi * W + tx.lo]));
                v = __fadd_rn(v, __fmul_rn(w4, (float)mask[ty.hi * W + tx.hi]));
                acc = __fadd_rn(acc, v);
            }
        }
        const float t = __fdiv_rn(acc, count);
        if (targets_out) targets_out[(size_t)r * MM + o] = t;
        if (logits) {
            const size_t at = ((size_t)r * C + label) * MM + o;
            const float x = logits[at];
            acc_loss += (double)bce_logits(x, t);
            if (grad) grad[at] = __fdiv_rn(__fsub_rn(sigmoid(x), t), denom);
        }
    }
    if (partial) {
        const double sum = block_sum256(acc_loss, scratch);
        if (tid == 0) partial[r] = sum;
    }
}

int dt_batch_args(const char* fn, int B, long rows) {
    COSY_REQUIRE(B >= 1 && B <= ARENA_MAX_IMAGES, "%s: B=%d outside [1, %d] images per call", fn, B, ARENA_MAX_IMAGES);
    COSY_REQUIRE(rows >= 1 && (long)B * rows < (1L << 30), "%s: %ld rows per image, %d images: outside [1, 2^30) rows", fn, rows, B);
    return COSY_OK;
}

}  // namespace
}  // namespace cosy

using namespace cosy;

extern "C" {

int cosy_dt_match(const cosy_rpn_levels_t* levels, int L, int A, const float* cand_boxes, const int* cand_counts, int N, int B, const float* gt_boxes,
                  const int* gt_off, const int* gt_labels, int G_max, int G_total, float high, float low, int allow_low_quality, unsigned* best_ws,
                  int* matched, float* matched_iou, int* labels, cosy_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    if (int rc = dt_batch_args("cosy_dt_match", B, N)) return rc;
    Cands cd = {cand_boxes, cand_counts, N, L, A};
    RpnLevels lv = {};
    if (!cand_boxes) {
        long total;
        if (int rc = rpn_levels_args("cosy_dt_match", levels, L, A, &total)) return rc;
        COSY_REQUIRE(total == N, "cosy_dt_match: N=%d, the levels hold %ld anchors", N, total);
        COSY_REQUIRE(cand_counts == nullptr, "cosy_dt_match: cand_counts go with cand_boxes, not with anchors");
        lv = *levels;
    }
    COSY_REQUIRE(G_max >= 1 && G_max <= COSY_DT_MAX_GT && G_total >= G_max, "cosy_dt_match: G_max=%d outside [1, %d] ground truths per image (G_total=%d)",
                 G_max, COSY_DT_MAX_GT, G_total);
    COSY_REQUIRE(low <= high, "cosy_dt_match: low=%g above high=%g (or NaN)", (double)low, (double)high);
    COSY_REQUIRE_PTR("cosy_dt_match", gt_boxes); COSY_REQUIRE_PTR("cosy_dt_match", gt_off); COSY_REQUIRE_PTR("cosy_dt_match", matched);
    COSY_REQUIRE_PTR("cosy_dt_match", matched_iou);
    COSY_REQUIRE(!allow_low_quality || best_ws != nullptr, "cosy_dt_match: null best_ws with allow_low_quality");
    COSY_REQUIRE(gt_labels == nullptr || labels != nullptr, "cosy_dt_match: gt_labels without labels");
    const dim3 grid(cdiv(N, DT_THREADS), B);
    if (allow_low_quality) {
        COSY_CHECK_HIP(hipMemsetAsync(best_ws, 0, sizeof(unsigned) * (size_t)G_total, s));
        hipLaunchKernelGGL(dt_best_kernel, grid, dim3(DT_THREADS), 0, s, lv, cd, gt_boxes, gt_off, best_ws);
        COSY_CHECK_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(dt_match_kernel, grid, dim3(DT_THREADS), 0, s, lv, cd, gt_boxes, gt_off, gt_labels, allow_low_quality ? best_ws : nullptr, high, low,
                       matched, matched_iou, labels);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

int cosy_dt_sample(const int* labels, const int* keys, int N, int B, int batch_size_per_image, int max_positives, int* samp_idx, int* samp_count,
                   int* pos_idx, int* pos_count, cosy_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    if (int rc = dt_batch_args("cosy_dt_sample", B, N)) return rc;
    COSY_REQUIRE(batch_size_per_image >= 1 && batch_size_per_image <= COSY_DT_MAX_BATCH && max_positives >= 0 && max_positives <= batch_size_per_image,
                 "cosy_dt_sample: batch_size_per_image=%d outside [1, %d] or max_positives=%d outside [0, batch_size_per_image]", batch_size_per_image,
                 COSY_DT_MAX_BATCH, max_positives);
    COSY_REQUIRE_PTR("cosy_dt_sample", labels); COSY_REQUIRE_PTR("cosy_dt_sample", keys); COSY_REQUIRE_PTR("cosy_dt_sample", samp_idx);
    COSY_REQUIRE_PTR("cosy_dt_sample", samp_count); COSY_REQUIRE_PTR("cosy_dt_sample", pos_idx); COSY_REQUIRE_PTR("cosy_dt_sample", pos_count);
    hipLaunchKernelGGL(dt_sample_kernel, dim3(B), dim3(DT_SEL_THREADS), 0, s, labels, keys, N, batch_size_per_image, max_positives, samp_idx, samp_count,
                       pos_idx, pos_count);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

int cosy_dt_encode(const float* reference_boxes, const float* boxes, long n, float wx, float wy, float ww, float wh, float* out, cosy_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    COSY_REQUIRE(n >= 0 && n < (1L << 29), "cosy_dt_encode: n=%ld outside [0, 2^29)", n);
    if (n == 0) return COSY_OK;
    COSY_REQUIRE_PTR("cosy_dt_encode", reference_boxes); COSY_REQUIRE_PTR("cosy_dt_encode", boxes); COSY_REQUIRE_PTR("cosy_dt_encode", out);
    hipLaunchKernelGGL(dt_encode_kernel, dim3(cdiv(n, DT_THREADS)), dim3(DT_THREADS), 0, s, reference_boxes, boxes, n, wx, wy, ww, wh, out);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

int cosy_dt_rpn_loss(const cosy_rpn_levels_t* levels, const cosy_rpn_levels_t* grads, int L, int A, int B, int batch_size_per_image, const int* samp_idx,
                     const int* samp_count, const int* matched, const float* gt_boxes, const int* gt_off, double* terms_ws, float* losses,
                     cosy_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    long total;
    if (int rc = rpn_levels_args("cosy_dt_rpn_loss", levels, L, A, &total)) return rc;
    if (int rc = dt_batch_args("cosy_dt_rpn_loss", B, total)) return rc;
    COSY_REQUIRE(batch_size_per_image >= 1 && batch_size_per_image <= COSY_DT_MAX_BATCH, "cosy_dt_rpn_loss: batch_size_per_image=%d outside [1, %d]",
                 batch_size_per_image, COSY_DT_MAX_BATCH);
    COSY_REQUIRE_PTR("cosy_dt_rpn_loss", grads);
    for (int l = 0; l < L; ++l)
        COSY_REQUIRE(levels->objectness[l] && levels->deltas[l] && grads->objectness[l] && grads->deltas[l],
                     "cosy_dt_rpn_loss: null objectness / deltas or their gradients of level %d", l);
    COSY_REQUIRE_PTR("cosy_dt_rpn_loss", samp_idx); COSY_REQUIRE_PTR("cosy_dt_rpn_loss", samp_count); COSY_REQUIRE_PTR("cosy_dt_rpn_loss", matched);
    COSY_REQUIRE_PTR("cosy_dt_rpn_loss", gt_boxes); COSY_REQUIRE_PTR("cosy_dt_rpn_loss", gt_off); COSY_REQUIRE_PTR("cosy_dt_rpn_loss", terms_ws);
    COSY_REQUIRE_PTR("cosy_dt_rpn_loss", losses);
    const long n = (long)B * batch_size_per_image;
    RpnGrads gr = {};
    for (int l = 0; l < L; ++l) { gr.objectness[l] = (float*)grads->objectness[l]; gr.deltas[l] = (float*)grads->deltas[l]; }
    hipLaunchKernelGGL(dt_rpn_loss_kernel, dim3(cdiv(n, DT_THREADS)), dim3(DT_THREADS), 0, s, *levels, gr, L, A, B, (int)total, batch_size_per_image,
                       samp_idx, samp_count, matched, gt_boxes, gt_off, terms_ws);
    COSY_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(dt_reduce_kernel, dim3(2), dim3(DT_THREADS), 0, s, terms_ws, n, samp_count, B, batch_size_per_image, 0L, 1L, losses);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

int cosy_dt_roi_candidates(const float* proposals, const int* counts, int rows_per_image, const float* gt_boxes, const int* gt_off, int B, int G_max,
                           float* cand_boxes, int* cand_counts, cosy_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    if (int rc = dt_batch_args("cosy_dt_roi_candidates", B, (long)rows_per_image + (G_max > 0 ? G_max : 0))) return rc;
    COSY_REQUIRE(rows_per_image >= 0 && G_max >= 1 && G_max <= COSY_DT_MAX_GT, "cosy_dt_roi_candidates: rows_per_image=%d, G_max=%d outside [1, %d]",
                 rows_per_image, G_max, COSY_DT_MAX_GT);
    COSY_REQUIRE(rows_per_image == 0 || proposals != nullptr, "cosy_dt_roi_candidates: null proposals");
    COSY_REQUIRE_PTR("cosy_dt_roi_candidates", counts); COSY_REQUIRE_PTR("cosy_dt_roi_candidates", gt_boxes); COSY_REQUIRE_PTR("cosy_dt_roi_candidates", gt_off);
    COSY_REQUIRE_PTR("cosy_dt_roi_candidates", cand_boxes); COSY_REQUIRE_PTR("cosy_dt_roi_candidates", cand_counts);
    const int rows = rows_per_image + G_max;
    hipLaunchKernelGGL(dt_roi_cands_kernel, dim3(cdiv((long)B * rows, DT_THREADS)), dim3(DT_THREADS), 0, s, proposals, counts, rows_per_image, gt_boxes,
                       gt_off, B, rows, cand_boxes, cand_counts);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

int cosy_dt_roi_gather(const float* cand_boxes, int N, const int* matched, const int* labels, const int* samp_idx, const int* samp_count,
                       const int* pos_idx, const int* pos_count, const float* gt_boxes, const int* gt_off, int B, int batch_size_per_image,
                       int max_positives, float wx, float wy, float ww, float wh, float* boxes, int* out_labels, int* out_matched, float* targets,
                       float* pos_boxes, int* pos_labels, int* pos_matched, cosy_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    if (int rc = dt_batch_args("cosy_dt_roi_gather", B, N)) return rc;
    COSY_REQUIRE(batch_size_per_image >= 1 && batch_size_per_image <= COSY_DT_MAX_BATCH && max_positives >= 0 && max_positives <= batch_size_per_image,
                 "cosy_dt_roi_gather: batch_size_per_image=%d outside [1, %d] or max_positives=%d outside [0, batch_size_per_image]", batch_size_per_image,
                 COSY_DT_MAX_BATCH, max_positives);
    COSY_REQUIRE_PTR("cosy_dt_roi_gather", cand_boxes); COSY_REQUIRE_PTR("cosy_dt_roi_gather", matched); COSY_REQUIRE_PTR("cosy_dt_roi_gather", labels);
    COSY_REQUIRE_PTR("cosy_dt_roi_gather", samp_idx); COSY_REQUIRE_PTR("cosy_dt_roi_gather", samp_count); COSY_REQUIRE_PTR("cosy_dt_roi_gather", pos_idx);
    COSY_REQUIRE_PTR("cosy_dt_roi_gather", pos_count); COSY_REQUIRE_PTR("cosy_dt_roi_gather", gt_boxes); COSY_REQUIRE_PTR("cosy_dt_roi_gather", gt_off);
    COSY_REQUIRE_PTR("cosy_dt_roi_gather", boxes); COSY_REQUIRE_PTR("cosy_dt_roi_gather", out_labels); COSY_REQUIRE_PTR("cosy_dt_roi_gather", out_matched);
    COSY_REQUIRE_PTR("cosy_dt_roi_gather", targets);
    COSY_REQUIRE(max_positives == 0 || (pos_boxes && pos_labels && pos_matched), "cosy_dt_roi_gather: null pos_boxes / pos_labels / pos_matched");
    const long n = (long)B * (batch_size_per_image + max_positives);
    hipLaunchKernelGGL(dt_roi_gather_kernel, dim3(cdiv(n, DT_THREADS)), dim3(DT_THREADS), 0, s, cand_boxes, N, matched, labels, samp_idx, samp_count, pos_idx,
                       pos_count, gt_boxes, gt_off, B, batch_size_per_image, max_positives, wx, wy, ww, wh, boxes, out_labels, out_matched, targets,
                       pos_boxes, pos_labels, pos_matched);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

int cosy_dt_fastrcnn_loss(const float* class_logits, const float* box_regression, const int* labels, const float* regression_targets, int R, int C,
                          int* n_real_ws, double* terms_ws, float* grad_logits, float* grad_box, float* losses, cosy_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    COSY_REQUIRE(R >= 1 && R < (1 << 22), "cosy_dt_fastrcnn_loss: R=%d outside [1, 2^22) rows", R);
    COSY_REQUIRE(C >= 2 && C <= COSY_DT_MAX_CLASSES, "cosy_dt_fastrcnn_loss: C=%d outside [2, %d] classes", C, COSY_DT_MAX_CLASSES);
    COSY_REQUIRE_PTR("cosy_dt_fastrcnn_loss", class_logits); COSY_REQUIRE_PTR("cosy_dt_fastrcnn_loss", box_regression);
    COSY_REQUIRE_PTR("cosy_dt_fastrcnn_loss", labels); COSY_REQUIRE_PTR("cosy_dt_fastrcnn_loss", regression_targets);
    COSY_REQUIRE_PTR("cosy_dt_fastrcnn_loss", n_real_ws); COSY_REQUIRE_PTR("cosy_dt_fastrcnn_loss", terms_ws);
    COSY_REQUIRE_PTR("cosy_dt_fastrcnn_loss", grad_logits); COSY_REQUIRE_PTR("cosy_dt_fastrcnn_loss", grad_box); COSY_REQUIRE_PTR("cosy_dt_fastrcnn_loss", losses);
    hipLaunchKernelGGL(dt_count_kernel, dim3(1), dim3(DT_THREADS), 0, s, labels, R, C, n_real_ws);
    COSY_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(dt_fastrcnn_kernel, dim3(cdiv(R, DT_THREADS / 64)), dim3(DT_THREADS), 0, s, class_logits, box_regression, labels, regression_targets, R,
                       C, n_real_ws, grad_logits, grad_box, terms_ws);
    COSY_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(dt_reduce_kernel, dim3(2), dim3(DT_THREADS), 0, s, terms_ws, (long)R, n_real_ws, 1, R, 0L, 1L, losses);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

int cosy_dt_mask_loss(const long long* mask_ptr, const int* mask_dims, int B, const float* boxes, const int* labels, const int* matched,
                      const int* pos_count, int rows_per_image, const float* mask_logits, int C, int M, double* partial_ws, float* grad, float* targets_out,
                      float* loss, cosy_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    if (int rc = dt_batch_args("cosy_dt_mask_loss", B, rows_per_image)) return rc;
    COSY_REQUIRE(M >= 1 && M <= COSY_DT_MAX_M, "cosy_dt_mask_loss: M=%d outside [1, %d]", M, COSY_DT_MAX_M);
    COSY_REQUIRE(C >= 1 && C <= COSY_DT_MAX_CLASSES, "cosy_dt_mask_loss: C=%d outside [1, %d] classes", C, COSY_DT_MAX_CLASSES);
    COSY_REQUIRE((long)B * rows_per_image * C * M * M < (1L << 31), "cosy_dt_mask_loss: %d x %d rows of %d x %d x %d logits are too many", B, rows_per_image, C, M, M);
    COSY_REQUIRE_PTR("cosy_dt_mask_loss", mask_ptr); COSY_REQUIRE_PTR("cosy_dt_mask_loss", mask_dims); COSY_REQUIRE_PTR("cosy_dt_mask_loss", boxes);
    COSY_REQUIRE_PTR("cosy_dt_mask_loss", matched);
    COSY_REQUIRE(mask_logits != nullptr || targets_out != nullptr, "cosy_dt_mask_loss: neither mask_logits nor targets_out: nothing to do");
    COSY_REQUIRE(mask_logits == nullptr || (labels && partial_ws && grad && loss), "cosy_dt_mask_loss: mask_logits need labels, partial_ws, grad and loss");
    const int R = B * rows_per_image;
    hipLaunchKernelGGL(dt_mask_kernel, dim3(R), dim3(DT_THREADS), 0, s, mask_ptr, mask_dims, B, boxes, labels, matched, pos_count, rows_per_image, R,
                       mask_logits, C, M, mask_logits ? grad : nullptr, targets_out, mask_logits ? partial_ws : nullptr);
    COSY_CHECK_HIP(hipGetLastError());
    if (mask_logits) {
        hipLaunchKernelGGL(dt_reduce_kernel, dim3(1), dim3(DT_THREADS), 0, s, partial_ws, (long)R, pos_count, B, rows_per_image, (long)R, (long)M * M, loss);
        COSY_CHECK_HIP(hipGetLastError());
    }
    return COSY_OK;
}

}  // extern "C"
