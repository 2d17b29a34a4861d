// Proposal side of the detector: what sits between the trunk's convolutions and the heads' inputs (torchvision 0.4.2 AnchorGenerator,
// RegionProposalNetwork.filter_proposals, MultiScaleRoIAlign with Mask R-CNN's defaults).  DESIGN.md section 22 states the contract;
// tests/detpre_ref.py is the CPU twin.  The NMS between decode and gather is kernels_detpost.hip's (cosy_nms_mask / cosy_nms_scan), unchanged.
//
//   rpn_select_kernel        ONE workgroup per (image, level): radix select of the k-th largest objectness logit over the order-preserving
//                            32-bit map of the float (four passes of 8 bits, per-wave LDS histograms, integer atomics), then an ordered
//                            compaction: the workgroup walks the level in chunks of 1024 anchors in index order and writes every anchor
//                            strictly above the threshold key, then the lowest-index ties at it.  An anchor whose logit or any delta is NaN
//                            is absent: never counted, never selected.  -0 counts as +0.
//   rpn_decode_kernel        ONE thread per arena slot (image, level, rank): the anchor from its index (anchor_box), BoxCoder.decode with weights 1,
//                            the log(1000/16) clamp and the clip to the image's own size (box_decode, both in det_device.h), the small-box test; a survivor leaves box, score, level,
//                            candidate index and the sort key  image << 52 | (0xffffffff - ordered score) << 20 | candidate index;  every
//                            other slot leaves the "empty slot of image b" key, which sorts behind all of b's candidates.
//   rpn_gather_kernel        the kept rows of cosy_nms_scan into (B, max_keep) padded proposals, scores, levels, candidate indices, counts
//   msroi_align_kernel       a workgroup owns one RoI and a group of channels: level mapper, then the P g tap indices and weights of each axis
//                            once into LDS (the taps are separable); lanes run over (channel, ph, pw), pw fastest, and write (R, C, P, P).
//   msroi_rows_kernel, msroi_align_backward_kernel   the adjoint of msroi_align_kernel into the feature maps, as a gather (DESIGN.md section
//                            24; tests/detbwd_ref.py is its twin): one thread per row notes image, level and touched cells; then a workgroup
//                            owns 16 x 16 cells of one (image, level) and 32 channels, lists the rows that meet its tile in ascending index
//                            and adds their terms to registers in a fixed order.  Every cell is stored once; no memset, no float atomic.
// Integer atomics only.  float32 with one rounding per operation: contraction is off (the pragma below and build.FILE_FLAGS).
#include <math.h>
#include "cosy_common.h"
#include "det_device.h"

#pragma clang fp contract(off)

namespace cosy {
namespace {

constexpr int SEL_THREADS = 1024;
constexpr int SEL_WAVES = SEL_THREADS / 64;
constexpr int PRE_THREADS = 256;
constexpr int RPN_KEY_INDEX_BITS = 20;                           // candidate index = level offset + anchor index < 2^20; 32 bits of score above
constexpr int MS_MAX_TAPS = 128;                                 // P g per axis

typedef cosy_msroi_levels_t MsLevels;

// larger float <=> larger key: all bits of a negative value flipped, the sign bit of any other; -0 is +0 first
__device__ __forceinline__ unsigned ordered_key(float v) {
    const unsigned u = v == 0.f ? 0u : __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// anchor i of a level = (cell, a) with a fastest; the head's NCHW planes are read in place
__device__ __forceinline__ float rpn_logit(const float* __restrict__ obj, int A, int HW, int i) {
    const int pos = i / A, a = i - pos * A;
    return obj[(size_t)a * HW + pos];
}
__device__ __forceinline__ bool rpn_deltas_finite(const float* __restrict__ del, int A, int HW, int i, float* d) {
    const int pos = i / A, a = i - pos * A;
    bool ok = true;
    for (int c = 0; c < 4; ++c) {
        d[c] = del[(size_t)(4 * a + c) * HW + pos];
        ok = ok && d[c] == d[c];
    }
    return ok;
}

__global__ __launch_bounds__(SEL_THREADS) void rpn_select_kernel(RpnLevels lv, int L, int A, int pre, int* __restrict__ sel_idx,
                                                                 int* __restrict__ sel_count) {
    __shared__ unsigned hist[SEL_WAVES][256];
    __shared__ unsigned wave_above[SEL_WAVES], wave_tie[SEL_WAVES];
    __shared__ unsigned s_prefix, s_need;
    __shared__ int s_k;
    const int l = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int HW = lv.H[l] * lv.W[l], n = A * HW;
    const float* obj = lv.objectness[l] + (size_t)b * A * HW;
    const float* del = lv.deltas[l] + (size_t)b * 4 * A * HW;
    float d[4];
    unsigned prefix = 0u, need = 0u;
    int k = 0;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        for (int i = tid; i < SEL_WAVES * 256; i += SEL_THREADS) (&hist[0][0])[i] = 0u;
        __syncthreads();
        for (int i = tid; i < n; i += SEL_THREADS) {
            const float v = rpn_logit(obj, A, HW, i);
            if (v != v) continue;
            const unsigned key = ordered_key(v);
            if (pass > 0 && (key >> (shift + 8)) != prefix) continue;
            if (!rpn_deltas_finite(del, A, HW, i, d)) continue;
            atomicAdd(&hist[wave][(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid < 256) {
            unsigned t = 0u;
            for (int w = 0; w < SEL_WAVES; ++w) t += hist[w][tid];
            hist[0][tid] = t;
        }
        __syncthreads();
        if (tid == 0) {
            if (pass == 0) {                                       // every present anchor is in the first histogram
                unsigned total = 0u;
                for (int q = 0; q < 256; ++q) total += hist[0][q];
                s_k = (int)(total < (unsigned)pre ? total : (unsigned)pre);
                s_need = (unsigned)s_k;
            }
            unsigned cum = 0u, want = s_need;
            int digit = 0;
            for (int q = 255; q >= 0; --q) {
                const unsigned c = hist[0][q];
                if (cum + c >= want) { digit = q; break; }
                cum += c;
            }
            s_need = want - cum;                                   // how many of the keys with this prefix are still wanted
            s_prefix = (prefix << 8) | (unsigned)digit;
        }
        __syncthreads();
        prefix = s_prefix; need = s_need; k = s_k;
        if (k == 0) break;                                         // (uniform)
    }
    if (tid == 0) sel_count[b * L + l] = k;
    if (k == 0) return;
    // `prefix` is the k-th largest key: all keys above it are taken, and the `need` lowest-index anchors at it
    const unsigned n_above = (unsigned)k - need;
    int* out = sel_idx + ((size_t)b * L + l) * pre;
    unsigned base_above = 0u, base_tie = 0u;
    for (int start = 0; start < n; start += SEL_THREADS) {
        const int i = start + tid;
        bool above = false, tie = false;
        if (i < n) {
            const float v = rpn_logit(obj, A, HW, i);
            if (v == v) {
                const unsigned key = ordered_key(v);
                if (key >= prefix && rpn_deltas_finite(del, A, HW, i, d)) { above = key > prefix; tie = key == prefix; }
            }
        }
        const unsigned long long ba = __ballot(above), bt = __ballot(tie);
        if (lane == 0) { wave_above[wave] = (unsigned)__popcll(ba); wave_tie[wave] = (unsigned)__popcll(bt); }
        __syncthreads();
        unsigned oa = 0u, ot = 0u, ta = 0u, tt = 0u;
        for (int w = 0; w < SEL_WAVES; ++w) {
            const unsigned ca = wave_above[w], ct = wave_tie[w];
            if (w < wave) { oa += ca; ot += ct; }
            ta += ca; tt += ct;
        }
        const unsigned long long below = (1ULL << lane) - 1ULL;
        if (above) {
            const unsigned p = base_above + oa + (unsigned)__popcll(ba & below);
            if (p < n_above) out[p] = i;
        }
        if (tie) {
            const unsigned p = base_tie + ot + (unsigned)__popcll(bt & below);
            if (p < need) out[n_above + p] = i;
        }
        base_above += ta; base_tie += tt;
        __syncthreads();
        if (base_above >= n_above && base_tie >= need) break;      // (uniform)
    }
}

__global__ __launch_bounds__(PRE_THREADS) void rpn_decode_kernel(RpnLevels lv, int L, int A, int B, int pre, const int* __restrict__ sel_idx,
                                                                 const int* __restrict__ sel_count, const float* __restrict__ net_sizes,
                                                                 float min_size, int cap, float* __restrict__ cand_boxes,
                                                                 float* __restrict__ cand_scores, int* __restrict__ cand_level,
                                                                 int* __restrict__ cand_src, long long* __restrict__ cand_keys,
                                                                 int* __restrict__ counts, unsigned* __restrict__ max_coord) {
    const long at = (long)blockIdx.x * PRE_THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63;
    if (at >= (long)B * cap) return;                               // (B cap is a multiple of 64: a wave is inside or outside as a whole)
    const int b = (int)(at / cap), s = (int)(at - (long)b * cap);  // one image per wave, for the same reason
    const int l = s / pre, j = s - l * pre;
    bool emit = false;
    Box o = {0.f, 0.f, 0.f, 0.f};
    float score = 0.f;
    int cand = 0;
    if (l < L) {
        int cnt = sel_count[b * L + l];
        cnt = cnt < pre ? cnt : pre;
        const int HW = lv.H[l] * lv.W[l];
        const int idx = j < cnt ? sel_idx[((size_t)b * L + l) * pre + j] : -1;
        if (idx >= 0 && idx < A * HW) {                            // an index read from memory: checked before it addresses anything
            float d[4];
            const float v = rpn_logit(lv.objectness[l] + (size_t)b * A * HW, A, HW, idx);
            const bool fin = rpn_deltas_finite(lv.deltas[l] + (size_t)b * 4 * A * HW, A, HW, idx, d);
            o = box_decode(anchor_box(lv, l, idx, A), d, net_sizes[2 * b], net_sizes[2 * b + 1]);   // (weights 1: the deltas as they are)
            score = v == 0.f ? 0.f : v;
            int first = 0;
            for (int m = 0; m < l; ++m) first += A * lv.H[m] * lv.W[m];
            cand = first + idx;
            emit = fin && v == v && __fsub_rn(o.x2, o.x1) >= min_size && __fsub_rn(o.y2, o.y1) >= min_size;   // (NaN fails every test)
        }
    }
    long long key = empty_key(b);
    if (emit) {
        store_box(cand_boxes, at, o);
        cand_scores[at] = score; cand_level[at] = l; cand_src[at] = cand;
        key = ((long long)b << ARENA_KEY_IMAGE_SHIFT) | ((long long)(0xffffffffu - ordered_key(score)) << RPN_KEY_INDEX_BITS) | (long long)cand;
        const unsigned big = __float_as_uint(o.x2 > o.y2 ? o.x2 : o.y2);       // clipped coordinates are >= +0: bits order as values
        if (big > __hip_atomic_load(&max_coord[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&max_coord[b], big);
    }
    cand_keys[at] = key;
    const unsigned long long grp = __ballot(emit);                 // one integer atomic per wave
    if (grp && lane == __ffsll((long long)grp) - 1) atomicAdd(&counts[b], __popcll(grp));
}

__global__ __launch_bounds__(PRE_THREADS) void rpn_gather_kernel(const int* __restrict__ kept, const int* __restrict__ n_kept,
                                                                 const float* __restrict__ cand_boxes, const float* __restrict__ cand_scores,
                                                                 const int* __restrict__ cand_level, const int* __restrict__ cand_src, int B,
                                                                 int cap, int max_keep, float* __restrict__ proposals,
                                                                 float* __restrict__ scores, int* __restrict__ levels, int* __restrict__ src,
                                                                 int* __restrict__ counts) {
    const long at = (long)blockIdx.x * PRE_THREADS + threadIdx.x;
    if (at < B) { const int n = n_kept[at]; counts[at] = n < 0 ? 0 : n < max_keep ? n : max_keep; }
    if (at >= (long)B * max_keep) return;
    const int b = (int)(at / max_keep), j = (int)(at - (long)b * max_keep);
    const long idx = kept[at];
    const bool ok = j < n_kept[b] && idx >= (long)b * cap && idx < (long)(b + 1) * cap;
    Box v = {0.f, 0.f, 0.f, 0.f};
    float sc = 0.f;
    int lvl = -1, s = -1;
    if (ok) {
        v = load_box(cand_boxes, idx);
        sc = cand_scores[idx]; lvl = cand_level[idx]; s = cand_src[idx];
    }
    store_box(proposals, at, v);
    scores[at] = sc; levels[at] = lvl; src[at] = s;
}

// (Tap / msroi_tap, one tap line of roi_align along one axis, live in det_device.h, as do anchor_box, box_decode and the arena's key layout above)
// The two pieces of a row that msroi_align_kernel and its adjoint must agree on to the bit: one definition each.
// LevelMapper: floor(4 + log2(sqrt(area) / 224 + 1e-6)) clamped to [k_min, k_max], minus k_min; a NaN (negative area) takes k_min
__device__ __forceinline__ int msroi_level(const Box& b, int k_min, int k_max) {
    const float sz = sqrtf(__fmul_rn(__fsub_rn(b.x2, b.x1), __fsub_rn(b.y2, b.y1)));
    const float t = floorf(__fadd_rn(4.f, log2f(__fadd_rn(__fdiv_rn(sz, 224.f), 1e-6f))));
    const int lvl = !(t >= (float)k_min) ? k_min : t > (float)k_max ? k_max : (int)t;
    return lvl - k_min;
}
// tap m = p g + i of one axis of a box [c1, c2] at a level of `size` cells
__device__ __forceinline__ Tap msroi_axis_tap(float c1, float c2, float scale, int P, int g, int m, int size) {
    const int p = m / g, i = m - p * g;
    const float lo = __fmul_rn(c1, scale), hi = __fmul_rn(c2, scale);
    const float ext = __fsub_rn(hi, lo);
    const float extent = ext > 1.f ? ext : 1.f;                    // max(extent, 1); a NaN extent gives 1
    return msroi_tap(lo, __fdiv_rn(extent, (float)P), p, i, g, size);
}

__global__ __launch_bounds__(PRE_THREADS) void msroi_align_kernel(MsLevels lv, int L, int B, int C, const float* __restrict__ boxes,
                                                                  const int* __restrict__ im_id, const int* __restrict__ counts,
                                                                  int rows_per_image, int P, int g, int cg, int k_min, int k_max,
                                                                  float* __restrict__ out, int* __restrict__ levels_out) {
    __shared__ int s_lo[2][MS_MAX_TAPS], s_hi[2][MS_MAX_TAPS];
    __shared__ float s_wl[2][MS_MAX_TAPS], s_wh[2][MS_MAX_TAPS];
    const int r = blockIdx.x, tid = threadIdx.x;
    const int c0 = blockIdx.y * cg, c1 = c0 + cg < C ? c0 + cg : C;
    const int PP = P * P, n_out = (c1 - c0) * PP;
    float* dst = out + ((size_t)r * C + c0) * PP;
    // everything below up to the tap tables is uniform over the workgroup
    int img = im_id ? im_id[r] : r / rows_per_image;
    bool row = img >= 0 && img < B;
    if (row && counts) row = r - img * rows_per_image < counts[img];
    const Box bx = load_box(boxes, r);
    const int lvl = msroi_level(bx, k_min, k_max);
    if (lvl < 0 || lvl >= L) row = false;                          // (the entry point refuses k_max - k_min >= L: never taken)
    if (blockIdx.y == 0 && tid == 0 && levels_out) levels_out[r] = row ? lvl : -1;
    if (!row) {                                                    // a row no image owns: zeros
        for (int o = tid; o < n_out; o += PRE_THREADS) dst[o] = 0.f;
        return;
    }
    const int H = lv.H[lvl], W = lv.W[lvl];
    const float scale = lv.scale[lvl];
    const int taps = P * g;
    for (int q = tid; q < 2 * taps; q += PRE_THREADS) {
        const int axis = q / taps, m = q - axis * taps;
        const Tap tp = msroi_axis_tap(axis ? bx.x1 : bx.y1, axis ? bx.x2 : bx.y2, scale, P, g, m, axis ? W : H);
        s_lo[axis][m] = tp.lo; s_hi[axis][m] = tp.hi; s_wl[axis][m] = tp.wl; s_wh[axis][m] = tp.wh;
    }
    __syncthreads();
    const size_t plane = (size_t)H * W;
    const float* feat = lv.feat[lvl] + ((size_t)img * C + c0) * plane;
    const float count = (float)(g * g);
    for (int o = tid; o < n_out; o += PRE_THREADS) {
        const int c = o / PP, rem = o - c * PP, ph = rem / P, pw = rem - ph * P;
        const float* p = feat + (size_t)c * plane;
        float acc = 0.f;
        for (int iy = 0; iy < g; ++iy) {
            const int ty = ph * g + iy, yl = s_lo[0][ty], yh = s_hi[0][ty];
            if (yl < 0) continue;
            const float ly = s_wl[0][ty], hy = s_wh[0][ty];
            for (int ix = 0; ix < g; ++ix) {
                const int tx = pw * g + ix, xl = s_lo[1][tx], xh = s_hi[1][tx];
                if (xl < 0) continue;
                const float lx = s_wl[1][tx], hx = s_wh[1][tx];
                const float w1 = __fmul_rn(hy, hx), w2 = __fmul_rn(hy, lx), w3 = __fmul_rn(ly, hx), w4 = __fmul_rn(ly, lx);
                float v = __fmul_rn(w1, p[yl * W + xl]);
                v = __fadd_rn(v, __fmul_rn(w2, p[yl * W + xh]));
                v = __fadd_rn(v, __fmul_rn(w3, p[yh * W + xl]));
                v = __fadd_rn(v, __fmul_rn(w4, p[yh * W + xh]));
                acc = __fadd_rn(acc, v);
            }
        }
        dst[o] = __fdiv_rn(acc, count);
    }
}

// ---- the adjoint of msroi_align_kernel: a gather, DESIGN.md section 24 ----------------------------------------------------------------
constexpr int BWD_TILE = 16;                                     // a workgroup owns 16 x 16 cells of one (image, level): one cell per thread
constexpr int BWD_CG = 32;                                       // ... and up to 32 channels, one accumulator register each
constexpr int BWD_SLOTS = 4;                                     // listed rows staged at a time, one per wave
constexpr int BWD_WS = 8;                                        // ints per row of the workspace: image (-1: adds nothing), level, y lo, y hi, x lo, x hi
constexpr int BWD_ENTRIES = 2 * MS_MAX_TAPS;                     // a tap puts its low and its high weight on one cell each

struct BwdPlan {
    float* grad[COSY_RPN_MAX_LEVELS];
    int first[COSY_RPN_MAX_LEVELS + 1];                            // blocks [first[l], first[l+1]) are level l's B x tiles; none for a level not asked for
    int tiles_x[COSY_RPN_MAX_LEVELS], tiles[COSY_RPN_MAX_LEVELS];
};

// one thread per row: what the forward decides once per row (image, padding, level) and the cells its valid taps touch
__global__ __launch_bounds__(PRE_THREADS) void msroi_rows_kernel(MsLevels lv, int L, int B, const float* __restrict__ boxes,
                                                                 const int* __restrict__ im_id, const int* __restrict__ counts,
                                                                 int rows_per_image, int R, int P, int g, int k_min, int k_max,
                                                                 int* __restrict__ ws) {
    const long r = (long)blockIdx.x * PRE_THREADS + threadIdx.x;
    if (r >= R) return;
    const int img = im_id ? im_id[r] : (int)(r / rows_per_image);
    bool row = img >= 0 && img < B;
    if (row && counts) row = r - (long)img * rows_per_image < counts[img];
    const Box bx = load_box(boxes, r);
    const int lvl = msroi_level(bx, k_min, k_max);
    if (lvl < 0 || lvl >= L) row = false;
    int lo[2] = {0x7fffffff, 0x7fffffff}, hi[2] = {-1, -1};
    if (row) {
        const float scale = lv.scale[lvl];
        for (int axis = 0; axis < 2; ++axis)
            for (int m = 0; m < P * g; ++m) {
                const Tap t = msroi_axis_tap(axis ? bx.x1 : bx.y1, axis ? bx.x2 : bx.y2, scale, P, g, m, axis ? lv.W[lvl] : lv.H[lvl]);
                if (t.lo < 0) continue;
                lo[axis] = t.lo < lo[axis] ? t.lo : lo[axis];
                hi[axis] = t.hi > hi[axis] ? t.hi : hi[axis];
            }
        row = hi[0] >= 0 && hi[1] >= 0;                            // no valid sample on an axis: every value of the row was 0
    }
    int* w = ws + BWD_WS * (size_t)r;
    w[0] = row ? img : -1; w[1] = lvl; w[2] = lo[0]; w[3] = hi[0]; w[4] = lo[1]; w[5] = hi[1]; w[6] = 0; w[7] = 0;
}

// A workgroup owns a tile of one (image, level) and a group of channels.  It walks the image's rows in ascending index, 256 at a time, and
// lists (ballot-ordered, so still ascending) those of its level whose taps meet the tile.  Wave w then stages listed row i + w: per axis its
// taps' weights bucketed by the tile's 16 coordinates, inside a bucket by ascending tap, of one tap the low weight first.  Every thread adds
// rows in list order, y entries outer, x entries inner: acc = fl(acc + fl(fl(wy wx) g)), and stores fl(acc / g^2) once.
__global__ __launch_bounds__(PRE_THREADS) void msroi_align_backward_kernel(MsLevels lv, BwdPlan plan, int L, int B, int C,
                                                                           const float* __restrict__ grad_out,
                                                                           const float* __restrict__ boxes, const int* __restrict__ ws,
                                                                           int rows_per_image, int R, int P, int g) {
    __shared__ int s_list[PRE_THREADS];
    __shared__ int s_wave[PRE_THREADS / 64];
    __shared__ int s_start[BWD_SLOTS][2][BWD_TILE + 1];
    __shared__ unsigned char s_bin[BWD_SLOTS][2][BWD_ENTRIES];     // p of the entry's tap
    __shared__ float s_w[BWD_SLOTS][2][BWD_ENTRIES];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    int l = 0;
    while (l + 1 < L && (int)blockIdx.x >= plan.first[l + 1]) ++l;  // (uniform)
    const int within = (int)blockIdx.x - plan.first[l];
    const int b = within / plan.tiles[l], t = within - b * plan.tiles[l];
    const int tile_y = t / plan.tiles_x[l], tile_x = t - tile_y * plan.tiles_x[l];
    const int H = lv.H[l], W = lv.W[l];
    const float scale = lv.scale[l];
    const int y0 = tile_y * BWD_TILE, x0 = tile_x * BWD_TILE, ly = tid >> 4, lx = tid & 15;
    const int c0 = blockIdx.y * BWD_CG, nc = C - c0 < BWD_CG ? C - c0 : BWD_CG;
    const int PP = P * P, taps = P * g;
    const long r_first = rows_per_image ? (long)b * rows_per_image : 0, r_last = rows_per_image ? r_first + rows_per_image : R;
    const int r_begin = (int)(r_first < R ? r_first : R), r_end = (int)(r_last < R ? r_last : R);
    const unsigned long long below = (1ULL << lane) - 1ULL;
    float acc[BWD_CG];
#pragma unroll
    for (int c = 0; c < BWD_CG; ++c) acc[c] = 0.f;
    for (int chunk = r_begin; chunk < r_end; chunk += PRE_THREADS) {
        const int r = chunk + tid;
        bool take = false;
        if (r < r_end) {
            const int* w = ws + BWD_WS * (size_t)r;
            take = w[0] == b && w[1] == l && w[2] < y0 + BWD_TILE && w[3] >= y0 && w[4] < x0 + BWD_TILE && w[5] >= x0;
        }
        const unsigned long long mine = __ballot(take);
        if (lane == 0) s_wave[wave] = __popcll(mine);
        __syncthreads();
        int before = 0, n = 0;
        for (int w = 0; w < PRE_THREADS / 64; ++w) { const int c = s_wave[w]; before += w < wave ? c : 0; n += c; }
        if (take) s_list[before + __popcll(mine & below)] = r;
        __syncthreads();
        for (int i0 = 0; i0 < n; i0 += BWD_SLOTS) {
            if (i0 + wave < n) {                                   // (uniform over the wave) stage one row per wave
                const int rr = s_list[i0 + wave];
                for (int axis = 0; axis < 2; ++axis) {
                    const float a1 = boxes[4 * (size_t)rr + 1 - axis], a2 = boxes[4 * (size_t)rr + 3 - axis];
                    const int size = axis ? W : H, first = axis ? x0 : y0;
                    Tap tp[2];                                     // taps lane and lane + 64 (MS_MAX_TAPS = 128)
#pragma unroll
                    for (int pass = 0; pass < 2; ++pass) {
                        tp[pass] = Tap{-1, -1, 0.f, 0.f};
                        if (lane + 64 * pass < taps) tp[pass] = msroi_axis_tap(a1, a2, scale, P, g, lane + 64 * pass, size);
                    }
                    int cnt = 0;                                   // (uniform) at most 2 taps entries over the 16 buckets
                    for (int k = 0; k < BWD_TILE; ++k) {
                        if (lane == 0) s_start[wave][axis][k] = cnt;
#pragma unroll
                        for (int pass = 0; pass < 2; ++pass) {
                            if (pass * 64 >= taps) continue;       // (uniform)
                            const Tap q = tp[pass];
                            const bool on_lo = q.lo == first + k, on_hi = q.hi == first + k;   // (an invalid tap has lo = hi = -1)
                            const unsigned long long blo = __ballot(on_lo), bhi = __ballot(on_hi);
                            const int pos = cnt + __popcll(blo & below) + __popcll(bhi & below);
                            const unsigned char bin = (unsigned char)((lane + 64 * pass) / g);
                            if (on_lo) { s_bin[wave][axis][pos] = bin; s_w[wave][axis][pos] = q.wh; }                 // wh: the low tap's weight
                            if (on_hi) { s_bin[wave][axis][pos + (on_lo ? 1 : 0)] = bin; s_w[wave][axis][pos + (on_lo ? 1 : 0)] = q.wl; }
                            cnt += __popcll(blo) + __popcll(bhi);
                        }
                    }
                    if (lane == 0) s_start[wave][axis][BWD_TILE] = cnt;
                }
            }
            __syncthreads();
            for (int s = 0; s < BWD_SLOTS && i0 + s < n; ++s) {
                const int ys = s_start[s][0][ly], ye = s_start[s][0][ly + 1], xs = s_start[s][1][lx], xe = s_start[s][1][lx + 1];
                if (ys == ye || xs == xe) continue;
                const float* gr = grad_out + ((size_t)s_list[i0 + s] * C + c0) * PP;
                for (int ey = ys; ey < ye; ++ey) {
                    const float wy = s_w[s][0][ey];
                    const float* gy = gr + (int)s_bin[s][0][ey] * P;
                    for (int ex = xs; ex < xe; ++ex) {
                        const float w = __fmul_rn(wy, s_w[s][1][ex]);
                        const float* gp = gy + (int)s_bin[s][1][ex];
#pragma unroll
                        for (int c = 0; c < BWD_CG; ++c)
                            if (c < nc) acc[c] = __fadd_rn(acc[c], __fmul_rn(w, gp[(size_t)c * PP]));
                    }
                }
            }
            __syncthreads();
        }
        __syncthreads();                                           // s_wave and s_list are rewritten by the next chunk
    }
    const int y = y0 + ly, x = x0 + lx;
    if (y >= H || x >= W) return;
    const float count = (float)(g * g);
    float* dst = plan.grad[l] + (((size_t)b * C + c0) * H + y) * W + x;
#pragma unroll
    for (int c = 0; c < BWD_CG; ++c)
        if (c < nc) dst[(size_t)c * H * W] = __fdiv_rn(acc[c], count);
}

int rpn_level_args(const char* fn,const cosy_rpn_levels_t* lv, int L, int A, int B, int pre) {
    long total;
    if (int rc = rpn_levels_args(fn, lv, L, A, &total)) return rc;
    COSY_REQUIRE(B >= 0 && B <= ARENA_MAX_IMAGES, "%s: B=%d outside [0, %d] images per call", fn, B, ARENA_MAX_IMAGES);
    COSY_REQUIRE(pre >= 1, "%s: pre_nms_top_n=%d", fn, pre);
    COSY_REQUIRE((long)pre * L <= (long)cosy_nms_max_candidates(), "%s: pre_nms_top_n L = %ld exceeds cosy_nms_max_candidates() = %d", fn, (long)pre * L,
                 cosy_nms_max_candidates());
    for (int l = 0; l < L; ++l)
        COSY_REQUIRE(B == 0 || (lv->objectness[l] != nullptr && lv->deltas[l] != nullptr), "%s: null objectness / deltas of level %d", fn, l);
    return COSY_OK;
}

// what cosy_msroi_align and its backward refuse alike
int msroi_args(const char* fn, const cosy_msroi_levels_t* levels, int L, int B, int C, const int* im_id, const int* counts, int rows_per_image,
               int R, int P, int sampling_ratio, int k_min, int k_max) {
    COSY_REQUIRE(levels != nullptr, "%s: null levels", fn);
    COSY_REQUIRE(L >= 1 && L <= COSY_RPN_MAX_LEVELS, "%s: L=%d outside [1, %d] levels", fn, L, COSY_RPN_MAX_LEVELS);
    COSY_REQUIRE(B >= 0 && R >= 0 && C >= 1, "%s: B=%d R=%d C=%d", fn, B, R, C);
    COSY_REQUIRE(sampling_ratio > 0, "%s: sampling_ratio=%d must be > 0", fn, sampling_ratio);
    COSY_REQUIRE(P >= 1 && (long)P * sampling_ratio <= MS_MAX_TAPS, "%s: P=%d with sampling_ratio=%d exceeds %d taps per axis", fn, P, sampling_ratio,
                 MS_MAX_TAPS);
    COSY_REQUIRE(k_min <= k_max && k_max - k_min < L, "%s: k_min=%d k_max=%d do not index %d levels", fn, k_min, k_max, L);
    COSY_REQUIRE(R == 0 || (im_id != nullptr) != (rows_per_image >= 1), "%s: exactly one of im_id and rows_per_image=%d >= 1 names the images", fn,
                 rows_per_image);
    COSY_REQUIRE(counts == nullptr || im_id == nullptr, "%s: counts go with rows_per_image, not with im_id", fn);
    COSY_REQUIRE(B >= 1 || R == 0, "%s: R=%d rows without an image", fn, R);
    for (int l = 0; l < L; ++l) {
        COSY_REQUIRE(levels->H[l] >= 1 && levels->W[l] >= 1 && (long)levels->H[l] * levels->W[l] < (1L << 30), "%s: level %d is %d x %d cells", fn, l,
                     levels->H[l], levels->W[l]);
        COSY_REQUIRE(levels->scale[l] > 0.f, "%s: scale of level %d is %g", fn, l, (double)levels->scale[l]);
    }
    return COSY_OK;
}

}  // namespace
}  // namespace cosy

using namespace cosy;

extern "C" {

int cosy_rpn_select(const cosy_rpn_levels_t* levels, int L, int A, int B, int pre_nms_top_n, int* sel_idx, int* sel_count, cosy_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    if (int rc = rpn_level_args("cosy_rpn_select", levels, L, A, B, pre_nms_top_n)) return rc;
    if (B == 0) return COSY_OK;
    COSY_REQUIRE_PTR("cosy_rpn_select", sel_idx); COSY_REQUIRE_PTR("cosy_rpn_select", sel_count);
    hipLaunchKernelGGL(rpn_select_kernel, dim3(L, B), dim3(SEL_THREADS), 0, s, *levels, L, A, pre_nms_top_n, sel_idx, sel_count);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

int cosy_rpn_decode(const cosy_rpn_levels_t* levels, int L, int A, int B, int pre_nms_top_n, const int* sel_idx, const int* sel_count,
                    const float* net_sizes, float min_size, int cap, float* cand_boxes, float* cand_scores, int* cand_level, int* cand_src,
                    long long* cand_keys, int* counts, float* max_coord, cosy_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    if (int rc = rpn_level_args("cosy_rpn_decode", levels, L, A, B, pre_nms_top_n)) return rc;
    if (int rc = arena_cap_args("cosy_rpn_decode", cap)) return rc;
    COSY_REQUIRE((long)pre_nms_top_n * L <= cap, "cosy_rpn_decode: cap=%d holds fewer than pre_nms_top_n L = %ld slots", cap, (long)pre_nms_top_n * L);
    COSY_REQUIRE(min_size >= 0.f, "cosy_rpn_decode: min_size=%g is negative or NaN", (double)min_size);
    if (B == 0) return COSY_OK;
    COSY_REQUIRE_PTR("cosy_rpn_decode", sel_idx); COSY_REQUIRE_PTR("cosy_rpn_decode", sel_count); COSY_REQUIRE_PTR("cosy_rpn_decode", net_sizes);
    COSY_REQUIRE_PTR("cosy_rpn_decode", cand_boxes); COSY_REQUIRE_PTR("cosy_rpn_decode", cand_scores); COSY_REQUIRE_PTR("cosy_rpn_decode", cand_level);
    COSY_REQUIRE_PTR("cosy_rpn_decode", cand_src); COSY_REQUIRE_PTR("cosy_rpn_decode", cand_keys); COSY_REQUIRE_PTR("cosy_rpn_decode", counts);
    COSY_REQUIRE_PTR("cosy_rpn_decode", max_coord);
    COSY_CHECK_HIP(hipMemsetAsync(counts, 0, sizeof(int) * (size_t)B, s));
    COSY_CHECK_HIP(hipMemsetAsync(max_coord, 0, sizeof(float) * (size_t)B, s));
    hipLaunchKernelGGL(rpn_decode_kernel, dim3(cdiv((long)B * cap, PRE_THREADS)), dim3(PRE_THREADS), 0, s, *levels, L, A, B, pre_nms_top_n, sel_idx,
                       sel_count, net_sizes, min_size, cap, cand_boxes, cand_scores, cand_level, cand_src, cand_keys, counts, (unsigned*)max_coord);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

int cosy_rpn_gather(const int* kept, const int* n_kept, const float* cand_boxes, const float* cand_scores, const int* cand_level,
                    const int* cand_src, int B, int cap, int max_keep, float* proposals, float* scores, int* levels, int* src, int* counts,
                    cosy_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    COSY_REQUIRE(B >= 0 && B <= ARENA_MAX_IMAGES && max_keep >= 0, "cosy_rpn_gather: B=%d max_keep=%d", B, max_keep);
    if (int rc = arena_cap_args("cosy_rpn_gather", cap, false)) return rc;
    COSY_REQUIRE((long)B * max_keep < (1L << 30), "cosy_rpn_gather: %d x %d rows are too many", B, max_keep);
    if (B == 0) return COSY_OK;
    COSY_REQUIRE_PTR("cosy_rpn_gather", n_kept); COSY_REQUIRE_PTR("cosy_rpn_gather", counts);
    if (max_keep > 0) {
        COSY_REQUIRE_PTR("cosy_rpn_gather", kept); COSY_REQUIRE_PTR("cosy_rpn_gather", cand_boxes); COSY_REQUIRE_PTR("cosy_rpn_gather", cand_scores);
        COSY_REQUIRE_PTR("cosy_rpn_gather", cand_level); COSY_REQUIRE_PTR("cosy_rpn_gather", cand_src); COSY_REQUIRE_PTR("cosy_rpn_gather", proposals);
        COSY_REQUIRE_PTR("cosy_rpn_gather", scores); COSY_REQUIRE_PTR("cosy_rpn_gather", levels); COSY_REQUIRE_PTR("cosy_rpn_gather", src);
    }
    const long threads = (long)B * max_keep > B ? (long)B * max_keep : B;
    hipLaunchKernelGGL(rpn_gather_kernel, dim3(cdiv(threads, PRE_THREADS)), dim3(PRE_THREADS), 0, s, kept, n_kept, cand_boxes, cand_scores, cand_level,
                       cand_src, B, cap, max_keep, proposals, scores, levels, src, counts);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

int cosy_msroi_align(const cosy_msroi_levels_t* levels, int L, int B, int C, const float* boxes, const int* im_id, const int* counts,
                     int rows_per_image, int R, int P, int sampling_ratio, int k_min, int k_max, float* out, int* levels_out,
                     cosy_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    if (int rc = msroi_args("cosy_msroi_align", levels, L, B, C, im_id, counts, rows_per_image, R, P, sampling_ratio, k_min, k_max)) return rc;
    for (int l = 0; l < L; ++l) COSY_REQUIRE(R == 0 || levels->feat[l] != nullptr, "cosy_msroi_align: null features of level %d", l);
    if (R == 0) return COSY_OK;
    COSY_REQUIRE_PTR("cosy_msroi_align", boxes); COSY_REQUIRE_PTR("cosy_msroi_align", out);
    int cg = 1;                                                    // channels per workgroup: the largest power of two with cg P^2 <= 4096
    while (cg * 2 * P * P <= 4096 && cg * 2 <= C) cg *= 2;
    COSY_REQUIRE(cdiv(C, cg) <= COSY_MAX_GRID_Y, "cosy_msroi_align: C=%d needs more than %d channel groups", C, COSY_MAX_GRID_Y);
    hipLaunchKernelGGL(msroi_align_kernel, dim3(R, cdiv(C, cg)), dim3(PRE_THREADS), 0, s, *levels, L, B, C, boxes, im_id, counts, rows_per_image, P,
                       sampling_ratio, cg, k_min, k_max, out, levels_out);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

int cosy_msroi_align_backward(const cosy_msroi_levels_t* levels, float* const* grad_feat, int L, int B, int C, const float* grad_out,
                              const float* boxes, const int* im_id, const int* counts, int rows_per_image, int R, int P, int sampling_ratio,
                              int k_min, int k_max, int* row_ws, cosy_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    if (int rc = msroi_args("cosy_msroi_align_backward", levels, L, B, C, im_id, counts, rows_per_image, R, P, sampling_ratio, k_min, k_max)) return rc;
    COSY_REQUIRE_PTR("cosy_msroi_align_backward", grad_feat);
    COSY_REQUIRE(R <= (1 << 30), "cosy_msroi_align_backward: R=%d rows exceed 2^30", R);
    COSY_REQUIRE(cdiv(C, BWD_CG) <= COSY_MAX_GRID_Y, "cosy_msroi_align_backward: C=%d needs more than %d channel groups", C, COSY_MAX_GRID_Y);
    BwdPlan plan;
    long blocks = 0;
    for (int l = 0; l < COSY_RPN_MAX_LEVELS; ++l) {
        plan.grad[l] = l < L ? grad_feat[l] : nullptr;
        plan.first[l] = (int)blocks;
        plan.tiles_x[l] = plan.tiles[l] = 1;
        if (!plan.grad[l]) continue;                               // a level whose gradient nobody needs
        plan.tiles_x[l] = cdiv(levels->W[l], BWD_TILE);
        plan.tiles[l] = plan.tiles_x[l] * cdiv(levels->H[l], BWD_TILE);
        blocks += (long)B * plan.tiles[l];
        COSY_REQUIRE(blocks <= 0x7fffffffL, "cosy_msroi_align_backward: B=%d images of levels 0 .. %d need more than 2^31 - 1 tiles", B, l);
    }
    plan.first[COSY_RPN_MAX_LEVELS] = (int)blocks;
    if (blocks == 0) return COSY_OK;
    if (R > 0) {
        COSY_REQUIRE_PTR("cosy_msroi_align_backward", grad_out); COSY_REQUIRE_PTR("cosy_msroi_align_backward", boxes);
        COSY_REQUIRE_PTR("cosy_msroi_align_backward", row_ws);
        hipLaunchKernelGGL(msroi_rows_kernel, dim3(cdiv(R, PRE_THREADS)), dim3(PRE_THREADS), 0, s, *levels, L, B, boxes, im_id, counts, rows_per_image, R,
                           P, sampling_ratio, k_min, k_max, row_ws);
        COSY_CHECK_HIP(hipGetLastError());
    }
    // without a row every requested cell still gets its +0
    hipLaunchKernelGGL(msroi_align_backward_kernel, dim3((unsigned)blocks, cdiv(C, BWD_CG)), dim3(PRE_THREADS), 0, s, *levels, plan, L, B, C, grad_out,
                       boxes, row_ws, im_id ? 0 : rows_per_image, R, P, sampling_ratio);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

}  // extern "C"
