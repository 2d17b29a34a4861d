// Output side of the detector: everything between the Mask R-CNN heads' raw outputs and the `detections` collection
// (torchvision 0.4.2 roi_heads.postprocess_detections, ops.batched_nms, GeneralizedRCNNTransform.postprocess, maskrcnn_inference and
// paste_masks_in_image; cosypose/integrated/detector.py:28-50 on top).  DESIGN.md section 21 states the contract; tests/detpost_ref.py is
// the torch-CPU twin.
//
//   detpost_init_kernel      keys <- "empty slot of image b" (sorts behind every candidate of b), counts <- 0, max coordinate <- 0
//   det_decode_kernel        ONE thread per proposal: softmax over the C logits, then per foreground class decode and clip (det_device.h's
//                            box_decode, the RPN side's too), score threshold and small-box test; a survivor takes a slot of its image's
//                            arena through a wave-aggregated integer atomic and leaves box, score, label, source index and its 64-bit sort key
//                            (image << 52 | (0x7fffffff - score bits) << 21 | candidate index): sorting the keys ascending gives image,
//                            then descending score, then ascending candidate index, whatever order the atomics handed the slots out in.
//   nms_mask_kernel          one wave per 64 x 64 tile (column block >= row block) of an image's suppression matrix: lane l holds box
//                            row_block * 64 + l and builds the 64-bit word "columns whose IoU with me is > threshold"; the column
//                            block's boxes sit in LDS.  Boxes are read through the sort order and shifted by label * (max + 1).
//   nms_scan_kernel          one workgroup per image walks the row blocks in order: wave 0 resolves the diagonal tile with 64 lane
//                            reads (no memory), then every thread ORs the kept rows' words of one later column block into the
//                            `removed` bit vector in LDS.  Stops at max_keep.  No host round trip.
//   det_gather_kernel        the kept candidates into (B, max_keep) padded rows: box as the network saw it, box in the frame
//                            (x * ratio_w, y * ratio_h), and the small int32 block the host reads (counts, labels, score bits)
//   paste_masks_kernel<V>    a workgroup owns 16384 consecutive pixels of one detection's (H, W) plane: where they meet the box it stages
//                            the sigmoid of the label's channel, zero-padded to (M+2)^2, in LDS and writes value > mask_th; everything
//                            else holds the value 0 and is written as 0 > mask_th by the same launch (false unless mask_th is negative;
//                            a NaN mask_th makes every pixel false).  V = 16 pixels per 16-byte store where the plane allows it.
// Integer atomics only (add, max on the bits of non-negative floats): equal inputs give equal bytes.  float32 with one rounding per
// operation; the file is compiled with contraction off (the pragma below and -ffp-contract=off in build.FILE_FLAGS).
#include <limits.h>
#include <math.h>
#include "cosy_common.h"
#include "det_device.h"

#pragma clang fp contract(off)

namespace cosy {
namespace {

constexpr int DP_THREADS = 256;
constexpr int NMS_MAX_CAP = 16384;                               // candidates per image (segment): 32 MiB of matrix per image at the cap
constexpr int NMS_MAX_BLOCKS = NMS_MAX_CAP / 64;
constexpr int DP_KEY_INDEX_BITS = 21;                            // candidate index = proposal * (C-1) + (label-1) < 2^21; 31 bits of score above
constexpr int PASTE_MAX_M = 62;                                  // (M+2)^2 floats of LDS: 16 KiB at the cap
constexpr int PASTE_ITERS = 4;                                   // 16-byte stores per thread: 16384 pixels per workgroup

__global__ __launch_bounds__(DP_THREADS) void detpost_init_kernel(long long* __restrict__ keys, int* __restrict__ counts,
                                                                  unsigned* __restrict__ max_coord, int B, int cap) {
    const long at = (long)blockIdx.x * DP_THREADS + threadIdx.x;
    if (at < (long)B * cap) keys[at] = empty_key((int)(at / cap));
    if (at < B) { counts[at] = 0; max_coord[at] = 0u; }
}

__global__ __launch_bounds__(DP_THREADS) void det_decode_kernel(const float* __restrict__ logits, const float* __restrict__ reg,
                                                                const float* __restrict__ proposals, const int* __restrict__ prop_offsets,
                                                                const float* __restrict__ net_sizes, int R, int C, int B, float score_thresh,
                                                                int cap, float* __restrict__ cand_boxes, float* __restrict__ cand_scores,
                                                                int* __restrict__ cand_labels, int* __restrict__ cand_src,
                                                                long long* __restrict__ cand_keys, int* __restrict__ counts,
                                                                unsigned* __restrict__ max_coord) {
    const int r = blockIdx.x * DP_THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63;
    // the proposal's image: offsets are non-decreasing with offsets[0] = 0 and offsets[B] = R; anything else finds no image and is skipped
    int img = -1, first = 0;
    if (r < R) {
        for (int b = 0; b < B; ++b) {
            const int lo = prop_offsets[b], hi = prop_offsets[b + 1];
            if (r >= lo && r < hi) { img = b; first = lo; break; }
        }
    }
    const bool valid = img >= 0;
    float m = 0.f, sum = 1.f, net_h = 0.f, net_w = 0.f;
    Box p = {0.f, 0.f, 0.f, 0.f};
    const float* x = logits + (size_t)(valid ? r : 0) * C;
    if (valid) {
        m = x[0];
        for (int j = 1; j < C; ++j) m = x[j] > m ? x[j] : m;
        sum = 0.f;
        for (int j = 0; j < C; ++j) sum = __fadd_rn(sum, expf(__fsub_rn(x[j], m)));
        net_h = net_sizes[2 * img]; net_w = net_sizes[2 * img + 1];
        p = load_box(proposals, r);
    }
    for (int j = 1; j < C; ++j) {                                  // (uniform trip count: the ballots below need every lane)
        bool emit = false;
        float score = 0.f;
        Box o = {0.f, 0.f, 0.f, 0.f};
        if (valid) {
            score = __fdiv_rn(expf(__fsub_rn(x[j], m)), sum);
            const float* d = reg + ((size_t)r * C + j) * 4;
            const float dd[4] = {__fdiv_rn(d[0], 10.f), __fdiv_rn(d[1], 10.f), __fdiv_rn(d[2], 5.f), __fdiv_rn(d[3], 5.f)};   // weights (10, 10, 5, 5)
            o = box_decode(p, dd, net_h, net_w);                   // (the proposal's centre and extent do not depend on j: computed once)
            emit = score > score_thresh && __fsub_rn(o.x2, o.x1) >= 1e-2f && __fsub_rn(o.y2, o.y1) >= 1e-2f;   // (NaN fails every test)
        }
        // one atomic per wave and image: the lanes of the leader's image take consecutive slots.  The loop runs once per image that has
        // an emitting lane in this wave: once inside an image, twice across one boundary, up to 64 times where images hold a proposal each
        unsigned long long todo = __ballot(emit);
        while (todo) {
            const int leader = __ffsll((long long)todo) - 1;
            const int limg = __shfl(img, leader);
            const bool mine = emit && img == limg;
            const unsigned long long grp = __ballot(mine);
            int base = 0;
            if (lane == leader) base = atomicAdd(&counts[limg], __popcll(grp));
            base = __shfl(base, leader);
            if (mine) {
                const int slot = base + __popcll(grp & ((1ULL << lane) - 1ULL));
                if (slot >= 0 && slot < cap) {                     // past the cap nothing is written; counts[] says so to the host
                    const size_t at = (size_t)img * cap + slot;
                    const int src = (r - first) * (C - 1) + (j - 1);
                    store_box(cand_boxes, at, o);
                    cand_scores[at] = score; cand_labels[at] = j; cand_src[at] = src;
                    const long long sbits = 0x7fffffffLL - (long long)(__float_as_uint(score) & 0x7fffffffu);
                    cand_keys[at] = ((long long)img << ARENA_KEY_IMAGE_SHIFT) | (sbits << DP_KEY_INDEX_BITS) | (long long)src;
                    const unsigned big = __float_as_uint(o.x2 > o.y2 ? o.x2 : o.y2);   // clipped coordinates are >= +0: bits order as values
                    if (big > __hip_atomic_load(&max_coord[img], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&max_coord[img], big);
                }
            }
            todo &= ~grp;
        }
    }
}

__device__ __forceinline__ Box nan_box() { const float q = __uint_as_float(0x7fc00000u); return {q, q, q, q}; }

// sorted row i of a segment, shifted by its label; a row outside the segment or an index outside the boxes gives NaNs (IoU NaN: never > threshold)
__device__ __forceinline__ Box nms_box(const float* __restrict__ boxes, const long long* __restrict__ order, const int* __restrict__ labels,
                                       float shift_unit, int start, int i, int n, int N) {
    if (i >= n) return nan_box();
    const long long idx = order ? order[start + i] : (long long)(start + i);
    if (idx < 0 || idx >= N) return nan_box();
    Box v = load_box(boxes, idx);
    if (labels) {
        const float off = __fmul_rn((float)labels[idx], shift_unit);
        v.x1 = __fadd_rn(v.x1, off); v.y1 = __fadd_rn(v.y1, off); v.x2 = __fadd_rn(v.x2, off); v.y2 = __fadd_rn(v.y2, off);
    }
    return v;
}

// a segment's rows [start, start + n): clamped so that nothing outside [0, N) or beyond `cap` rows is ever addressed
__device__ __forceinline__ int seg_rows(const int* __restrict__ seg_start, const int* __restrict__ seg_count, int b, int N, int cap, int* start) {
    const int s = seg_start[b];
    int n = seg_count[b];
    n = n < cap ? n : cap;
    if (s < 0 || n < 0 || s > N || n > N - s) n = 0;
    *start = s;
    return n;
}

__global__ __launch_bounds__(64) void nms_mask_kernel(const float* __restrict__ boxes, const long long* __restrict__ order,
                                                      const int* __restrict__ labels, const float* __restrict__ max_coord,
                                                      const int* __restrict__ seg_start, const int* __restrict__ seg_count, int N, int cap,
                                                      float iou_thresh, unsigned long long* __restrict__ mask) {
    __shared__ Box cols[64];
    const int cb = blockIdx.x, rb = blockIdx.y, b = blockIdx.z, lane = threadIdx.x;
    int start;
    const int n = seg_rows(seg_start, seg_count, b, N, cap, &start);
    if (cb < rb || cb * 64 >= n) return;                           // (uniform; rb <= cb, so rb * 64 < n too)
    const float unit = labels ? __fadd_rn(max_coord[b], 1.f) : 0.f;
    const int row = rb * 64 + lane;
    cols[lane] = nms_box(boxes, order, labels, unit, start, cb * 64 + lane, n, N);
    const Box mine = rb == cb ? cols[lane] : nms_box(boxes, order, labels, unit, start, row, n, N);
    __syncthreads();
    unsigned long long word = 0ULL;
    for (int j = 0; j < 64; ++j) {
        const int col = cb * 64 + j;
        if (col > row && col < n && box_iou(mine, cols[j]) > iou_thresh) word |= 1ULL << j;
    }
    mask[((size_t)b * cap + row) * (cap / 64) + cb] = word;         // row < cap: rb < cap / 64 by the grid
}

__global__ __launch_bounds__(DP_THREADS) void nms_scan_kernel(const unsigned long long* __restrict__ mask, const long long* __restrict__ order,
                                                              const int* __restrict__ seg_start, const int* __restrict__ seg_count, int N,
                                                              int cap, int max_keep, int* __restrict__ kept, int* __restrict__ n_kept,
                                                              unsigned char* __restrict__ keep_flags) {
    __shared__ unsigned long long removed[NMS_MAX_BLOCKS];
    __shared__ unsigned long long kept_word;
    const int b = blockIdx.x, tid = threadIdx.x;
    int start;
    const int n = seg_rows(seg_start, seg_count, b, N, cap, &start);
    const int nb = (n + 63) / 64, nblk = cap / 64;
    for (int i = tid; i < nb; i += DP_THREADS) removed[i] = 0ULL;
    for (int j = tid; j < max_keep; j += DP_THREADS) kept[(size_t)b * max_keep + j] = -1;
    __syncthreads();
    int total = 0;
    for (int rb = 0; rb < nb && total < max_keep; ++rb) {
        if (tid < 64) {                                            // wave 0, all 64 lanes: the diagonal tile, resolved in registers
            const int row = rb * 64 + tid;
            const unsigned long long d = row < n ? mask[((size_t)b * cap + row) * nblk + rb] : 0ULL;
            const int lo = (int)(unsigned)d, hi = (int)(unsigned)(d >> 32);
            const int left = n - rb * 64;
            unsigned long long alive = ~removed[rb] & (left >= 64 ? ~0ULL : (1ULL << left) - 1ULL);
#pragma unroll
            for (int i = 0; i < 64; ++i) {                         // row i is kept when nothing kept before it removed it; its word has bits > i only
                const unsigned long long di = (unsigned long long)(unsigned)__builtin_amdgcn_readlane(lo, i) |
                                              ((unsigned long long)(unsigned)__builtin_amdgcn_readlane(hi, i) << 32);
                if ((alive >> i) & 1ULL) alive &= ~di;
            }
            while (__popcll(alive) > max_keep - total) alive &= ~(1ULL << (63 - __clzll((long long)alive)));   // the cut: lowest rows first
            if ((alive >> tid) & 1ULL) {
                const long long idx = order ? order[start + row] : (long long)(start + row);
                kept[(size_t)b * max_keep + total + __popcll(alive & ((1ULL << tid) - 1ULL))] = (int)idx;
                if (keep_flags && idx >= 0 && idx < N) keep_flags[idx] = 1;
            }
            if (tid == 0) kept_word = alive;
        }
        __syncthreads();
        const unsigned long long kw = kept_word;
        total += __popcll(kw);
        if (total < max_keep) {
            for (int cb = rb + 1 + tid; cb < nb; cb += DP_THREADS) {   // one thread per later column block: no atomics
                unsigned long long acc = 0ULL, w = kw;
                while (w) {
                    const int i = __ffsll((long long)w) - 1;
                    w &= w - 1ULL;
                    acc |= mask[((size_t)b * cap + rb * 64 + i) * nblk + cb];
                }
                removed[cb] |= acc;
            }
        }
        __syncthreads();
    }
    if (tid == 0) n_kept[b] = total;
}

__global__ __launch_bounds__(DP_THREADS) void det_gather_kernel(const int* __restrict__ kept, const int* __restrict__ n_kept,
                                                                const int* __restrict__ counts, const float* __restrict__ cand_boxes,
                                                                const float* __restrict__ cand_scores, const int* __restrict__ cand_labels,
                                                                const int* __restrict__ cand_src, const float* __restrict__ ratios, int B,
                                                                int cap, int max_keep, float* __restrict__ boxes_net,
                                                                float* __restrict__ boxes_frame, int* __restrict__ src, int* __restrict__ packed) {
    const long at = (long)blockIdx.x * DP_THREADS + threadIdx.x;
    const long rows = (long)B * max_keep;
    if (at < B) { packed[at] = counts[at]; packed[B + at] = n_kept[at]; }
    if (at >= rows) return;
    const int b = (int)(at / max_keep), j = (int)(at - (long)b * max_keep);
    const long idx = kept[at];
    const bool ok = j < n_kept[b] && idx >= (long)b * cap && idx < (long)(b + 1) * cap;
    Box v = {0.f, 0.f, 0.f, 0.f};
    int label = -1, s = -1;
    unsigned sbits = 0u;
    if (ok) {
        v = load_box(cand_boxes, idx);
        label = cand_labels[idx]; s = cand_src[idx]; sbits = __float_as_uint(cand_scores[idx]);
    }
    const float rw = ratios[2 * b], rh = ratios[2 * b + 1];
    store_box(boxes_net, at, v);
    store_box(boxes_frame, at, {__fmul_rn(v.x1, rw), __fmul_rn(v.y1, rh), __fmul_rn(v.x2, rw), __fmul_rn(v.y2, rh)});
    src[at] = s;
    packed[2 * B + at] = label;
    packed[2 * B + rows + at] = (int)sbits;
}

// float -> int as torch's .to(int64) truncates, for any float: NaN gives 0, the rest is clamped to +-2^29 (the frame has fewer than 2^30 pixels: a
// box that far out covers or misses it either way, and every sum and difference below stays inside int)
__device__ __forceinline__ int trunc_box(float v) {
    if (v != v) return 0;
    return v >= 536870912.f ? (1 << 29) : v <= -536870912.f ? -(1 << 29) : (int)v;
}

struct PasteAxis { int i0, i1; float l0, l1; };

// torch's upsample_bilinear2d(align_corners=False) along one axis: n_in taps, n_out outputs, scale = float(n_in) / float(n_out)
__device__ __forceinline__ PasteAxis paste_axis(int dst, float scale, int n_in) {
    float s = __fsub_rn(__fmul_rn(scale, __fadd_rn((float)dst, 0.5f)), 0.5f);
    s = s < 0.f ? 0.f : s;
    int i0 = (int)s;
    i0 = i0 < n_in - 1 ? i0 : n_in - 1;
    PasteAxis a;
    a.i0 = i0; a.i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
    a.l1 = __fsub_rn(s, (float)i0); a.l0 = __fsub_rn(1.f, a.l1);
    return a;
}

template <int V>
__global__ __launch_bounds__(DP_THREADS) void paste_masks_kernel(const float* __restrict__ mask_logits, const float* __restrict__ boxes,
                                                                 const int* __restrict__ labels, int C, int M, int H, int W, float mask_th,
                                                                 unsigned char* __restrict__ out) {
    __shared__ float sm[(PASTE_MAX_M + 2) * (PASTE_MAX_M + 2)];
    const int d = blockIdx.y, tid = threadIdx.x;
    const int P = M + 2;
    const long plane = (long)H * W;
    const long chunk0 = (long)blockIdx.x * (DP_THREADS * PASTE_ITERS * V);
    const long chunk1 = chunk0 + DP_THREADS * PASTE_ITERS * V < plane ? chunk0 + DP_THREADS * PASTE_ITERS * V : plane;
    // the box, expanded by the padding's share and truncated toward zero (expand_boxes + .to(int64))
    const Box roi = load_box(boxes, d);
    const float scale = __fdiv_rn((float)P, (float)M);
    const float xc = __fmul_rn(__fadd_rn(roi.x2, roi.x1), 0.5f), yc = __fmul_rn(__fadd_rn(roi.y2, roi.y1), 0.5f);
    const float wh = __fmul_rn(__fmul_rn(__fsub_rn(roi.x2, roi.x1), 0.5f), scale), hh = __fmul_rn(__fmul_rn(__fsub_rn(roi.y2, roi.y1), 0.5f), scale);
    const int bx1 = trunc_box(__fsub_rn(xc, wh)), by1 = trunc_box(__fsub_rn(yc, hh));
    const int bx2 = trunc_box(__fadd_rn(xc, wh)), by2 = trunc_box(__fadd_rn(yc, hh));
    const int bw = bx2 - bx1 + 1 > 1 ? bx2 - bx1 + 1 : 1, bh = by2 - by1 + 1 > 1 ? by2 - by1 + 1 : 1;
    const int xa = bx1 > 0 ? bx1 : 0, xb = bx2 + 1 < W ? bx2 + 1 : W;         // frame columns [xa, xb) and rows [ya, yb) take the mask
    const int ya = by1 > 0 ? by1 : 0, yb = by2 + 1 < H ? by2 + 1 : H;
    const int label = labels[d];
    const int row_first = (int)(chunk0 / W), row_last = (int)((chunk1 - 1) / W);    // (chunk0 < plane by the grid)
    const bool touches = label >= 0 && label < C && xa < xb && ya < yb && row_last >= ya && row_first < yb;   // uniform over the workgroup
    if (touches) {
        const float* src = mask_logits + ((size_t)d * C + label) * M * M;
        for (int i = tid; i < P * P; i += DP_THREADS) {
            const int py = i / P - 1, px = i % P - 1;
            float v = 0.f;
            if (py >= 0 && py < M && px >= 0 && px < M) v = __fdiv_rn(1.f, __fadd_rn(1.f, expf(-src[py * M + px])));
            sm[i] = v;
        }
        __syncthreads();
    }
    const float sx = __fdiv_rn((float)P, (float)bw), sy = __fdiv_rn((float)P, (float)bh);
    const bool outside = 0.f > mask_th;
    unsigned char* o = out + (size_t)d * plane;
    for (int k = 0; k < PASTE_ITERS; ++k) {
        const long at = chunk0 + ((long)k * DP_THREADS + tid) * V;
        if (at >= plane) break;
        int y = (int)(at / W), x = (int)(at - (long)y * W);
        unsigned r[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < V; ++j) {                               // (V = 16 only where plane % 16 == 0: all 16 pixels lie in the plane)
            bool on = outside;                                      // a pixel the box does not reach holds the value 0
            if (touches && x >= xa && x < xb && y >= ya && y < yb) {
                const PasteAxis ay = paste_axis(y - by1, sy, P), ax = paste_axis(x - bx1, sx, P);
                const float top = __fadd_rn(__fmul_rn(ax.l0, sm[ay.i0 * P + ax.i0]), __fmul_rn(ax.l1, sm[ay.i0 * P + ax.i1]));
                const float bot = __fadd_rn(__fmul_rn(ax.l0, sm[ay.i1 * P + ax.i0]), __fmul_rn(ax.l1, sm[ay.i1 * P + ax.i1]));
                const float v = __fadd_rn(__fmul_rn(ay.l0, top), __fmul_rn(ay.l1, bot));
                on = v > mask_th;
            }
            r[j / 4] |= (unsigned)on << (8 * (j % 4));
            if (++x == W) { x = 0; ++y; }
        }
        if (V == 16) *reinterpret_cast<uint4*>(o + at) = make_uint4(r[0], r[1], r[2], r[3]);
        else o[at] = (unsigned char)r[0];
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace
}  // namespace cosy

using namespace cosy;

extern "C" {

int cosy_nms_max_candidates(void) { return NMS_MAX_CAP; }

int cosy_det_decode(const float* class_logits, const float* box_regression, const float* proposals, const int* prop_offsets,
                    const float* net_sizes, int R, int C, int B, float score_thresh, int cap, float* cand_boxes, float* cand_scores,
                    int* cand_labels, int* cand_src, long long* cand_keys, int* counts, float* max_coord, cosy_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    COSY_REQUIRE(R >= 0 && B >= 0, "cosy_det_decode: R=%d B=%d", R, B);
    COSY_REQUIRE(C >= 2 && C <= 4096, "cosy_det_decode: C=%d outside [2, 4096] (background + at least one class)", C);
    COSY_REQUIRE(B <= ARENA_MAX_IMAGES, "cosy_det_decode: B=%d exceeds %d images per call", B, ARENA_MAX_IMAGES);
    if (int rc = arena_cap_args("cosy_det_decode", cap)) return rc;
    COSY_REQUIRE((long)R * (C - 1) <= (1L << DP_KEY_INDEX_BITS), "cosy_det_decode: R (C-1) = %ld exceeds 2^%d candidates per call", (long)R * (C - 1), DP_KEY_INDEX_BITS);
    COSY_REQUIRE(score_thresh >= 0.f, "cosy_det_decode: score_thresh=%g is negative or NaN", (double)score_thresh);
    if (B == 0) return COSY_OK;
    COSY_REQUIRE_PTR("cosy_det_decode", cand_keys); COSY_REQUIRE_PTR("cosy_det_decode", counts); COSY_REQUIRE_PTR("cosy_det_decode", max_coord);
    if (R > 0) {                                                   // every check before the first launch: a refused call leaves nothing behind
        COSY_REQUIRE_PTR("cosy_det_decode", class_logits); COSY_REQUIRE_PTR("cosy_det_decode", box_regression); COSY_REQUIRE_PTR("cosy_det_decode", proposals);
        COSY_REQUIRE_PTR("cosy_det_decode", prop_offsets); COSY_REQUIRE_PTR("cosy_det_decode", net_sizes);
        COSY_REQUIRE_PTR("cosy_det_decode", cand_boxes); COSY_REQUIRE_PTR("cosy_det_decode", cand_scores);
        COSY_REQUIRE_PTR("cosy_det_decode", cand_labels); COSY_REQUIRE_PTR("cosy_det_decode", cand_src);
    }
    hipLaunchKernelGGL(detpost_init_kernel, dim3(cdiv((long)B * cap, DP_THREADS)), dim3(DP_THREADS), 0, s, cand_keys, counts, (unsigned*)max_coord, B, cap);
    COSY_CHECK_HIP(hipGetLastError());
    if (R == 0) return COSY_OK;
    hipLaunchKernelGGL(det_decode_kernel, dim3(cdiv(R, DP_THREADS)), dim3(DP_THREADS), 0, s, class_logits, box_regression, proposals, prop_offsets,
                       net_sizes, R, C, B, score_thresh, cap, cand_boxes, cand_scores, cand_labels, cand_src, cand_keys, counts, (unsigned*)max_coord);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

static int nms_args(const char* fn, int B, int N, int cap, const void* seg_start, const void* seg_count) {
    COSY_REQUIRE(B >= 0 && N >= 0, "%s: B=%d N=%d", fn, B, N);
    COSY_REQUIRE(B <= COSY_MAX_GRID_Y, "%s: B=%d exceeds %d segments per call", fn, B, COSY_MAX_GRID_Y);
    if (int rc = arena_cap_args(fn, cap)) return rc;
    COSY_REQUIRE(B == 0 || (seg_start != nullptr && seg_count != nullptr), "%s: null seg_start / seg_count", fn);
    return COSY_OK;
}

int cosy_nms_mask(const float* boxes, const long long* order, const int* labels, const float* max_coord, const int* seg_start,
                  const int* seg_count, int B, int N, int cap, float iou_thresh, unsigned long long* mask, cosy_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    if (int rc = nms_args("cosy_nms_mask", B, N, cap, seg_start, seg_count)) return rc;
    COSY_REQUIRE(labels == nullptr || max_coord != nullptr, "cosy_nms_mask: labels without max_coord");
    if (B == 0 || N == 0) return COSY_OK;
    COSY_REQUIRE_PTR("cosy_nms_mask", boxes); COSY_REQUIRE_PTR("cosy_nms_mask", mask);
    COSY_REQUIRE(((uintptr_t)mask & 7) == 0, "cosy_nms_mask: mask not 8-byte aligned");
    hipLaunchKernelGGL(nms_mask_kernel, dim3(cap / 64, cap / 64, B), dim3(64), 0, s, boxes, order, labels, max_coord, seg_start, seg_count, N, cap,
                       iou_thresh, mask);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

int cosy_nms_scan(const unsigned long long* mask, const long long* order, const int* seg_start, const int* seg_count, int B, int N, int cap,
                  int max_keep, int* kept, int* n_kept, unsigned char* keep_flags, cosy_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    if (int rc = nms_args("cosy_nms_scan", B, N, cap, seg_start, seg_count)) return rc;
    COSY_REQUIRE(max_keep >= 0, "cosy_nms_scan: max_keep=%d", max_keep);
    if (B == 0) return COSY_OK;
    COSY_REQUIRE_PTR("cosy_nms_scan", n_kept);
    COSY_REQUIRE(max_keep == 0 || kept != nullptr, "cosy_nms_scan: null kept");
    COSY_REQUIRE(N == 0 || mask != nullptr, "cosy_nms_scan: null mask");
    COSY_REQUIRE(((uintptr_t)mask & 7) == 0, "cosy_nms_scan: mask not 8-byte aligned");
    if (keep_flags && N > 0) COSY_CHECK_HIP(hipMemsetAsync(keep_flags, 0, (size_t)N, s));
    hipLaunchKernelGGL(nms_scan_kernel, dim3(B), dim3(DP_THREADS), 0, s, mask, order, seg_start, seg_count, N, cap, max_keep, kept, n_kept, keep_flags);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

int cosy_det_gather(const int* kept, const int* n_kept, const int* counts, const float* cand_boxes, const float* cand_scores,
                    const int* cand_labels, const int* cand_src, const float* ratios, int B, int cap, int max_keep, float* boxes_net,
                    float* boxes_frame, int* src, int* packed, cosy_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    COSY_REQUIRE(B >= 0 && B <= ARENA_MAX_IMAGES && max_keep >= 0, "cosy_det_gather: B=%d max_keep=%d", B, max_keep);
    if (int rc = arena_cap_args("cosy_det_gather", cap, false)) return rc;
    COSY_REQUIRE((long)B * max_keep < (1L << 30), "cosy_det_gather: %d x %d rows are too many", B, max_keep);
    if (B == 0) return COSY_OK;
    COSY_REQUIRE_PTR("cosy_det_gather", n_kept); COSY_REQUIRE_PTR("cosy_det_gather", counts); COSY_REQUIRE_PTR("cosy_det_gather", packed);
    COSY_REQUIRE_PTR("cosy_det_gather", ratios);
    if (max_keep > 0) {
        COSY_REQUIRE_PTR("cosy_det_gather", kept); COSY_REQUIRE_PTR("cosy_det_gather", cand_boxes); COSY_REQUIRE_PTR("cosy_det_gather", cand_scores);
        COSY_REQUIRE_PTR("cosy_det_gather", cand_labels); COSY_REQUIRE_PTR("cosy_det_gather", cand_src);
        COSY_REQUIRE_PTR("cosy_det_gather", boxes_net); COSY_REQUIRE_PTR("cosy_det_gather", boxes_frame); COSY_REQUIRE_PTR("cosy_det_gather", src);
    }
    const long threads = (long)B * max_keep > B ? (long)B * max_keep : B;
    hipLaunchKernelGGL(det_gather_kernel, dim3(cdiv(threads, DP_THREADS)), dim3(DP_THREADS), 0, s, kept, n_kept, counts, cand_boxes, cand_scores,
                       cand_labels, cand_src, ratios, B, cap, max_keep, boxes_net, boxes_frame, src, packed);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

int cosy_paste_masks(const float* mask_logits, const float* boxes, const int* labels, int D, int C, int M, int H, int W, float mask_th,
                     unsigned char* out, cosy_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    COSY_REQUIRE(D >= 0 && C >= 1 && H > 0 && W > 0, "cosy_paste_masks: D=%d C=%d H=%d W=%d", D, C, H, W);
    COSY_REQUIRE(M >= 1 && M <= PASTE_MAX_M, "cosy_paste_masks: M=%d outside [1, %d]", M, PASTE_MAX_M);
    COSY_REQUIRE(D <= COSY_MAX_GRID_Y, "cosy_paste_masks: D=%d exceeds %d detections per call", D, COSY_MAX_GRID_Y);
    COSY_REQUIRE((long)H * W < (1L << 30), "cosy_paste_masks: a frame of %d x %d is too large", H, W);
    if (D == 0) return COSY_OK;
    COSY_REQUIRE_PTR("cosy_paste_masks", mask_logits); COSY_REQUIRE_PTR("cosy_paste_masks", boxes); COSY_REQUIRE_PTR("cosy_paste_masks", labels);
    COSY_REQUIRE_PTR("cosy_paste_masks", out);
    const long plane = (long)H * W;
    const bool wide = plane % 16 == 0 && aligned16(out);
    const dim3 grid(cdiv(plane, (long)DP_THREADS * PASTE_ITERS * (wide ? 16 : 1)), D);
    if (wide) hipLaunchKernelGGL(paste_masks_kernel<16>, grid, dim3(DP_THREADS), 0, s, mask_logits, boxes, labels, C, M, H, W, mask_th, out);
    else hipLaunchKernelGGL(paste_masks_kernel<1>, grid, dim3(DP_THREADS), 0, s, mask_logits, boxes, labels, C, M, H, W, mask_th, out);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

}  // extern "C"
