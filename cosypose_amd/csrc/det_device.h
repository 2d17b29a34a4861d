// What the detector's files must decide alike, to the last bit, one definition each: box_iou (kernels_det.hip's box_iou / box_iou_pairs, the
// suppression matrix of kernels_detpost.hip's NMS -- a keep set is decided by exactly the bits box_iou returns -- and kernels_dettrain.hip's
// matcher), the anchor formed from its index (the proposals kernels_detpre.hip emits and the anchors kernels_dettrain.hip's RPN loss matches
// are the same boxes), BoxCoder's decode (both decode kernels) and encode, the candidate arena's key layout and `cap` rule, the taps of roi_align.
// Every operation is rounded to float32 on its own: the includers are compiled with contraction off (#pragma clang fp contract(off) and
// -ffp-contract=off in build.FILE_FLAGS, which covers this header); the functions here rely on it wherever they do not spell out __f*_rn.
#pragma once
#include <math.h>
#include "cosy_common.h"

namespace cosy {

// torch.max / torch.min / clamp(min=0): a NaN operand gives NaN (fmaxf / fminf would drop it)
__device__ __forceinline__ float max_nan(float a, float b) { return a != a ? a : b != b ? b : a > b ? a : b; }
__device__ __forceinline__ float min_nan(float a, float b) { return a != a ? a : b != b ? b : a < b ? a : b; }
__device__ __forceinline__ float clamp0_nan(float a) { return a != a ? a : a < 0.f ? 0.f : a; }

struct Box { float x1, y1, x2, y2; };
typedef cosy_rpn_levels_t RpnLevels;

// row `row` of an (n,4) xyxy table, four scalar accesses (kernels_det.hip has a float4 form of its own for tables it knows to be aligned)
__device__ __forceinline__ Box load_box(const float* p, size_t row) { return {p[4 * row], p[4 * row + 1], p[4 * row + 2], p[4 * row + 3]}; }
__device__ __forceinline__ void store_box(float* p, size_t row, const Box& b) {
    p[4 * row] = b.x1; p[4 * row + 1] = b.y1; p[4 * row + 2] = b.x2; p[4 * row + 3] = b.y2;
}

// torchvision.ops.box_iou, every operation rounded to float32 on its own
__device__ __forceinline__ float box_iou(const Box& a, const Box& b) {
    const float area_a = __fmul_rn(__fsub_rn(a.x2, a.x1), __fsub_rn(a.y2, a.y1));
    const float area_b = __fmul_rn(__fsub_rn(b.x2, b.x1), __fsub_rn(b.y2, b.y1));
    const float w = clamp0_nan(__fsub_rn(min_nan(a.x2, b.x2), max_nan(a.x1, b.x1)));
    const float h = clamp0_nan(__fsub_rn(min_nan(a.y2, b.y2), max_nan(a.y1, b.y1)));
    const float inter = __fmul_rn(w, h);
    return __fdiv_rn(inter, __fsub_rn(__fadd_rn(area_a, area_b), inter));
}

// anchor idx (in [0, A H W), checked by the caller) of level l = (cell y W + x, a) with a fastest: base[l][a] + (x stride_w, y stride_h) on both corners
__device__ __forceinline__ Box anchor_box(const RpnLevels& lv, int l, int idx, int A) {
    const int W = lv.W[l], pos = idx / A, a = idx - pos * A, y = pos / W, x = pos - y * W;
    const float sx = __fmul_rn((float)x, lv.stride_w[l]), sy = __fmul_rn((float)y, lv.stride_h[l]);
    return {__fadd_rn(lv.base[l][a][0], sx), __fadd_rn(lv.base[l][a][1], sy), __fadd_rn(lv.base[l][a][2], sx), __fadd_rn(lv.base[l][a][3], sy)};
}

// the level table (host) as every entry point that forms anchors checks it; *total: anchors per image, at most 2^20 (the candidate index's bits)
inline int rpn_levels_args(const char* fn, const RpnLevels* lv, int L, int A, long* total) {
    COSY_REQUIRE(lv != nullptr, "%s: null levels", fn);
    COSY_REQUIRE(L >= 1 && L <= COSY_RPN_MAX_LEVELS, "%s: L=%d outside [1, %d] levels", fn, L, COSY_RPN_MAX_LEVELS);
    COSY_REQUIRE(A >= 1 && A <= COSY_RPN_MAX_ANCHORS, "%s: A=%d outside [1, %d] anchors per cell", fn, A, COSY_RPN_MAX_ANCHORS);
    *total = 0;
    for (int l = 0; l < L; ++l) {
        COSY_REQUIRE(lv->H[l] >= 1 && lv->W[l] >= 1, "%s: level %d is %d x %d cells", fn, l, lv->H[l], lv->W[l]);
        *total += (long)A * lv->H[l] * lv->W[l];
        COSY_REQUIRE(*total <= (1L << 20), "%s: more than 2^20 anchors per image (levels 0 .. %d)", fn, l);
    }
    return COSY_OK;
}

constexpr float BBOX_XFORM_CLIP = 4.135166556742356f;            // log(1000 / 16)

// BoxCoder.decode_single followed by clip_boxes_to_image: d = the deltas ALREADY divided by the coder's weights, (net_h, net_w) the image's own size.
// Centre and extent of `ref`, the clamp on dw / dh (a NaN stays NaN), expf, then half extents around the new centre.
__device__ __forceinline__ Box box_decode(const Box& ref, const float d[4], float net_h, float net_w) {
    const float w = __fsub_rn(ref.x2, ref.x1), h = __fsub_rn(ref.y2, ref.y1);
    const float cx = __fadd_rn(ref.x1, __fmul_rn(0.5f, w)), cy = __fadd_rn(ref.y1, __fmul_rn(0.5f, h));
    const float dw = min_nan(d[2], BBOX_XFORM_CLIP), dh = min_nan(d[3], BBOX_XFORM_CLIP);
    const float pcx = __fadd_rn(__fmul_rn(d[0], w), cx), pcy = __fadd_rn(__fmul_rn(d[1], h), cy);
    const float pw = __fmul_rn(expf(dw), w), ph = __fmul_rn(expf(dh), h);
    const float hw = __fmul_rn(0.5f, pw), hh = __fmul_rn(0.5f, ph);
    return {min_nan(max_nan(__fsub_rn(pcx, hw), 0.f), net_w), min_nan(max_nan(__fsub_rn(pcy, hh), 0.f), net_h),
            min_nan(max_nan(__fadd_rn(pcx, hw), 0.f), net_w), min_nan(max_nan(__fadd_rn(pcy, hh), 0.f), net_h)};
}

// BoxCoder.encode_single, the inverse: the targets that take `p` to `ref`; a zero extent gives the IEEE result
__device__ __forceinline__ void box_encode(const Box& ref, const Box& p, float wx, float wy, float ww, float wh, float* t) {
    const float ew = __fsub_rn(p.x2, p.x1), eh = __fsub_rn(p.y2, p.y1);
    const float ecx = __fadd_rn(p.x1, __fmul_rn(0.5f, ew)), ecy = __fadd_rn(p.y1, __fmul_rn(0.5f, eh));
    const float gw = __fsub_rn(ref.x2, ref.x1), gh = __fsub_rn(ref.y2, ref.y1);
    const float gcx = __fadd_rn(ref.x1, __fmul_rn(0.5f, gw)), gcy = __fadd_rn(ref.y1, __fmul_rn(0.5f, gh));
    t[0] = __fdiv_rn(__fmul_rn(wx, __fsub_rn(gcx, ecx)), ew);
    t[1] = __fdiv_rn(__fmul_rn(wy, __fsub_rn(gcy, ecy)), eh);
    t[2] = __fmul_rn(ww, logf(__fdiv_rn(gw, ew)));
    t[3] = __fmul_rn(wh, logf(__fdiv_rn(gh, eh)));
}

// The candidate arena, B x cap slots.  A slot's 64-bit sort key is  image << 52 | score field | candidate index  (the two lower fields are the
// decode kernel's own: widths and score mapping differ); an unused slot holds empty_key(b), which sorts behind every candidate of image b.
constexpr int ARENA_KEY_IMAGE_SHIFT = 52;
constexpr int ARENA_MAX_IMAGES = 2047;                           // 11 bits of image keep the key positive
__device__ __forceinline__ long long empty_key(int b) { return ((long long)b << ARENA_KEY_IMAGE_SHIFT) | ((1LL << ARENA_KEY_IMAGE_SHIFT) - 1); }

// `cap` (host): a multiple of 64 in [64, cosy_nms_max_candidates()] where waves and 64-bit mask words are laid over it; the gathers only index
inline int arena_cap_args(const char* fn, int cap, bool whole_words = true) {
    const int max = cosy_nms_max_candidates();
    if (whole_words) COSY_REQUIRE(cap >= 64 && cap <= max && cap % 64 == 0, "%s: cap=%d is no multiple of 64 in [64, %d]", fn, cap, max);
    else COSY_REQUIRE(cap >= 64 && cap <= max, "%s: cap=%d outside [64, %d]", fn, cap, max);
    return COSY_OK;
}

// one tap line of roi_align along one axis (kernels_geom.hip roi_pixel's rules), shared by kernels_detpre.hip (multi-scale RoIAlign) and
// kernels_dettrain.hip (mask targets): lo < 0 marks a sample outside [-1, size], which adds nothing
struct Tap { int lo, hi; float wl, wh; };

__device__ __forceinline__ Tap msroi_tap(float start, float bin, int p, int i, int g, int size) {
    float v = __fadd_rn(__fadd_rn(start, __fmul_rn((float)p, bin)), __fdiv_rn(__fmul_rn(__fadd_rn((float)i, .5f), bin), (float)g));
    Tap t = {-1, -1, 0.f, 0.f};
    if (!(v >= -1.0f && v <= (float)size)) return t;               // (a NaN sample is outside too)
    if (v <= 0.f) v = 0.f;
    int lo = (int)v, hi;
    if (lo >= size - 1) { hi = lo = size - 1; v = (float)lo; } else hi = lo + 1;
    t.lo = lo; t.hi = hi;
    t.wl = __fsub_rn(v, (float)lo);                                // weight of the high tap
    t.wh = __fsub_rn(1.f, t.wl);                                   // weight of the low tap
    return t;
}

}  // namespace cosy
