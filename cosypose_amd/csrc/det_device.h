// Box IoU with torchvision.ops.box_iou's float32 arithmetic, shared by kernels_det.hip (box_iou / box_iou_pairs) and kernels_detpost.hip
// (the suppression matrix of NMS): one definition, so a keep set of NMS is decided by exactly the bits box_iou returns.
// Every operation is rounded to float32 on its own; both files are compiled with contraction off.
#pragma once
#include <hip/hip_runtime.h>

namespace cosy {

// torch.max / torch.min / clamp(min=0): a NaN operand gives NaN (fmaxf / fminf would drop it)
__device__ __forceinline__ float max_nan(float a, float b) { return a != a ? a : b != b ? b : a > b ? a : b; }
__device__ __forceinline__ float min_nan(float a, float b) { return a != a ? a : b != b ? b : a < b ? a : b; }
__device__ __forceinline__ float clamp0_nan(float a) { return a != a ? a : a < 0.f ? 0.f : a; }

struct Box { float x1, y1, x2, y2; };

// torchvision.ops.box_iou, every operation rounded to float32 on its own
__device__ __forceinline__ float box_iou(const Box& a, const Box& b) {
    const float area_a = __fmul_rn(__fsub_rn(a.x2, a.x1), __fsub_rn(a.y2, a.y1));
    const float area_b = __fmul_rn(__fsub_rn(b.x2, b.x1), __fsub_rn(b.y2, b.y1));
    const float w = clamp0_nan(__fsub_rn(min_nan(a.x2, b.x2), max_nan(a.x1, b.x1)));
    const float h = clamp0_nan(__fsub_rn(min_nan(a.y2, b.y2), max_nan(a.y1, b.y1)));
    const float inter = __fmul_rn(w, h);
    return __fdiv_rn(inter, __fsub_rn(__fadd_rn(area_a, area_b), inter));
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
