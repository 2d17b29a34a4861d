// What kernels_bop.hip and kernels_gt.hip share: the packed depth windows of cosy_bop_render_windows and the float32 depth-to-distance
// function of DESIGN.md section 15.  Both files compile this text with contraction off, so a distance has the same bits in either.
#pragma once
#include "cosy_common.h"

#pragma clang fp contract(off)

namespace cosy {

// empty boxes: x1 = y1 = -1 for an instance that can be drawn, BOX_DEAD for one that cannot (ids outside the tables, a non-finite pose or K):
// a pair with such an instance has no pixels at all, whatever its other instance shows
constexpr int BOX_DEAD = -2;

struct Window {
    long off;         // the instance's window in the store, row-major bw x bh
    long room;        // words of the store from off on
    int x0, y0, bw, bh;
};

// the window of instance n, or bw = 0 when the box is empty or the offset lies outside the store
__device__ __forceinline__ Window window_of(const int* __restrict__ boxes, const long long* __restrict__ win_offset, long n_px, int n, int H, int W) {
    Window w{0, 0, 0, 0, 0, 0};
    const int x0 = boxes[n * 4], y0 = boxes[n * 4 + 1], x1 = boxes[n * 4 + 2], y1 = boxes[n * 4 + 3];
    const long long off = win_offset[n];
    if (x0 < 0 || y0 < 0 || x1 >= W || y1 >= H || x1 < x0 || y1 < y0 || off < 0 || off >= n_px) return w;
    w.off = off; w.room = n_px - off; w.x0 = x0; w.y0 = y0; w.bw = x1 - x0 + 1; w.bh = y1 - y0 + 1;
    return w;
}

// index of frame pixel (x, y) in the store, or -1 outside the window (or past the store: a window that does not fit is never touched there)
__device__ __forceinline__ long window_index(const Window& w, int x, int y) {
    const int wx = x - w.x0, wy = y - w.y0;
    if (wx < 0 || wx >= w.bw || wy < 0 || wy >= w.bh) return -1;
    const long at = (long)wy * w.bw + wx;
    return at < w.room ? w.off + at : -1;
}

__device__ __forceinline__ float window_depth(const Window& w, const float* __restrict__ store, int x, int y) {
    const long at = window_index(w, x, y);
    return at >= 0 ? store[at] : 0.f;
}

// depth -> distance from the camera centre: subtract, multiply, divide; three squares; (X^2 + Y^2) + z^2; square root
__device__ __forceinline__ float depth_to_dist(float z, float xc, float yc, float fx, float fy) {
    const float X = (xc * z) / fx, Y = (yc * z) / fy;
    return sqrtf((X * X + Y * Y) + z * z);
}

}  // namespace cosy
