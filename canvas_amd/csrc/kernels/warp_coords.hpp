// warp_coords.hpp -- what the units of one warp share BEFORE the filter: the source coordinates (u, v) of a target pixel, where
// the pixels of the two views lie, and the launchers' checks of their parameters.  transform_ops.hip and perspective_ops.hip hold
// the nearest and the bilinear kernels, warp_cubic_ops.hip the Catmull-Rom kernels of both warps; the arithmetic is stated in the
// head of transform_ops.hip (affine) and perspective_ops.hip (corner pin) and is written once, here.
#pragma once
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "stream_common.hpp"

namespace warp {

// ---------------------------------------------------------------- the affine warp: coordinates ABSOLUTE

// pixel (i, j) of a view
template <int HALF>
__device__ __forceinline__ char *affine_address(const cvk_view &f, int i, int j) {
    return static_cast<char *>(f.data) + ((long long)(j - f.fy0) * f.pitch + (i - f.fx0)) * (HALF ? 8 : 16);
}

// the target pixel of this lane in a tw x th tile (lanes along x first), false beyond the window
__device__ __forceinline__ bool affine_pixel(const cvk_transform_params &tp, int &x, int &y) {
    const int shift = __builtin_ctz((unsigned)tp.tw);
    const int lx = (int)threadIdx.x & (tp.tw - 1), ly = (int)threadIdx.x >> shift;
    x = tp.w.x0 + ((int)blockIdx.x << shift) + lx;
    y = tp.w.y0 + (int)blockIdx.y * tp.th + ly;
    return x <= tp.w.x1 && y <= tp.w.y1;
}

__device__ __forceinline__ void affine_uv(const float (&m)[6], int x, int y, float &u, float &v) {
    const float fx = (float)x, fy = (float)y;
    u = (m[0] * fx + m[1] * fy) + m[2];
    v = (m[3] * fx + m[4] * fy) + m[5];
}

// what cvk_transform and cvk_transform_cubic refuse: 0, or the HIP error
inline int transform_params_refused(const cvk_transform_params &tp, int threads) {
    if (rowstream::rect_empty(tp.s) || tp.tw < 8 || tp.tw > threads || (tp.tw & (tp.tw - 1)) || tp.tw * tp.th != threads) return (int)hipErrorInvalidValue;
    // the window written inside the target's buffer, the source window inside the source's: nothing else is ever addressed
    if (tp.w.x0 < tp.out.fx0 || tp.w.y0 < tp.out.fy0 || tp.w.x1 > tp.out.fx1 || tp.w.y1 > tp.out.fy1) return (int)hipErrorInvalidValue;
    if (tp.s.x0 < tp.in.fx0 || tp.s.y0 < tp.in.fy0 || tp.s.x1 > tp.in.fx1 || tp.s.y1 > tp.in.fy1) return (int)hipErrorInvalidValue;
    return 0;
}

// ---------------------------------------------------------------- the corner pin: coordinates RELATIVE to the two origins

constexpr int kPinTileW = 32, kPinTileH = 8, kPinTileShift = 5;

// relative pixel (x, y) of a view whose first pixel is (-dx, -dy)
template <int HALF>
__device__ __forceinline__ char *pinned_address(const cvk_view &f, long long dx, long long dy, int x, int y) {
    return static_cast<char *>(f.data) + ((dy + y) * f.pitch + (dx + x)) * (HALF ? 8 : 16);
}

__device__ __forceinline__ bool pinned_pixel(const cvk_perspective_params &pp, int &x, int &y) {
    const int lx = (int)threadIdx.x & (kPinTileW - 1), ly = (int)threadIdx.x >> kPinTileShift;
    x = pp.w.x0 + ((int)blockIdx.x << kPinTileShift) + lx;
    y = pp.w.y0 + (int)blockIdx.y * kPinTileH + ly;
    return x <= pp.w.x1 && y <= pp.w.y1;
}

// u, v of the pixel, and whether it is drawn at all: not on or beyond the vanishing line (false for a NaN w).  u and v of a pixel
// that is not drawn may be NaN or +-Inf: the filters clamp before they convert
__device__ __forceinline__ bool pinned_uv(const float (&h)[9], int x, int y, float &u, float &v) {
    const float fx = (float)x, fy = (float)y;
    const float nu = (h[0] * fx + h[1] * fy) + h[2], nv = (h[3] * fx + h[4] * fy) + h[5];
    const float w = (h[6] * fx + h[7] * fy) + h[8];
    u = nu / w;
    v = nv / w;
    return w > 0.0f;
}

// r + (dx, dy), the rectangle counted from the view's first pixel, lies inside the view
inline bool inside_view(const cvk_rect &r, long long dx, long long dy, const cvk_view &v) {
    return r.x0 + dx >= 0 && r.y0 + dy >= 0 && r.x1 + dx < v.pitch && r.y1 + dy <= (long long)v.fy1 - v.fy0;
}

// what cvk_perspective and cvk_perspective_cubic refuse: 0, or the HIP error
inline int perspective_params_refused(const cvk_perspective_params &pp) {
    if (rowstream::rect_empty(pp.s)) return (int)hipErrorInvalidValue;
    const int span = 1 << 23;
    if (pp.w.x0 < -span || pp.w.y0 < -span || pp.w.x1 > span || pp.w.y1 > span || pp.s.x0 < -span || pp.s.y0 < -span || pp.s.x1 > span || pp.s.y1 > span)
        return (int)hipErrorInvalidValue;
    // the window written inside the target's buffer, the source window inside the source's: nothing else is ever addressed
    if (!inside_view(pp.w, pp.tdx, pp.tdy, pp.out) || !inside_view(pp.s, pp.sdx, pp.sdy, pp.in)) return (int)hipErrorInvalidValue;
    return 0;
}

}  // namespace warp
