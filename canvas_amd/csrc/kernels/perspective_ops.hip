// perspective_ops.hip -- VideoCornerPinFilter: a projective warp of un-premultiplied RGBA device frames, the bilinear filter
// weighted by alpha.
//
// No reference code; the contract is DESIGN.md "Corner pin" and the comment of include/canvas_perspective.h.
// Coordinates are RELATIVE: `w` is the window written minus the target origin, `s` the source's current window minus the source
// origin (host/perspective.c forms both in 64 bit and refuses a coordinate beyond +-2^23, so every one is an exact float), h the
// TARGET -> SOURCE coefficients between the two.  In f32, every operation rounded on its own:
//     x, y = (float) of the target pixel's relative coordinates
//     nu = (h0*x + h1*y) + h2;  nv = (h3*x + h4*y) + h5;  w = (h6*x + h7*y) + h8
//     not (w > 0):  out = 0            on or beyond the vanishing line, where the plane folds back, and NaN
//     u = nu / w;  v = nv / w          IEEE divides
// then the nearest or the bilinear filter of warp_sample.hpp, which states the arithmetic from (u, v) on, with S = `s` and
// source(i, j) the pixel `s`dx + i columns and `s`dy + j rows from the source view's first.  Its clamp before any conversion is
// what keeps the NaN and +-Inf that w == 0 makes from ever forming an address outside the source's window, whatever h holds.
// The w > 0 rule is a select on the finished pixel: a wave does not diverge at the vanishing line.
//
// Shape, as the affine kernel measured and kept (DESIGN.md "Affine transform"): a 256-lane workgroup owns a 32 x 8 tile of
// target pixels, lanes along x first (a wave covers a 32 x 2 patch whose source footprint is compact under any map), one pixel
// per lane, taps straight from global memory (one 16-byte load per f32 tap, one 8-byte load per half tap), non-temporal stores,
// bands of kMaxGridY rows of tiles per launch.  Four instances: f32 / f16 x nearest / bilinear.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "warp_sample.hpp"

namespace {

using namespace warp;
using rowstream::rect_empty;

constexpr int kTileW = 32, kTileH = 8, kTileShift = 5;

// relative pixel (x, y) of a view whose first pixel is (-dx, -dy)
template <int HALF>
__device__ __forceinline__ char *address(const cvk_view &f, long long dx, long long dy, int x, int y) {
    return static_cast<char *>(f.data) + ((dy + y) * f.pitch + (dx + x)) * (HALF ? 8 : 16);
}

template <int HALF, int BILINEAR>
__global__ __launch_bounds__(kThreads) void k_perspective(cvk_perspective_params pp) {
    const int lx = (int)threadIdx.x & (kTileW - 1), ly = (int)threadIdx.x >> kTileShift;
    const int x = pp.w.x0 + ((int)blockIdx.x << kTileShift) + lx, y = pp.w.y0 + (int)blockIdx.y * kTileH + ly;
    if (x > pp.w.x1 || y > pp.w.y1) return;
    const float fx = (float)x, fy = (float)y;
    const float nu = (pp.h[0] * fx + pp.h[1] * fy) + pp.h[2], nv = (pp.h[3] * fx + pp.h[4] * fy) + pp.h[5];
    const float w = (pp.h[6] * fx + pp.h[7] * fy) + pp.h[8];
    const bool front = w > 0.0f;                                 // false for NaN
    const v4 o = sample<HALF, BILINEAR>(nu / w, nv / w, Window(pp.s), [&](int i, int j) { return address<HALF>(pp.in, pp.sdx, pp.sdy, i, j); });
    store<HALF>(address<HALF>(pp.out, pp.tdx, pp.tdy, x, y), front ? o : v4{ 0u, 0u, 0u, 0u });
}

template <int HALF, int BILINEAR>
int launch(const cvk_perspective_params &pp, hipStream_t st) { return launch_bands(k_perspective<HALF, BILINEAR>, pp, kTileW, kTileH, st); }

// r + (dx, dy), the rectangle counted from the view's first pixel, lies inside the view
bool inside_view(const cvk_rect &r, long long dx, long long dy, const cvk_view &v) {
    return r.x0 + dx >= 0 && r.y0 + dy >= 0 && r.x1 + dx < v.pitch && r.y1 + dy <= (long long)v.fy1 - v.fy0;
}

}  // namespace

extern "C" int cvk_perspective(const cvk_perspective_params *in, int half, void *stream) {
    const cvk_perspective_params &pp = *in;
    if (rect_empty(pp.w)) return 0;
    if (rect_empty(pp.s)) return (int)hipErrorInvalidValue;
    const int span = 1 << 23;
    if (pp.w.x0 < -span || pp.w.y0 < -span || pp.w.x1 > span || pp.w.y1 > span || pp.s.x0 < -span || pp.s.y0 < -span || pp.s.x1 > span || pp.s.y1 > span)
        return (int)hipErrorInvalidValue;
    // the window written inside the target's buffer, the source window inside the source's: nothing else is ever addressed
    if (!inside_view(pp.w, pp.tdx, pp.tdy, pp.out) || !inside_view(pp.s, pp.sdx, pp.sdy, pp.in)) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    if (!pp.bilinear) return half ? launch<1, 0>(pp, st) : launch<0, 0>(pp, st);
    return half ? launch<1, 1>(pp, st) : launch<0, 1>(pp, st);
}
