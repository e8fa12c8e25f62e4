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
// bands of kMaxGridY rows of tiles per launch.  Four instances: f32 / f16 x nearest / bilinear (the Catmull-Rom filter's two are in
// warp_cubic_ops.hip: this object holds exactly these four).
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "warp_coords.hpp"
#include "warp_sample.hpp"

namespace {

using namespace warp;
using rowstream::rect_empty;

// (the pixel of a lane, u, v and the w > 0 rule, and the addresses: warp_coords.hpp, shared with the Catmull-Rom kernel of
// warp_cubic_ops.hip)
template <int HALF, int BILINEAR>
__global__ __launch_bounds__(kThreads) void k_perspective(cvk_perspective_params pp) {
    int x, y;
    if (!pinned_pixel(pp, x, y)) return;
    float u, v;
    const bool front = pinned_uv(pp.h, x, y, u, v);
    const v4 o = sample<HALF, BILINEAR>(u, v, Window(pp.s), [&](int i, int j) { return pinned_address<HALF>(pp.in, pp.sdx, pp.sdy, i, j); });
    store<HALF>(pinned_address<HALF>(pp.out, pp.tdx, pp.tdy, x, y), front ? o : v4{ 0u, 0u, 0u, 0u });
}

template <int HALF, int BILINEAR>
int launch(const cvk_perspective_params &pp, hipStream_t st) { return launch_bands(k_perspective<HALF, BILINEAR>, pp, kPinTileW, kPinTileH, st); }

}  // namespace

extern "C" int cvk_perspective(const cvk_perspective_params *in, int half, void *stream) {
    const cvk_perspective_params &pp = *in;
    if (rect_empty(pp.w)) return 0;
    const int refused = perspective_params_refused(pp);
    if (refused != 0) return refused;
    hipStream_t st = (hipStream_t)stream;
    if (!pp.bilinear) return half ? launch<1, 0>(pp, st) : launch<0, 0>(pp, st);
    return half ? launch<1, 1>(pp, st) : launch<0, 1>(pp, st);
}
