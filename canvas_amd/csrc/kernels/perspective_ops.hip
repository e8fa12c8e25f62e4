// perspective_ops.hip -- VideoCornerPinFilter: a projective warp of un-premultiplied RGBA device frames, the bilinear filter
// weighted by alpha.
//
// No reference code; the contract is DESIGN.md "Corner pin" and the comment of include/canvas_perspective.h, restated here.
// Coordinates are RELATIVE: `w` is the window written minus the target origin, `s` the source's current window minus the source
// origin (host/perspective.c forms both in 64 bit and refuses a coordinate beyond +-2^23, so every one is an exact float), h the
// TARGET -> SOURCE coefficients between the two.  In f32 (a half widened exactly), every operation rounded on its own in BOTH
// arithmetic flavours (one build of the unit: not in FMA_KERN):
//     x, y = (float) of the target pixel's relative coordinates
//     nu = (h0*x + h1*y) + h2;  nv = (h3*x + h4*y) + h5;  w = (h6*x + h7*y) + h8
//     not (w > 0):  out = 0            on or beyond the vanishing line, where the plane folds back, and NaN
//     u = nu / w;  v = nv / w          IEEE divides
//     then nearest / bilinear word for word as transform_ops.hip, in(i, j) tested against `s`, source(i, j) the pixel `s`dx + i
//     columns and `s`dy + j rows from the source view's first.
// The tap code is transform_ops.hip's: a tap coordinate is turned into an integer only after it has been clamped into `s` as a
// float, so NaN, +-Inf (w == 0 makes them) and values no int holds never reach a conversion and no address is formed outside
// the source's window, whatever h holds; a tap outside loads the clamped address and a select drops what it would have added.
// The w > 0 rule is a select on the finished pixel as well: a wave does not diverge at the vanishing line.
//
// Shape, as the affine kernel measured and kept (DESIGN.md "Affine transform"): a 256-lane workgroup owns a 32 x 8 tile of
// target pixels, lanes along x first (a wave covers a 32 x 2 patch whose source footprint is compact under any map), one pixel
// per lane, taps straight from global memory (one 16-byte load per f32 tap, one 8-byte load per half tap), non-temporal stores,
// bands of kMaxGridY rows of tiles per launch.  Four instances: f32 / f16 x nearest / bilinear.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "pixel_math.hpp"
#include "stream_common.hpp"

namespace {

using rowstream::v2;
using rowstream::v4;
using rowstream::rect_empty;
using rowstream::kMaxGridY;

constexpr int kThreads = 256, kTileW = 32, kTileH = 8, kTileShift = 5;

struct Px { v4 raw; cvs::px32 f; };                             // raw: the pixel's own dwords (two of them for a half pixel)

template <int HALF>
__device__ __forceinline__ Px load(const cvk_perspective_params &pp, int i, int j) {
    const char *p = static_cast<const char *>(pp.in.data) + ((pp.sdy + j) * pp.in.pitch + (pp.sdx + i)) * (HALF ? 8 : 16);
    if (HALF) {
        const v2 t = *reinterpret_cast<const v2 *>(p);
        return Px{ v4{ t.x, t.y, 0u, 0u }, cvs::widen(make_uint2(t.x, t.y)) };
    }
    const v4 t = *reinterpret_cast<const v4 *>(p);
    return Px{ t, cvs::px32{ __uint_as_float(t.x), __uint_as_float(t.y), __uint_as_float(t.z), __uint_as_float(t.w) } };
}

template <int HALF>
__device__ __forceinline__ void store(const cvk_perspective_params &pp, int x, int y, v4 raw) {
    char *p = static_cast<char *>(pp.out.data) + ((pp.tdy + y) * pp.out.pitch + (pp.tdx + x)) * (HALF ? 8 : 16);
    if (HALF) __builtin_nontemporal_store(v2{ raw.x, raw.y }, reinterpret_cast<v2 *>(p));
    else __builtin_nontemporal_store(raw, reinterpret_cast<v4 *>(p));
}

__device__ __forceinline__ float clampf(float t, float lo, float hi) { return fminf(fmaxf(t, lo), hi); }   // a NaN comes out as lo

struct Sum { float a, r, g, b; };
__device__ __forceinline__ void tap(Sum &s, float w, const cvs::px32 &p, bool inside) {
    const float q = w * p.a;
    const float a = s.a + q, r = s.r + q * p.r, g = s.g + q * p.g, b = s.b + q * p.b;
    s.a = inside ? a : s.a; s.r = inside ? r : s.r; s.g = inside ? g : s.g; s.b = inside ? b : s.b;
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
    const float u = nu / w, v = nv / w;
    const float sx0 = (float)pp.s.x0, sx1 = (float)pp.s.x1, sy0 = (float)pp.s.y0, sy1 = (float)pp.s.y1;
    const v4 zero = { 0u, 0u, 0u, 0u };

    if (!BILINEAR) {
        const float fi = floorf(u + 0.5f), fj = floorf(v + 0.5f);
        const bool inside = fi >= sx0 && fi <= sx1 && fj >= sy0 && fj <= sy1;
        const Px p = load<HALF>(pp, (int)clampf(fi, sx0, sx1), (int)clampf(fj, sy0, sy1));
        store<HALF>(pp, x, y, (inside && front) ? p.raw : zero);
        return;
    }

    const float fi = floorf(u), fj = floorf(v), fi1 = fi + 1.0f, fj1 = fj + 1.0f;
    const float a = u - fi, b = v - fj, wa = 1.0f - a, wb = 1.0f - b;
    const bool x0in = fi >= sx0 && fi <= sx1, x1in = fi1 >= sx0 && fi1 <= sx1;
    const bool y0in = fj >= sy0 && fj <= sy1, y1in = fj1 >= sy0 && fj1 <= sy1;
    const int j0 = (int)clampf(fj, sy0, sy1), j1 = (int)clampf(fj1, sy0, sy1);
    const int i0 = (int)clampf(fi, sx0, sx1), i1 = (int)clampf(fi1, sx0, sx1);
    const Px p00 = load<HALF>(pp, i0, j0);
    const Px p10 = load<HALF>(pp, i1, j0);
    const Px p01 = load<HALF>(pp, i0, j1);
    const Px p11 = load<HALF>(pp, i1, j1);
    Sum s = { 0.0f, 0.0f, 0.0f, 0.0f };
    tap(s, wa * wb, p00.f, x0in && y0in);
    tap(s, a * wb, p10.f, x1in && y0in);
    tap(s, wa * b, p01.f, x0in && y1in);
    tap(s, a * b, p11.f, x1in && y1in);
    v4 o = zero;
    if (s.a != 0.0f) {
        const cvs::px32 c = { s.r / s.a, s.g / s.a, s.b / s.a, s.a };
        if (HALF) { const uint2 n = cvs::narrow(c); o = v4{ n.x, n.y, 0u, 0u }; }
        else o = v4{ __float_as_uint(c.r), __float_as_uint(c.g), __float_as_uint(c.b), __float_as_uint(c.a) };
    }
    if (a == 0.0f && b == 0.0f) o = (x0in && y0in) ? p00.raw : zero;   // on a sample: a copy
    store<HALF>(pp, x, y, front ? o : zero);
}

template <int HALF, int BILINEAR>
int launch(const cvk_perspective_params &pp, hipStream_t st) {
    const long long cols = (long long)pp.w.x1 - pp.w.x0 + 1, rows = (long long)pp.w.y1 - pp.w.y0 + 1;
    const long long tiles = (rows + kTileH - 1) / kTileH;
    // a window of any height: bands of at most kMaxGridY rows of tiles, one launch each (a tile depends on nothing but its
    // own coordinates, so a band is the same kernel on a window that starts further down)
    for (long long first = 0; first < tiles; first += kMaxGridY) {
        const long long n = tiles - first < kMaxGridY ? tiles - first : kMaxGridY;
        cvk_perspective_params band = pp;
        band.w.y0 = (int)(pp.w.y0 + first * kTileH);
        const long long last = (long long)band.w.y0 + n * kTileH - 1;
        band.w.y1 = last < pp.w.y1 ? (int)last : pp.w.y1;
        const dim3 grid((unsigned)((cols + kTileW - 1) / kTileW), (unsigned)n, 1);
        hipLaunchKernelGGL((k_perspective<HALF, BILINEAR>), grid, dim3(kThreads), 0, st, band);
        const int rc = (int)hipGetLastError();
        if (rc != 0) return rc;
    }
    return 0;
}

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
