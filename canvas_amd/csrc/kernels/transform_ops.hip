// transform_ops.hip -- VideoTransformFilter: an affine warp of un-premultiplied RGBA device frames, the bilinear filter weighted
// by alpha.
//
// No reference code; the contract is DESIGN.md "Affine transform" and the comment of include/canvas_hip.h, restated here.  S = the
// source's current window, `w` the window written, m the TARGET -> SOURCE coefficients.  In f32 (a half widened exactly), every
// operation rounded on its own in BOTH arithmetic flavours (one build of the unit: not in FMA_KERN):
//     x, y = (float) of the target pixel's coordinates;  u = (m0*x + m1*y) + m2;  v = (m3*x + m4*y) + m5
//     in(i, j) = S.x0 <= i <= S.x1 and S.y0 <= j <= S.y1, compared as floats: false for NaN and +-Inf
//     nearest:   i = floorf(u + 0.5f), j = floorf(v + 0.5f);  out = in(i, j) ? source(i, j) code for code : 0
//     bilinear:  i = floorf(u), j = floorf(v);  a = u - i;  b = v - j;  wa = 1 - a;  wb = 1 - b
//                a == 0 and b == 0:  out = in(i, j) ? source(i, j) code for code : 0
//                else A = R = G = B = 0;  for (w, di, dj) in (wa*wb, 0, 0), (a*wb, 1, 0), (wa*b, 0, 1), (a*b, 1, 1):
//                         if in(i + di, j + dj):  p = source(i + di, j + dj);  q = w * p.a;  A += q;  R += q*p.r;  G += q*p.g;  B += q*p.b
//                     out = A != 0 ? (R / A, G / A, B / A, A) : 0                       f16 truncated once at the store
// Every coordinate of S is within +-2^23 (host/transform.c refuses others), so the window's bounds are exact floats, and a tap
// coordinate is turned into an integer only after it has been clamped into S as a float: NaN, +-Inf and values no int holds
// never reach a conversion, and no address is ever formed outside S.  A tap outside S loads the clamped address and a select
// drops what it would have added, so the four taps do not diverge at the layer's edge.
//
// Shape: the reads follow a rotated footprint, so a wave that owned 64 pixels of one row would touch up to 64 source rows.  A
// 256-lane workgroup owns a tw x th tile of target pixels instead (tw * th == 256, planned in host/transform.c; lanes run along x
// first, so a wave covers 64 / tw rows of the tile when tw < 64): under any angle the wave's source footprint is a compact patch
// that the 32 KiB L1 serves, and stores stay lane-contiguous along x.  Taps come straight from global memory: one 16-byte load
// per f32 tap, one 8-byte load per half tap.  The other form of the half taps -- the two horizontally adjacent ones in one 16-byte
// load at 8-byte alignment from the pair's column clamped to S.x0 .. S.x1 - 1, the lane sorting out which half is which (PAIR) --
// measured 1.7 to 1.9 times slower (DESIGN.md "Affine transform", Measured) and exists in the diagnostic build only.
// One pixel per lane, stores non-temporal.  Four instances: f32 / f16 x nearest / bilinear.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "pixel_math.hpp"
#include "stream_common.hpp"

namespace {

using rowstream::v2;
using rowstream::v4;
using rowstream::rect_empty;
using rowstream::kMaxGridY;

constexpr int kThreads = 256;
typedef v4 v4_align8 __attribute__((aligned(8)));

struct Px { v4 raw; cvs::px32 f; };                             // raw: the pixel's own dwords (two of them for a half pixel)

template <int HALF>
__device__ __forceinline__ const char *address(const cvk_view &in, int i, int j) {
    return static_cast<const char *>(in.data) + ((long long)(j - in.fy0) * in.pitch + (i - in.fx0)) * (HALF ? 8 : 16);
}

__device__ __forceinline__ Px from_half(uint32_t lo, uint32_t hi) { return Px{ v4{ lo, hi, 0u, 0u }, cvs::widen(make_uint2(lo, hi)) }; }

template <int HALF>
__device__ __forceinline__ Px load(const cvk_view &in, int i, int j) {
    if (HALF) {
        const v2 t = *reinterpret_cast<const v2 *>(address<1>(in, i, j));
        return from_half(t.x, t.y);
    }
    const v4 t = *reinterpret_cast<const v4 *>(address<0>(in, i, j));
    return Px{ t, cvs::px32{ __uint_as_float(t.x), __uint_as_float(t.y), __uint_as_float(t.z), __uint_as_float(t.w) } };
}

template <int HALF>
__device__ __forceinline__ void store(const cvk_view &out, int x, int y, v4 raw) {
    char *p = static_cast<char *>(out.data) + ((long long)(y - out.fy0) * out.pitch + (x - out.fx0)) * (HALF ? 8 : 16);
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

template <int HALF, int BILINEAR, int PAIR>
__global__ __launch_bounds__(kThreads) void k_transform(cvk_transform_params tp) {
    const int shift = __builtin_ctz((unsigned)tp.tw);
    const int lx = (int)threadIdx.x & (tp.tw - 1), ly = (int)threadIdx.x >> shift;
    const int x = tp.w.x0 + ((int)blockIdx.x << shift) + lx, y = tp.w.y0 + (int)blockIdx.y * tp.th + ly;
    if (x > tp.w.x1 || y > tp.w.y1) return;
    const float fx = (float)x, fy = (float)y;
    const float u = (tp.m[0] * fx + tp.m[1] * fy) + tp.m[2], v = (tp.m[3] * fx + tp.m[4] * fy) + tp.m[5];
    const float sx0 = (float)tp.s.x0, sx1 = (float)tp.s.x1, sy0 = (float)tp.s.y0, sy1 = (float)tp.s.y1;
    const v4 zero = { 0u, 0u, 0u, 0u };

    if (!BILINEAR) {
        const float fi = floorf(u + 0.5f), fj = floorf(v + 0.5f);
        const bool inside = fi >= sx0 && fi <= sx1 && fj >= sy0 && fj <= sy1;
        const Px p = load<HALF>(tp.in, (int)clampf(fi, sx0, sx1), (int)clampf(fj, sy0, sy1));
        store<HALF>(tp.out, x, y, inside ? p.raw : zero);
        return;
    }

    const float fi = floorf(u), fj = floorf(v), fi1 = fi + 1.0f, fj1 = fj + 1.0f;
    const float a = u - fi, b = v - fj, wa = 1.0f - a, wb = 1.0f - b;
    const bool x0in = fi >= sx0 && fi <= sx1, x1in = fi1 >= sx0 && fi1 <= sx1;
    const bool y0in = fj >= sy0 && fj <= sy1, y1in = fj1 >= sy0 && fj1 <= sy1;
    const int j0 = (int)clampf(fj, sy0, sy1), j1 = (int)clampf(fj1, sy0, sy1);
    Px p00, p10, p01, p11;
    if (HALF && PAIR) {
        // S is at least two columns wide (the launcher's condition): the pair (ip, ip + 1) lies inside S, and holds both taps
        // in order when the left tap is its first pixel; otherwise one tap is outside S and the other is the pair's far pixel
        const float fip = clampf(fi, sx0, sx1 - 1.0f);
        const int ip = (int)fip;
        const bool ordered = fi == fip;
        const v4 r0 = *reinterpret_cast<const v4_align8 *>(address<1>(tp.in, ip, j0));
        const v4 r1 = *reinterpret_cast<const v4_align8 *>(address<1>(tp.in, ip, j1));
        p00 = ordered ? from_half(r0.x, r0.y) : from_half(r0.z, r0.w);
        p10 = ordered ? from_half(r0.z, r0.w) : from_half(r0.x, r0.y);
        p01 = ordered ? from_half(r1.x, r1.y) : from_half(r1.z, r1.w);
        p11 = ordered ? from_half(r1.z, r1.w) : from_half(r1.x, r1.y);
    } else {
        const int i0 = (int)clampf(fi, sx0, sx1), i1 = (int)clampf(fi1, sx0, sx1);
        p00 = load<HALF>(tp.in, i0, j0);
        p10 = load<HALF>(tp.in, i1, j0);
        p01 = load<HALF>(tp.in, i0, j1);
        p11 = load<HALF>(tp.in, i1, j1);
    }
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
    store<HALF>(tp.out, x, y, o);
}

template <int HALF, int BILINEAR, int PAIR>
int launch(const cvk_transform_params &tp, hipStream_t st) {
    const long long cols = (long long)tp.w.x1 - tp.w.x0 + 1, rows = (long long)tp.w.y1 - tp.w.y0 + 1;
    const long long tiles = (rows + tp.th - 1) / tp.th;
    // a window of any height: bands of at most kMaxGridY rows of tiles, one launch each (a tile depends on nothing but its
    // own coordinates, so a band is the same kernel on a window that starts further down)
    for (long long first = 0; first < tiles; first += kMaxGridY) {
        const long long n = tiles - first < kMaxGridY ? tiles - first : kMaxGridY;
        cvk_transform_params band = tp;
        band.w.y0 = (int)(tp.w.y0 + first * tp.th);
        const long long last = (long long)band.w.y0 + n * tp.th - 1;
        band.w.y1 = last < tp.w.y1 ? (int)last : tp.w.y1;
        const dim3 grid((unsigned)((cols + tp.tw - 1) / tp.tw), (unsigned)n, 1);
        hipLaunchKernelGGL((k_transform<HALF, BILINEAR, PAIR>), grid, dim3(kThreads), 0, st, band);
        const int rc = (int)hipGetLastError();
        if (rc != 0) return rc;
    }
    return 0;
}

}  // namespace

extern "C" int cvk_transform(const cvk_transform_params *in, int half, void *stream) {
    const cvk_transform_params &tp = *in;
    if (rect_empty(tp.w)) return 0;
    if (rect_empty(tp.s) || tp.tw < 8 || tp.tw > kThreads || (tp.tw & (tp.tw - 1)) || tp.tw * tp.th != kThreads) return (int)hipErrorInvalidValue;
    // the window written inside the target's buffer, the source window inside the source's: nothing else is ever addressed
    if (tp.w.x0 < tp.out.fx0 || tp.w.y0 < tp.out.fy0 || tp.w.x1 > tp.out.fx1 || tp.w.y1 > tp.out.fy1) return (int)hipErrorInvalidValue;
    if (tp.s.x0 < tp.in.fx0 || tp.s.y0 < tp.in.fy0 || tp.s.x1 > tp.in.fx1 || tp.s.y1 > tp.in.fy1) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    if (!tp.bilinear) return half ? launch<1, 0, 0>(tp, st) : launch<0, 0, 0>(tp, st);
    if (!half) return launch<0, 1, 0>(tp, st);
#ifdef CVS_DIAG
    if (tp.pair_loads && tp.s.x1 > tp.s.x0) return launch<1, 1, 1>(tp, st);                // a one-column S has no pair
#endif
    return launch<1, 1, 0>(tp, st);
}
