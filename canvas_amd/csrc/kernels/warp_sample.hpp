// warp_sample.hpp -- what the warp kernels (transform_ops.hip, perspective_ops.hip, warp_cubic_ops.hip) share from the source
// coordinates (u, v) on: the nearest, the alpha-weighted bilinear and the alpha-weighted Catmull-Rom filter of un-premultiplied
// RGBA, and the launches of a window of any height.
//
// The arithmetic contract, stated here once.  S = the source window in the coordinate system of u and v (every bound within
// +-2^23, which the callers' hosts see to, so the bounds are exact floats).  In f32 (a half widened exactly), every operation
// rounded on its own in BOTH arithmetic flavours (the units are built once: not in FMA_KERN):
//     in(i, j) = S.x0 <= i <= S.x1 and S.y0 <= j <= S.y1, compared as floats: false for NaN and +-Inf
//     nearest:   i = floorf(u + 0.5f), j = floorf(v + 0.5f);  out = in(i, j) ? source(i, j) code for code : 0
//     bilinear:  i = floorf(u), j = floorf(v);  a = u - i;  b = v - j;  wa = 1 - a;  wb = 1 - b
//                a == 0 and b == 0:  out = in(i, j) ? source(i, j) code for code : 0
//                else A = R = G = B = 0;  for (w, di, dj) in (wa*wb, 0, 0), (a*wb, 1, 0), (wa*b, 0, 1), (a*b, 1, 1):
//                         if in(i + di, j + dj):  p = source(i + di, j + dj);  q = w * p.a;  A += q;  R += q*p.r;  G += q*p.g;  B += q*p.b
//                     out = A != 0 ? (R / A, G / A, B / A, A) : 0                       f16 truncated once at the store
// A tap coordinate is turned into an integer only after it has been clamped into S as a float: NaN, +-Inf and values no int
// holds never reach a conversion, and no address is ever formed outside S, whatever the coefficients hold.  A tap outside S
// loads the clamped address and a select drops what it would have added, so the four taps do not diverge at the layer's edge.
//
//
// The Catmull-Rom filter (the cubic that interpolates: on a sample it returns the sample), S, in() and the clamp before any
// conversion as above, in f32, every product and every sum rounded on its own in both flavours:
//     i = floorf(u), j = floorf(v);  a = u - i;  b = v - j
//     weights of a fraction t (wx[0..3] from a, wy[0..3] from b), Horner, in this order:
//         w0 = ((-0.5f*t + 1.0f)*t - 0.5f)*t        w1 = ((1.5f*t - 2.5f)*t)*t + 1.0f
//         w2 = ((-1.5f*t + 2.0f)*t + 0.5f)*t        w3 = ((0.5f*t - 0.5f)*t)*t
//     a == 0 and b == 0:  out = in(i, j) ? source(i, j) code for code : 0                        the copy rule, as bilinear
//     else  A = R = G = B = 0;  lo_c = +inf, hi_c = -inf per colour channel;  lo_a = +inf, hi_a = -inf
//           for l in 0..3 (rows j-1+l), for k in 0..3 (columns i-1+k), in this order (the coordinates are the floats
//           i + (float)(k-1), j + (float)(l-1)):
//               p = source(i-1+k, j-1+l) if in(...);  counts = in(...) and p.a > 0               false for a NaN alpha
//               if counts:  q = (wx[k]*wy[l]) * p.a;  A += q;  R += q*p.r;  G += q*p.g;  B += q*p.b
//                           lo_c = fmin(lo_c, p.c);  hi_c = fmax(hi_c, p.c)                      per colour channel
//               ta = counts ? p.a : 0;  lo_a = fmin(lo_a, ta);  hi_a = fmax(hi_a, ta)            all 16 positions
//           out = A > 0 ? (clamp(R/A, lo_r, hi_r), clamp(G/A, ..), clamp(B/A, ..), clamp(A, lo_a, hi_a)) : 0
//           clamp(t, lo, hi) = fmin(fmax(t, lo), hi);  fmin / fmax: a NaN operand loses;  IEEE divides
// The clamp rule: the result never leaves the range of the 4 x 4 samples it was made from.  Each colour channel stays between the
// least and the greatest value of that channel among the taps that count; alpha between the least and greatest alpha of the
// sixteen positions, one outside S or with an alpha not above 0 counting as 0.  A tap that does not count adds nothing to any
// sum, so A > 0 implies a counting tap and the colour limits are never the initial infinities.  No negative light out of
// non-negative light, no alpha above the layer's own, no blow-up of the colour where A collapses under mixed-sign weights; the
// interior of an opaque layer stays exactly opaque and a flat colour exactly flat (the limits coincide).  What a NaN colour
// under a positive alpha gives is what the arithmetic above gives; NaN payloads are not pinned, nor is the sign of a zero that
// a minimum or maximum returns.
//
// A kernel computes u and v its own way and says where source(i, j) and the target pixel lie (`at`: (i, j) inside S -> address).
#pragma once
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "pixel_math.hpp"
#include "stream_common.hpp"

namespace warp {

using rowstream::v2;
using rowstream::v4;

constexpr int kThreads = 256;

struct Px { v4 raw; cvs::px32 f; };                             // raw: the pixel's own dwords (two of them for a half pixel)

__device__ __forceinline__ Px from_half(uint32_t lo, uint32_t hi) { return Px{ v4{ lo, hi, 0u, 0u }, cvs::widen(make_uint2(lo, hi)) }; }

template <int HALF>
__device__ __forceinline__ Px load(const char *p) {
    if (HALF) {
        const v2 t = *reinterpret_cast<const v2 *>(p);
        return from_half(t.x, t.y);
    }
    const v4 t = *reinterpret_cast<const v4 *>(p);
    return Px{ t, cvs::px32{ __uint_as_float(t.x), __uint_as_float(t.y), __uint_as_float(t.z), __uint_as_float(t.w) } };
}

template <int HALF>
__device__ __forceinline__ void store(char *p, v4 raw) {
    if (HALF) __builtin_nontemporal_store(v2{ raw.x, raw.y }, reinterpret_cast<v2 *>(p));
    else __builtin_nontemporal_store(raw, reinterpret_cast<v4 *>(p));
}

__device__ __forceinline__ float clampf(float t, float lo, float hi) { return fminf(fmaxf(t, lo), hi); }   // a NaN comes out as lo

// S as floats, with in() and the clamp-then-convert of one axis
struct Window {
    float x0, x1, y0, y1;
    __device__ __forceinline__ explicit Window(const cvk_rect &s) : x0((float)s.x0), x1((float)s.x1), y0((float)s.y0), y1((float)s.y1) {}
    __device__ __forceinline__ bool xin(float fi) const { return fi >= x0 && fi <= x1; }
    __device__ __forceinline__ bool yin(float fj) const { return fj >= y0 && fj <= y1; }
    __device__ __forceinline__ int col(float fi) const { return (int)clampf(fi, x0, x1); }
    __device__ __forceinline__ int row(float fj) const { return (int)clampf(fj, y0, y1); }
};

template <int HALF, class At>
__device__ __forceinline__ v4 nearest(float u, float v, const Window &s, At at) {
    const float fi = floorf(u + 0.5f), fj = floorf(v + 0.5f);
    const bool inside = s.xin(fi) && s.yin(fj);
    const Px p = load<HALF>(at(s.col(fi), s.row(fj)));
    return inside ? p.raw : v4{ 0u, 0u, 0u, 0u };
}

// the four taps of (u, v): the left and upper tap's coordinates, the weights, and which columns and rows lie in S
struct Taps {
    float fi, fj, a, b;
    bool x0in, x1in, y0in, y1in;
    __device__ __forceinline__ Taps(float u, float v, const Window &s) : fi(floorf(u)), fj(floorf(v)), a(u - fi), b(v - fj),
        x0in(s.xin(fi)), x1in(s.xin(fi + 1.0f)), y0in(s.yin(fj)), y1in(s.yin(fj + 1.0f)) {}
};

struct Sum { float a, r, g, b; };
__device__ __forceinline__ void tap(Sum &s, float w, const cvs::px32 &p, bool inside) {
    const float q = w * p.a;
    const float a = s.a + q, r = s.r + q * p.r, g = s.g + q * p.g, b = s.b + q * p.b;
    s.a = inside ? a : s.a; s.r = inside ? r : s.r; s.g = inside ? g : s.g; s.b = inside ? b : s.b;
}

// the pixel of the four taps, however they were loaded (a tap outside S may hold anything)
template <int HALF>
__device__ __forceinline__ v4 blend(const Taps &t, const Px &p00, const Px &p10, const Px &p01, const Px &p11) {
    const float wa = 1.0f - t.a, wb = 1.0f - t.b;
    const v4 zero = { 0u, 0u, 0u, 0u };
    Sum s = { 0.0f, 0.0f, 0.0f, 0.0f };
    tap(s, wa * wb, p00.f, t.x0in && t.y0in);
    tap(s, t.a * wb, p10.f, t.x1in && t.y0in);
    tap(s, wa * t.b, p01.f, t.x0in && t.y1in);
    tap(s, t.a * t.b, p11.f, t.x1in && t.y1in);
    v4 o = zero;
    if (s.a != 0.0f) {
        const cvs::px32 c = { s.r / s.a, s.g / s.a, s.b / s.a, s.a };
        if (HALF) { const uint2 n = cvs::narrow(c); o = v4{ n.x, n.y, 0u, 0u }; }
        else o = v4{ __float_as_uint(c.r), __float_as_uint(c.g), __float_as_uint(c.b), __float_as_uint(c.a) };
    }
    if (t.a == 0.0f && t.b == 0.0f) o = (t.x0in && t.y0in) ? p00.raw : zero;   // on a sample: a copy
    return o;
}

template <int HALF, class At>
__device__ __forceinline__ v4 bilinear(float u, float v, const Window &s, At at) {
    const Taps t(u, v, s);
    const int i0 = s.col(t.fi), i1 = s.col(t.fi + 1.0f), j0 = s.row(t.fj), j1 = s.row(t.fj + 1.0f);
    const Px p00 = load<HALF>(at(i0, j0));
    const Px p10 = load<HALF>(at(i1, j0));
    const Px p01 = load<HALF>(at(i0, j1));
    const Px p11 = load<HALF>(at(i1, j1));
    return blend<HALF>(t, p00, p10, p01, p11);
}

// ---------------------------------------------------------------- Catmull-Rom (the contract: the head of this file)

// the four weights of a fraction t, Horner, every product and sum rounded on its own
__device__ __forceinline__ void cubic_weights(float t, float (&w)[4]) {
    w[0] = ((-0.5f * t + 1.0f) * t - 0.5f) * t;
    w[1] = ((1.5f * t - 2.5f) * t) * t + 1.0f;
    w[2] = ((-1.5f * t + 2.0f) * t + 0.5f) * t;
    w[3] = ((0.5f * t - 0.5f) * t) * t;
}

// lo and hi widened by the four values of a tap row; a NaN among them loses, which is how a tap that does not count stays out.
// (Minima and maxima in any grouping: the same value, the sign of a zero apart.  Written so that each folds into two three-operand
// instructions.)
struct Range { float lo, hi; };
__device__ __forceinline__ void widen_range(Range &r, const float (&t)[4]) {
    r.lo = fminf(fminf(fminf(t[0], t[1]), t[2]), fminf(fminf(t[3], r.lo), r.lo));
    r.hi = fmaxf(fmaxf(fmaxf(t[0], t[1]), t[2]), fmaxf(fmaxf(t[3], r.hi), r.hi));
}

// The source reads the sixteen taps row by row; taps(col, j, p): the four pixels of row j at the columns col[0..3], every one of
// them inside S, however it loads them.  (hipcc hoists all sixteen loads above the arithmetic all the same: DESIGN.md
// "Catmull-Rom warps" has the registers.)
// A tap that does not count is kept out by selects on what goes IN, not on the sums and limits that come out: its alpha becomes 0
// and its colour 0 for the sums -- q is then +-0 and so is every product (the weights of a finite fraction are finite), and a sum
// that began at +0 is never -0, so adding +-0 leaves its bits -- and its colour becomes NaN for the limits, where a NaN loses.
// With u or v not finite the weights are NaN, every tap is outside S, A becomes NaN and A > 0 is false: 0, as the contract says.
template <int HALF, class Row>
__device__ __forceinline__ v4 cubic_rows(float u, float v, const Window &s, Row taps) {
    const float fi = floorf(u), fj = floorf(v), a = u - fi, b = v - fj;
    float wx[4], wy[4];
    cubic_weights(a, wx);
    cubic_weights(b, wy);
    bool xin[4];
    int col[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const float fk = fi + (float)(k - 1);
        xin[k] = s.xin(fk);
        col[k] = s.col(fk);
    }
    const float inf = __builtin_inff(), nan = __builtin_nanf("");
    const v4 zero = { 0u, 0u, 0u, 0u };
    Sum sum = { 0.0f, 0.0f, 0.0f, 0.0f };
    Range rr = { inf, -inf }, rg = { inf, -inf }, rb = { inf, -inf }, ra = { inf, -inf };
    v4 centre = zero;                                           // source(i, j), for the copy rule
#pragma unroll
    for (int l = 0; l < 4; l++) {
        const float fl = fj + (float)(l - 1);
        const bool yin = s.yin(fl);
        const int row = s.row(fl);
        Px p[4];
        taps(col, row, p);
        if (l == 1) centre = p[1].raw;
        float ta[4], tr[4], tg[4], tb[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const cvs::px32 &f = p[k].f;
            const bool counts = xin[k] && yin && f.a > 0.0f;    // false for a NaN alpha
            ta[k] = counts ? f.a : 0.0f;
            const float q = (wx[k] * wy[l]) * ta[k];
            sum.a = sum.a + q;
            sum.r = sum.r + q * (counts ? f.r : 0.0f);
            sum.g = sum.g + q * (counts ? f.g : 0.0f);
            sum.b = sum.b + q * (counts ? f.b : 0.0f);
            tr[k] = counts ? f.r : nan;
            tg[k] = counts ? f.g : nan;
            tb[k] = counts ? f.b : nan;
        }
        widen_range(rr, tr);
        widen_range(rg, tg);
        widen_range(rb, tb);
        widen_range(ra, ta);
    }
    v4 o = zero;
    if (sum.a > 0.0f) {
        const cvs::px32 c = { clampf(sum.r / sum.a, rr.lo, rr.hi), clampf(sum.g / sum.a, rg.lo, rg.hi), clampf(sum.b / sum.a, rb.lo, rb.hi),
                              clampf(sum.a, ra.lo, ra.hi) };
        if (HALF) { const uint2 n = cvs::narrow(c); o = v4{ n.x, n.y, 0u, 0u }; }
        else o = v4{ __float_as_uint(c.r), __float_as_uint(c.g), __float_as_uint(c.b), __float_as_uint(c.a) };
    }
    if (a == 0.0f && b == 0.0f) o = (xin[1] && s.yin(fj)) ? centre : zero;    // on a sample: a copy
    return o;
}

// one load per tap: 8 bytes of a half pixel, 16 of an f32 one
template <int HALF, class At>
__device__ __forceinline__ v4 cubic(float u, float v, const Window &s, At at) {
    return cubic_rows<HALF>(u, v, s, [&](const int (&col)[4], int j, Px (&p)[4]) {
#pragma unroll
        for (int k = 0; k < 4; k++) p[k] = load<HALF>(at(col[k], j));
    });
}

template <int HALF, int BILINEAR, class At>
__device__ __forceinline__ v4 sample(float u, float v, const Window &s, At at) {
    return BILINEAR ? bilinear<HALF>(u, v, s, at) : nearest<HALF>(u, v, s, at);
}

// A window `w` of any height in tiles of tw x th target pixels (tw * th == kThreads): bands of at most kMaxGridY rows of tiles,
// one launch each (a tile depends on nothing but its own coordinates, so a band is the same kernel on a window that starts
// further down).  0, or the HIP error
template <class Params>
int launch_bands(void (*kernel)(Params), const Params &p, int tw, int th, hipStream_t st) {
    const long long cols = (long long)p.w.x1 - p.w.x0 + 1, rows = (long long)p.w.y1 - p.w.y0 + 1;
    const long long tiles = (rows + th - 1) / th;
    for (long long first = 0; first < tiles; first += rowstream::kMaxGridY) {
        const long long n = tiles - first < rowstream::kMaxGridY ? tiles - first : rowstream::kMaxGridY;
        Params band = p;
        band.w.y0 = (int)(p.w.y0 + first * th);
        const long long last = (long long)band.w.y0 + n * th - 1;
        band.w.y1 = last < p.w.y1 ? (int)last : p.w.y1;
        const dim3 grid((unsigned)((cols + tw - 1) / tw), (unsigned)n, 1);
        hipLaunchKernelGGL(kernel, grid, dim3(kThreads), 0, st, band);
        const int rc = (int)hipGetLastError();
        if (rc != 0) return rc;
    }
    return 0;
}

}  // namespace warp
