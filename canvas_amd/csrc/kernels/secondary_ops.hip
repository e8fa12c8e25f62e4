// secondary_ops.hip -- secondaries on un-premultiplied RGBA device frames: a qualifier that makes a matte from a pixel's hue,
// saturation and luma (VideoQualifierFilter), and a mix of two frames through a matte held in a third (VideoMatteMixFilter).
//
// No reference code.  The contract is DESIGN.md "Secondaries" and include/canvas_secondary.h, restated here.  All of it is in f32
// (a half widened exactly).  sel(t) = (t > 0) ? ((t < 1) ? t : 1) : 0, so NaN gives 0: a pixel that cannot be measured is not
// selected (the key's ramp keeps it).  The host (host/secondary.c) hands over, formed once per call in f32:
//     hc = fmodf(center, 360) / 60, plus 6 if negative ;  hw = width / 120 ;  hs = softness / 60 ;  h_edge = hw + hs ;
//     inv_hs = 1 / hs where hs > 0 ;  per value range lo_edge = low - soft_low, hi_edge = high + soft_high and the two
//     reciprocals, each where its softness is > 0.
// Qualifier, per pixel (r, g, b) of the key frame (the source itself where no key frame is given) and pixel s of the source:
//     any of r, g, b NaN -> m = 0                                        an explicit test, nothing rests on max / min of a NaN
//     mx = max(r, g, b) ; mn = min(r, g, b) ; c = mx - mn
//     y  = (r*0.2126f + g*0.7152f) + b*0.0722f                           the key kernel's luma
//     s  = mx > 0 ? c / mx : 0                                           HSV saturation
//     hue in sextants, only where c > 0:
//         r == mx (tested first): h = (g - b) / c ; if h < 0: h = h + 6
//         else g == mx:           h = (b - r) / c + 2
//         else:                   h = (r - g) / c + 4
//         d = |h - hc| ; e = 6 - d ; d = e < d ? e : d
//     m_h = !(c > 0) ? 0 : hs > 0 ? sel((h_edge - d) * inv_hs) : (d <= hw ? 1 : 0)
//     range(v) = min(soft_low > 0 ? sel((v - lo_edge) * inv_soft_low) : (v >= low ? 1 : 0),
//                    soft_high > 0 ? sel((hi_edge - v) * inv_soft_high) : (v <= high ? 1 : 0))
//     m = (m_h * range_sat(s)) * range_luma(y)                           an axis that does not qualify contributes exactly 1
//     invert: m = 1 - m
//     a' = s.a * m
//     out = matte view ? (a', a', a', 1) : (s.r, s.g, s.b, a')           colour code for code
// Mix through a matte, per pixel of a, b and the matte M:
//     v = luma ? (M.r*0.2126f + M.g*0.7152f) + M.b*0.0722f : M.a ;  k = sel(v) ;  invert: k = 1 - k
//     k == 0: out = a's four codes ;  k == 1: out = b's four codes       selected, not computed
//     else for c in r, g, b, a:  e = b.c - a.c ; f = k * e ; out.c = a.c + f
// Every operation is rounded on its own in BOTH arithmetic flavours (the stance of key_ops.hip: no reference code exists for
// these expressions), so there is one build of the unit: it is not in FMA_KERN.  The divides are IEEE, correctly rounded (the
// plain `/` of temporal_ops.hip and perspective_ops.hip; no rcp).  f16 targets are truncated once, at the store.
//
// Bound: HBM.  Pure streams: no table, no LDS, no scratch, no cross-lane traffic.  Algorithmic bytes per pixel on f16 frames:
// qualifier 8 read + 8 written, 16 + 8 with a key frame; mix 24 read + 8 written (twice that on f32).  Shape: key_ops.hip's
// (stream_common.hpp) -- a one-wave workgroup owns 64 lanes x PIX columns over a segment of consecutive rows, one 16-byte access
// per lane, row and input: an f32 pixel, or two half pixels where base, pitch and window parity of ALL frames of the call allow
// (pair_view), else one half pixel in 8 bytes.  The next row's loads, of every input, are issued before the current row is
// worked out.  Stores are non-temporal.  In place on any input needs nothing special: a lane reads the pixels it writes, each
// before it writes it, and no other lane touches them; inputs that share a buffer are only read.
// Instances: the pixel form x key frame or not x hue alone or any axes x matte view (24), and the pixel form x alpha or luma (6).
// An absent axis multiplies by exactly 1, so the instance that takes any axes is right for every set: hue alone is a matter of
// speed (no saturation divide, no luma).
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "pixel_math.hpp"
#include "stream_common.hpp"

namespace {

using namespace rowstream;

constexpr float c00 = 0.2126f, c01 = 0.7152f, c02 = 0.0722f;

__device__ __forceinline__ float sel(float t) { return (t > 0.0f) ? ((t < 1.0f) ? t : 1.0f) : 0.0f; }

__device__ __forceinline__ float luma_of(float r, float g, float b) { return (r * c00 + g * c01) + b * c02; }

__device__ __forceinline__ float range_of(const cvk_value_range &vr, float v) {       // soft_lo, soft_hi: wave-uniform
    const float lo = vr.soft_lo ? sel((v - vr.lo_edge) * vr.inv_lo) : (v >= vr.low ? 1.0f : 0.0f);
    const float hi = vr.soft_hi ? sel((vr.hi_edge - v) * vr.inv_hi) : (v <= vr.high ? 1.0f : 0.0f);
    return hi < lo ? hi : lo;
}

// the factor on the source's alpha that the key pixel (r, g, b) earns.  ANY: saturation and luma may qualify, and hue may not
template <bool ANY>
__device__ __forceinline__ float qualify_of(const cvk_qualify_params &qp, float r, float g, float b) {
    float m = 0.0f;
    if (!(r != r || g != g || b != b)) {
        float mx = r > g ? r : g, mn = r < g ? r : g;
        mx = b > mx ? b : mx;
        mn = b < mn ? b : mn;
        const float c = mx - mn;
        float mh = 1.0f;
        if (!ANY || qp.hue) {                                           // wave-uniform
            mh = 0.0f;
            if (c > 0.0f) {
                const bool rmax = r == mx, gmax = g == mx;
                const float num = rmax ? g - b : (gmax ? b - r : r - g);
                float h = num / c;
                if (rmax) h = h < 0.0f ? h + 6.0f : h;
                else h = h + (gmax ? 2.0f : 4.0f);
                float d = fabsf(h - qp.hc);
                const float e = 6.0f - d;
                d = e < d ? e : d;
                mh = qp.hue_soft ? sel((qp.h_edge - d) * qp.inv_hs) : (d <= qp.hw ? 1.0f : 0.0f);
            }
        }
        m = mh;
        if (ANY) {
            float rs = 1.0f, ry = 1.0f;
            if (qp.saturation) rs = range_of(qp.sat, mx > 0.0f ? c / mx : 0.0f);
            if (qp.lum) ry = range_of(qp.luma, luma_of(r, g, b));
            m = (mh * rs) * ry;
        }
    }
    return qp.invert ? 1.0f - m : m;
}

// one f32 pixel as its four dwords: s the source's, k the key frame's
template <bool ANY, bool MATTE>
__device__ __forceinline__ v4 qualify_f32(const cvk_qualify_params &qp, v4 s, v4 k) {
    const float m = qualify_of<ANY>(qp, __uint_as_float(k.x), __uint_as_float(k.y), __uint_as_float(k.z));
    const uint32_t a1 = __float_as_uint(__uint_as_float(s.w) * m);
    if (MATTE) return v4{ a1, a1, a1, 0x3F800000u };
    return v4{ s.x, s.y, s.z, a1 };
}

// one half pixel as its two dwords (lo = g:r, hi = a:b)
template <bool ANY, bool MATTE>
__device__ __forceinline__ v2 qualify_f16(const cvk_qualify_params &qp, uint32_t slo, uint32_t shi, uint32_t klo, uint32_t khi) {
    const float m = qualify_of<ANY>(qp, cvs::h2f(klo & 0xFFFFu), cvs::h2f(klo >> 16), cvs::h2f(khi & 0xFFFFu));
    const float a1 = cvs::h2f(shi >> 16) * m;
    if (MATTE) return v2{ cvs::f2h_rz2(a1, a1), cvs::f2h_rz2(a1, 1.0f) };
    return v2{ slo, (shi & 0xFFFFu) | (cvs::f2h_rz(a1) << 16) };
}

__device__ __forceinline__ float mix_weight(bool luma, bool invert, float r, float g, float b, float a) {
    const float k = sel(luma ? luma_of(r, g, b) : a);
    return invert ? 1.0f - k : k;
}

__device__ __forceinline__ float mix_of(float a, float b, float k) {
    const float e = b - a, f = k * e;
    return a + f;
}

template <bool LUMA>
__device__ __forceinline__ v4 mix_f32(bool invert, v4 a, v4 b, v4 m) {
    const float k = mix_weight(LUMA, invert, __uint_as_float(m.x), __uint_as_float(m.y), __uint_as_float(m.z), __uint_as_float(m.w));
    if (k == 0.0f) return a;
    if (k == 1.0f) return b;
    return v4{ __float_as_uint(mix_of(__uint_as_float(a.x), __uint_as_float(b.x), k)), __float_as_uint(mix_of(__uint_as_float(a.y), __uint_as_float(b.y), k)),
               __float_as_uint(mix_of(__uint_as_float(a.z), __uint_as_float(b.z), k)), __float_as_uint(mix_of(__uint_as_float(a.w), __uint_as_float(b.w), k)) };
}

template <bool LUMA>
__device__ __forceinline__ v2 mix_f16(bool invert, uint32_t alo, uint32_t ahi, uint32_t blo, uint32_t bhi, uint32_t mlo, uint32_t mhi) {
    const float k = mix_weight(LUMA, invert, cvs::h2f(mlo & 0xFFFFu), cvs::h2f(mlo >> 16), cvs::h2f(mhi & 0xFFFFu), cvs::h2f(mhi >> 16));
    if (k == 0.0f) return v2{ alo, ahi };
    if (k == 1.0f) return v2{ blo, bhi };
    return v2{ cvs::f2h_rz2(mix_of(cvs::h2f(alo & 0xFFFFu), cvs::h2f(blo & 0xFFFFu), k), mix_of(cvs::h2f(alo >> 16), cvs::h2f(blo >> 16), k)),
               cvs::f2h_rz2(mix_of(cvs::h2f(ahi & 0xFFFFu), cvs::h2f(bhi & 0xFFFFu), k), mix_of(cvs::h2f(ahi >> 16), cvs::h2f(bhi >> 16), k)) };
}

// HALF: 0 = rgba_f32 frames, one pixel per lane; 1 = rgba_f16, one pixel per lane; 2 = rgba_f16, two pixels per lane
template <int HALF>
__device__ __forceinline__ v4 load_row(const cvk_view &v, int x, int y) {
    if (HALF) return load_px<HALF>(v, x, y);
    return *reinterpret_cast<const v4 *>(static_cast<const char *>(v.data) + ((long long)(y - v.fy0) * v.pitch + (x - v.fx0)) * 16);
}

template <int HALF>
__device__ __forceinline__ void store_row(const cvk_view &v, int x, int y, v4 c, bool m0, bool m1) {
    if (HALF) { store_px<(HALF == 2 ? 2 : 1)>(v, x, y, c, m0, m1); return; }
    char *p = static_cast<char *>(v.data) + ((long long)(y - v.fy0) * v.pitch + (x - v.fx0)) * 16;
    __builtin_nontemporal_store(c, reinterpret_cast<v4 *>(p));
}

template <int HALF, bool KEY, bool ANY, bool MATTE>
__global__ __launch_bounds__(kLanes) void k_qualify(cvk_qualify_params qp, cvk_view out, cvk_view in, cvk_view key, cvk_rect w, int xs, int seg) {
    constexpr int PIX = HALF == 2 ? 2 : 1;
    ROWSTREAM_LANE(w, xs, seg)
    v4 cur = load_row<HALF>(in, x, y0), kcur = cur;
    if (KEY) kcur = load_row<HALF>(key, x, y0);
    for (int y = y0; y <= y1; y++) {
        v4 next = cur, knext = kcur;
        if (y < y1) {                                                   // wave-uniform
            next = load_row<HALF>(in, x, y + 1);
            if (KEY) knext = load_row<HALF>(key, x, y + 1);
        }
        if (!KEY) kcur = cur;
        v4 c;
        if (HALF) {
            const v2 p0 = qualify_f16<ANY, MATTE>(qp, cur.x, cur.y, kcur.x, kcur.y);
            c = v4{ p0.x, p0.y, 0u, 0u };
            if (PIX == 2) { const v2 p1 = qualify_f16<ANY, MATTE>(qp, cur.z, cur.w, kcur.z, kcur.w); c.z = p1.x; c.w = p1.y; }
        } else {
            c = qualify_f32<ANY, MATTE>(qp, cur, kcur);
        }
        store_row<HALF>(out, x, y, c, m0, m1);
        cur = next;
        kcur = knext;
    }
}

template <int HALF, bool LUMA>
__global__ __launch_bounds__(kLanes) void k_matte_mix(cvk_view out, cvk_view a, cvk_view b, cvk_view matte, cvk_rect w, int invert, int xs, int seg) {
    constexpr int PIX = HALF == 2 ? 2 : 1;
    ROWSTREAM_LANE(w, xs, seg)
    const bool inv = invert != 0;
    v4 ca = load_row<HALF>(a, x, y0), cb = load_row<HALF>(b, x, y0), cm = load_row<HALF>(matte, x, y0);
    for (int y = y0; y <= y1; y++) {
        v4 na = ca, nb = cb, nm = cm;
        if (y < y1) {                                                   // wave-uniform
            na = load_row<HALF>(a, x, y + 1);
            nb = load_row<HALF>(b, x, y + 1);
            nm = load_row<HALF>(matte, x, y + 1);
        }
        v4 c;
        if (HALF) {
            const v2 p0 = mix_f16<LUMA>(inv, ca.x, ca.y, cb.x, cb.y, cm.x, cm.y);
            c = v4{ p0.x, p0.y, 0u, 0u };
            if (PIX == 2) { const v2 p1 = mix_f16<LUMA>(inv, ca.z, ca.w, cb.z, cb.w, cm.z, cm.w); c.z = p1.x; c.w = p1.y; }
        } else {
            c = mix_f32<LUMA>(inv, ca, cb, cm);
        }
        store_row<HALF>(out, x, y, c, m0, m1);
        ca = na;
        cb = nb;
        cm = nm;
    }
}

template <int HALF, bool KEY, bool ANY>
int launch_qualify2(const cvk_qualify_params &qp, const cvk_view &out, const cvk_view &in, const cvk_view &key, const cvk_rect &w, const Shape &s, hipStream_t st) {
    if (qp.matte) hipLaunchKernelGGL((k_qualify<HALF, KEY, ANY, true>), s.grid, dim3(kLanes), 0, st, qp, out, in, key, w, s.xs, s.seg);
    else hipLaunchKernelGGL((k_qualify<HALF, KEY, ANY, false>), s.grid, dim3(kLanes), 0, st, qp, out, in, key, w, s.xs, s.seg);
    return (int)hipGetLastError();
}

template <int HALF>
int launch_qualify(const cvk_qualify_params &qp, const cvk_view &out, const cvk_view &in, const cvk_view *key, const cvk_rect &w, const Shape &s, hipStream_t st) {
    const bool hue_alone = qp.hue && !qp.saturation && !qp.lum;
    if (key) return hue_alone ? launch_qualify2<HALF, true, false>(qp, out, in, *key, w, s, st) : launch_qualify2<HALF, true, true>(qp, out, in, *key, w, s, st);
    return hue_alone ? launch_qualify2<HALF, false, false>(qp, out, in, in, w, s, st) : launch_qualify2<HALF, false, true>(qp, out, in, in, w, s, st);
}

template <int HALF>
int launch_mix(const cvk_view &out, const cvk_view &a, const cvk_view &b, const cvk_view &m, const cvk_rect &w, int luma, int invert, const Shape &s, hipStream_t st) {
    if (luma) hipLaunchKernelGGL((k_matte_mix<HALF, true>), s.grid, dim3(kLanes), 0, st, out, a, b, m, w, invert, s.xs, s.seg);
    else hipLaunchKernelGGL((k_matte_mix<HALF, false>), s.grid, dim3(kLanes), 0, st, out, a, b, m, w, invert, s.xs, s.seg);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int cvk_qualify(const cvk_qualify_params *qp, cvk_view out, cvk_view src, const cvk_view *key, cvk_rect w, int half, int cus, void *stream) {
    if (rect_empty(w)) return 0;
    const int xs2 = w.x0 - (int)(((long long)w.x0 - out.fx0) & 1);
    const Shape s = shape(w, half && pair_view(out, xs2) && pair_view(src, xs2) && (!key || pair_view(*key, xs2)), out.fx0, cus);
    if (!half) return launch_qualify<0>(*qp, out, src, key, w, s, (hipStream_t)stream);
    return s.pix == 2 ? launch_qualify<2>(*qp, out, src, key, w, s, (hipStream_t)stream) : launch_qualify<1>(*qp, out, src, key, w, s, (hipStream_t)stream);
}

extern "C" int cvk_matte_mix(cvk_view out, cvk_view a, cvk_view b, cvk_view matte, cvk_rect w, int luma, int invert, int half, int cus, void *stream) {
    if (rect_empty(w)) return 0;
    const int xs2 = w.x0 - (int)(((long long)w.x0 - out.fx0) & 1);
    const Shape s = shape(w, half && pair_view(out, xs2) && pair_view(a, xs2) && pair_view(b, xs2) && pair_view(matte, xs2), out.fx0, cus);
    if (!half) return launch_mix<0>(out, a, b, matte, w, luma, invert, s, (hipStream_t)stream);
    return s.pix == 2 ? launch_mix<2>(out, a, b, matte, w, luma, invert, s, (hipStream_t)stream) : launch_mix<1>(out, a, b, matte, w, luma, invert, s, (hipStream_t)stream);
}
