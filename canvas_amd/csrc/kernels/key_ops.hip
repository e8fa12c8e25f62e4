// key_ops.hip -- VideoChromaKeyFilter: a chroma-distance keyer with spill suppression on un-premultiplied RGBA device frames.
//
// No reference code (its notes only name "Chromakey effects", docs/sphinx/feature-proposal/hints.rst:70).  The contract is
// DESIGN.md "Chroma key", restated here.  The host (host/key.c) hands over kpb, kpr (the key colour's Pb, Pr), tolerance,
// inv_soft = 1 / softness, inv_spill = 1 / spill_range (each used only where its width is > 0) and spill clamped to [0, 1].
// Per pixel s of the window, in f32 (a half widened exactly), with the A14 Rec.709 R'G'B' -> Y'PbPr rows c0, c1, c2 (dv_ops.hip):
//     pb = (s.r*c10 + s.g*c11) + s.b*c12 ;  pr = (s.r*c20 + s.g*c21) + s.b*c22
//     dx = pb - kpb ; dy = pr - kpr ; d = sqrtf(dx*dx + dy*dy)           correctly rounded IEEE square root
//     ramp(t) = (t < 1) ? ((t > 0) ? t : 0) : 1                            NaN -> 1: a pixel whose distance is NaN is kept
//     m  = softness > 0 ? ramp((d - tolerance) * inv_soft) : (d <= tolerance ? 0 : 1)
//     a' = s.a * m
//     spill > 0:  q  = spill_range > 0 ? ramp((d - tolerance) * inv_spill) : (d <= tolerance ? 0 : 1)
//                 ws = spill * (1 - q) ;  y = (s.r*c00 + s.g*c01) + s.b*c02
//                 for c in r, g, b:  e = y - s.c ; f = ws * e ; c' = s.c + f
//     spill == 0: c' = s.c, code for code (its own instance, not s + 0 * e)
//     out = matte view ? (a', a', a', 1) : (r', g', b', a')               f16 targets truncated once at the store
// Every operation is rounded on its own in BOTH arithmetic flavours (the stance of the field softening and the unsharp mask: no
// clang build of the reference exists for this expression to follow), so there is one build of the unit: it is not in FMA_KERN.
// The square root is __builtin_sqrtf: with this tree's flags that is v_sqrt_f32 followed by the two fused residual steps and the
// +-1 code selection, correctly rounded; __fsqrt_rn compiles to the bare scaled v_sqrt_f32, good to 1 ulp only.
//
// Bound: HBM.  A pure stream: no table, no LDS, no cross-lane traffic.  Algorithmic bytes per pixel: 8 read + 8 written on f16
// frames, 16 + 16 on f32.  Shape: field_ops.hip's (stream_common.hpp) -- a one-wave workgroup owns 64 lanes x PIX columns over a
// segment of consecutive rows, one 16-byte access per lane and row: an f32 pixel, or two half pixels where base, pitch and
// window parity of both frames allow (pair_view), else one half pixel in 8 bytes.  A pair cut by the window's left or right edge
// is loaded whole (it lies inside the buffer's row) and stored by halves.  The next row's load is issued before the current row
// is worked out.  Stores are non-temporal.  In place (target = source frame) needs nothing special: a lane reads the pixels
// it writes, each before it writes it, and no other lane touches them.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "pixel_math.hpp"
#include "stream_common.hpp"

namespace {

using namespace rowstream;

constexpr float c00 = 0.2126f, c01 = 0.7152f, c02 = 0.0722f;
constexpr float c10 = -0.114572f, c11 = -0.385428f, c12 = 0.5f;
constexpr float c20 = 0.5f, c21 = -0.454153f, c22 = -0.045847f;

__device__ __forceinline__ float ramp(float t) { return (t < 1.0f) ? ((t > 0.0f) ? t : 0.0f) : 1.0f; }

// what the key does to one pixel: the factor on its alpha and the weight that pulls its colours towards their luma
struct Keyed { float m, ws; };

template <bool SPILL>
__device__ __forceinline__ Keyed key_of(const cvk_key_params &kp, float r, float g, float b) {
    const float pb = (r * c10 + g * c11) + b * c12, pr = (r * c20 + g * c21) + b * c22;
    const float dx = pb - kp.kpb, dy = pr - kp.kpr;
    const float d = __builtin_sqrtf(dx * dx + dy * dy);
    const float hard = d <= kp.tolerance ? 0.0f : 1.0f, past = d - kp.tolerance;
    Keyed k;
    k.m = kp.soft ? ramp(past * kp.inv_soft) : hard;                   // kp.soft, kp.fade: wave-uniform
    k.ws = 0.0f;
    if (SPILL) {
        const float q = kp.fade ? ramp(past * kp.inv_spill) : hard;
        k.ws = kp.spill * (1.0f - q);
    }
    return k;
}

__device__ __forceinline__ float despill(float c, float y, float ws) {
    const float e = y - c, f = ws * e;
    return c + f;
}

// one f32 pixel as its four dwords
template <bool SPILL, bool MATTE>
__device__ __forceinline__ v4 key_f32(const cvk_key_params &kp, v4 p) {
    const float r = __uint_as_float(p.x), g = __uint_as_float(p.y), b = __uint_as_float(p.z), a = __uint_as_float(p.w);
    const Keyed k = key_of<SPILL>(kp, r, g, b);
    const uint32_t a1 = __float_as_uint(a * k.m);
    if (MATTE) return v4{ a1, a1, a1, 0x3F800000u };
    if (!SPILL) return v4{ p.x, p.y, p.z, a1 };
    const float y = (r * c00 + g * c01) + b * c02;
    return v4{ __float_as_uint(despill(r, y, k.ws)), __float_as_uint(despill(g, y, k.ws)), __float_as_uint(despill(b, y, k.ws)), a1 };
}

// one half pixel as its two dwords (lo = g:r, hi = a:b)
template <bool SPILL, bool MATTE>
__device__ __forceinline__ v2 key_f16(const cvk_key_params &kp, uint32_t lo, uint32_t hi) {
    const float r = cvs::h2f(lo & 0xFFFFu), g = cvs::h2f(lo >> 16), b = cvs::h2f(hi & 0xFFFFu), a = cvs::h2f(hi >> 16);
    const Keyed k = key_of<SPILL>(kp, r, g, b);
    const float a1 = a * k.m;
    if (MATTE) return v2{ cvs::f2h_rz2(a1, a1), cvs::f2h_rz2(a1, 1.0f) };
    if (!SPILL) return v2{ lo, (hi & 0xFFFFu) | (cvs::f2h_rz(a1) << 16) };
    const float y = (r * c00 + g * c01) + b * c02;
    return v2{ cvs::f2h_rz2(despill(r, y, k.ws), despill(g, y, k.ws)), cvs::f2h_rz2(despill(b, y, k.ws), a1) };
}

// HALF: 0 = rgba_f32 frames, one pixel per lane; 1 = rgba_f16, one pixel per lane; 2 = rgba_f16, two pixels per lane
template <int HALF>
__device__ __forceinline__ v4 load_row(const cvk_view &v, int x, int y) {
    if (HALF) return load_px<HALF>(v, x, y);
    return *reinterpret_cast<const v4 *>(static_cast<const char *>(v.data) + ((long long)(y - v.fy0) * v.pitch + (x - v.fx0)) * 16);
}

template <int HALF, bool SPILL, bool MATTE>
__global__ __launch_bounds__(kLanes) void k_chroma_key(cvk_key_params kp, cvk_view out, cvk_view in, cvk_rect w, int xs, int seg) {
    constexpr int PIX = HALF == 2 ? 2 : 1;
    ROWSTREAM_LANE(w, xs, seg)
    v4 cur = load_row<HALF>(in, x, y0);
    for (int y = y0; y <= y1; y++) {
        v4 next = cur;
        if (y < y1) next = load_row<HALF>(in, x, y + 1);                // wave-uniform
        if (HALF) {
            const v2 p0 = key_f16<SPILL, MATTE>(kp, cur.x, cur.y);
            v4 c = { p0.x, p0.y, 0u, 0u };
            if (PIX == 2) { const v2 p1 = key_f16<SPILL, MATTE>(kp, cur.z, cur.w); c.z = p1.x; c.w = p1.y; }
            store_px<PIX>(out, x, y, c, m0, m1);
        } else {
            char *p = static_cast<char *>(out.data) + ((long long)(y - out.fy0) * out.pitch + (x - out.fx0)) * 16;
            __builtin_nontemporal_store(key_f32<SPILL, MATTE>(kp, cur), reinterpret_cast<v4 *>(p));
        }
        cur = next;
    }
}

template <int HALF>
int launch(const cvk_key_params &kp, const cvk_view &out, const cvk_view &in, const cvk_rect &w, const Shape &s, hipStream_t st) {
    // the matte view shows no colour: it runs without the spill arithmetic whatever kp.spill says
    if (kp.matte) hipLaunchKernelGGL((k_chroma_key<HALF, false, true>), s.grid, dim3(kLanes), 0, st, kp, out, in, w, s.xs, s.seg);
    else if (kp.spill > 0.0f) hipLaunchKernelGGL((k_chroma_key<HALF, true, false>), s.grid, dim3(kLanes), 0, st, kp, out, in, w, s.xs, s.seg);
    else hipLaunchKernelGGL((k_chroma_key<HALF, false, false>), s.grid, dim3(kLanes), 0, st, kp, out, in, w, s.xs, s.seg);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int cvk_chroma_key(const cvk_key_params *kp, cvk_view out, cvk_view in, cvk_rect w, int half, int cus, void *stream) {
    if (rect_empty(w)) return 0;
    const int xs2 = w.x0 - (int)(((long long)w.x0 - out.fx0) & 1);
    const Shape s = shape(w, half && pair_view(out, xs2) && pair_view(in, xs2), out.fx0, cus);
    if (!half) return launch<0>(*kp, out, in, w, s, (hipStream_t)stream);
    return s.pix == 2 ? launch<2>(*kp, out, in, w, s, (hipStream_t)stream) : launch<1>(*kp, out, in, w, s, (hipStream_t)stream);
}
