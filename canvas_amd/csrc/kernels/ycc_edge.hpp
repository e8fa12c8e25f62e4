// ycc_edge.hpp -- what the six Y'CbCr edge kernels compute alike: mpeg2_ops.hip, mpeg2_recon_ops.hip, ycc422_ops.hip,
// ycc422_recon_ops.hip, ycc420_ops.hip and ycc420_recon_ops.hip.  The pixel fetch of the export edges, the matrix in both
// directions, the quantiser, the 1/4 1/2 1/4 filter, the two-sample accesses, the decode tables, the pixel-pair store, and on the
// host the strip plan of the persistent launch.  Schedules, unit shapes and kMaxStrip stay with each kernel; the table's placement
// is table_placement.hpp's.
//
// Every product and every sum here rounds on its own: the arithmetic relies on -ffp-contract=off, and the pixels must not depend
// on the arithmetic flavour.
#pragma once
#ifdef CVS_CONTRACT
#error "the Y'CbCr edge units are built once, not in FMA_KERN: no FMA in either arithmetic flavour"
#endif
#include <hip/hip_runtime.h>
#include <type_traits>
#include "kernels.h"
#include "pixel_math.hpp"
#include "table_placement.hpp"

namespace cvs {

typedef uint32_t v4 __attribute__((ext_vector_type(4)));
typedef uint32_t v4a8 __attribute__((ext_vector_type(4), aligned(8)));     // a pixel pair: 8-byte aligned only

__device__ __forceinline__ bool aligned(const void *p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---- export: half RGBA -> codes

// Pixels (x, y) and (x + 1, y) as four dwords {rg0, ba0, rg1, ba1}; zero where a pixel is outside `w`.  Preconditions: `w` lies
// inside the view (or is empty with x1 < x0 and y1 < y0, which reads nothing), so every pixel that passes its test is addressable;
// x is even or not, but |x| stays within the coordinate bound, so x + 1 does not wrap.  Under these the early return (pair wholly
// left or right of w), then "x >= w.x0" and "x + 1 <= w.x1" alone, decide each pixel exactly as the full tests x0 <= x <= x1 and
// x0 <= x + 1 <= x1 do.  Blocks left of the raster (a wave's lane 0 at the left edge) are the callers' to refuse.
__device__ __forceinline__ v4 fetch_pair(const cvk_view &f, const cvk_rect &w, long long x, int y) {
    v4 v = { 0u, 0u, 0u, 0u };
    if (y < w.y0 || y > w.y1 || x + 1 < w.x0 || x > w.x1) return v;
    const uint2 *p = reinterpret_cast<const uint2 *>(f.data) + (ptrdiff_t)(y - f.fy0) * (ptrdiff_t)f.pitch + (x - f.fx0);
    if (x >= w.x0 && x + 1 <= w.x1) return __builtin_nontemporal_load(reinterpret_cast<const v4a8 *>(p));
    if (x >= w.x0) { const uint2 a = p[0]; v.x = a.x; v.y = a.y; }
    if (x + 1 <= w.x1) { const uint2 a = p[1]; v.z = a.x; v.w = a.y; }
    return v;
}

struct Mat9 { float m0, m1, m2, m3, m4, m5, m6, m7, m8; };      // a 3x3 matrix row by row
__host__ __device__ inline Mat9 mat9(const float m[9]) { return Mat9{ m[0], m[1], m[2], m[3], m[4], m[5], m[6], m[7], m[8] }; }
struct Ycc { float y, cb, cr; };

// r, g, b through the table where there is one, widened to f32, times the R'G'B' -> Y'CbCr matrix; alpha ignored
template <int TABLE>
__device__ __forceinline__ Ycc encode(uint32_t rg, uint32_t ba, const Mat9 &m, const uint16_t *t) {
    float r, g, b;
    if constexpr (TABLE == kTableNone) { r = h2f(rg & 0xFFFFu); g = h2f(rg >> 16); b = h2f(ba & 0xFFFFu); }
    else { r = h2f(t[rg & 0xFFFFu]); g = h2f(t[rg >> 16]); b = h2f(t[ba & 0xFFFFu]); }
    Ycc o;
    o.y = (r * m.m0 + g * m.m1) + b * m.m2;
    o.cb = (r * m.m3 + g * m.m4) + b * m.m5;
    o.cr = (r * m.m6 + g * m.m7) + b * m.m8;
    return o;
}

// what GL stores into a normalised texture: scale, clamp (maxnum / minnum: NaN -> 0), round half to even; then the code's own
// clamp (10-bit studio range reserves 0-3 and 1020-1023; lo = 0 and hi = top clamp nothing)
__device__ __forceinline__ uint32_t quantise(float v, float scale, float offset, float top, uint32_t lo, uint32_t hi) {
    const float q = v * scale + offset;
    const uint32_t code = (uint32_t)__builtin_rintf(__builtin_fminf(__builtin_fmaxf(q, 0.0f), 1.0f) * top);
    __builtin_assume(code <= (uint32_t)top);      // (which the compiler does not see through the rounding: it lets a constant hi >= top fold)
    return min(max(code, lo), hi);
}

// the 1/4, 1/2, 1/4 filter, left to right
__device__ __forceinline__ float tent(float a, float b, float c) {
    float v = 0.25f * a;
    v = v + 0.5f * b;
    v = v + 0.25f * c;
    return v;
}

// two neighbouring samples: 8-bit one 16-bit access, 10-bit one 32-bit access, where aligned; sample by sample otherwise
template <bool TEN>
__device__ __forceinline__ void store_two(uint8_t *p, uint32_t a, uint32_t b) {
    if constexpr (TEN) {
        if (aligned(p, 4)) *reinterpret_cast<uint32_t *>(p) = a | (b << 16);
        else { reinterpret_cast<uint16_t *>(p)[0] = (uint16_t)a; reinterpret_cast<uint16_t *>(p)[1] = (uint16_t)b; }
    } else {
        if (aligned(p, 2)) *reinterpret_cast<uint16_t *>(p) = (uint16_t)(a | (b << 8));
        else { p[0] = (uint8_t)a; p[1] = (uint8_t)b; }
    }
}

// ---- import: codes -> half RGBA

// as one word: 8-bit a | b << 8, 10-bit a | b << 16 (raw: the bits that carry no code still in place)
template <bool TEN>
__device__ __forceinline__ uint32_t load_two(const uint8_t *p) {
    if constexpr (TEN) {
        if (aligned(p, 4)) return *reinterpret_cast<const uint32_t *>(p);
        const uint16_t *q = reinterpret_cast<const uint16_t *>(p);
        return (uint32_t)q[0] | ((uint32_t)q[1] << 16);
    } else {
        if (aligned(p, 2)) return *reinterpret_cast<const uint16_t *>(p);
        return (uint32_t)p[0] | ((uint32_t)p[1] << 8);
    }
}

// the decode tables of N codes per kind, f = ((float)code - off) / div, correctly rounded: built in LDS by every workgroup with
// the same division; the caller's __syncthreads() ends it
template <int N, int LANES>
__device__ __forceinline__ void build_decode(float *dec_y, float *dec_c, float y_off, float y_div, float c_off, float c_div) {
    for (int i = threadIdx.x; i < N; i += LANES) {
        dec_y[i] = ((float)i - y_off) / y_div;
        dec_c[i] = ((float)i - c_off) / c_div;
    }
}

// one pixel: the Y'CbCr -> R'G'B' matrix, f2h_rz, {rg, ba} codes through the table where there is one (`alpha` has been already)
template <int TABLE>
__device__ __forceinline__ uint2 pixel(float yf, float cb, float cr, const Mat9 &m, const uint16_t *t, uint32_t alpha) {
    const float r = (yf * m.m0 + cb * m.m1) + cr * m.m2;
    const float g = (yf * m.m3 + cb * m.m4) + cr * m.m5;
    const float b = (yf * m.m6 + cb * m.m7) + cr * m.m8;
    const uint32_t rg = f2h_rz2(r, g), bc = f2h_rz(b);
    if constexpr (TABLE == kTableNone) return make_uint2(rg, bc | (alpha << 16));
    else return make_uint2((uint32_t)t[rg & 0xFFFFu] | ((uint32_t)t[rg >> 16] << 16), (uint32_t)t[bc] | (alpha << 16));
}

// pixels p0, p1 to o[0], o[1], each where it is inside the window: one 16-byte store where both are and the pair is aligned
// (non-temporal where neighbouring lanes write neighbouring pairs), 8-byte stores otherwise.  NONTEMPORAL is a template parameter
// on purpose: as a function argument the two 16-byte stores are merged into one before the constant arrives, and the merged store
// is a plain one (measured: the byte layouts' 4:2:2 import 10% slower at 3840x2160).
template <bool NONTEMPORAL>
__device__ __forceinline__ void store_pixel_pair(uint2 *o, uint2 p0, uint2 p1, bool in0, bool in1) {
    if (in0 && in1 && aligned(o, 16)) {
        if constexpr (NONTEMPORAL) __builtin_nontemporal_store(v4{ p0.x, p0.y, p1.x, p1.y }, reinterpret_cast<v4 *>(o));
        else *reinterpret_cast<v4 *>(o) = v4{ p0.x, p0.y, p1.x, p1.y };
    } else {
        if (in0) o[0] = p0;
        if (in1) o[1] = p1;
    }
}

// ---- host: the persistent launch over (strip of rows, run of lanes) units

// `chunks` runs per row and `rows` rows of work on a raster of `pixels`: where the table lives, at most `most` workgroups, `strip`
// rows per unit and `units` of them.  The strip is the fewest rows that leave no unit without a wave (one trip per wave where the
// raster allows it, no second round for a few waves), max_strip at most.  Some CUs may stay idle (4K interlaced MPEG-2: 210 of 256
// workgroups); handing every wave an equal share instead fills them all but spreads neighbouring waves' stores over rows far
// apart, and measured slower at 4K.  Without a table the launch is the gathered form's: small workgroups, several
// per CU.  False where the units do not fit the kernels' int arithmetic.
struct StripPlan { int table; long long most, strip, units; };

inline bool plan_strips(long long chunks, long long rows, long long pixels, bool has_lut, long long cus, int max_strip, StripPlan *p) {
    if (chunks * rows > 0x7FFFFFFFLL - (1LL << 20)) return false;
    // (the diagnostic build's CVS_MPEG2_TABLE: any value other than the L2 form's means LDS here)
    p->table = !has_lut ? kTableNone : (table_placement(pixels) == kTableL2 ? kTableL2 : kTableLds);
    p->most = table_workgroups(p->table, cus);
    const long long waves = p->most * (table_lanes(p->table) / 64);
    const long long strip = (chunks * rows + waves - 1) / waves;
    p->strip = strip < 1 ? 1 : (strip > max_strip ? max_strip : strip);
    p->units = chunks * ((rows + p->strip - 1) / p->strip);
    return true;
}

// f(TABLE, LANES) with the two as compile-time constants, for a table that is there: launch<TABLE(), LANES()>(...)
template <class F>
inline void with_table(int table, F f) {
    if (table == kTableL2) f(std::integral_constant<int, kTableL2>{}, std::integral_constant<int, kTableL2Lanes>{});
    else f(std::integral_constant<int, kTableLds>{}, std::integral_constant<int, kTableLdsLanes>{});
}

}  // namespace cvs
