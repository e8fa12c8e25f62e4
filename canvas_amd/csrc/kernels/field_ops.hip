// field_ops.hip -- conversions between woven (interlaced) frames and whole pictures on half RGBA device frames.
//
//   k_field_to_frame    one field made into a whole picture (bob / discard-a-field deinterlace)
//   k_soften_fields     vertical [1/4, 1/2, 1/4] before weaving ("weave interlace" of the design, canvas.rst:283-303)
//   k_interlace_fields  two pictures woven into one frame (bob interlace, 2:3 pulldown addition)
// No reference code (the design lists the conversions, docs/sphinx/feature-proposal/canvas.rst:283-303, and
// fluggo/editor/model/sources.py:536-542 names them; only the pulldown removal was built).  The contract is DESIGN.md "Field
// conversions", restated here.  Row parity is that of the absolute plane coordinate, y & 1 in two's complement.
//     field_to_frame  rows with (y & 1) == field: the codes of `in`, copied.  Every other row: from rows y-1 and y+1 of `in`, each
//                     used if it lies inside in's current window; both: per channel (alpha included, un-premultiplied, as
//                     video_scale.c filters) t = upper * 0.5f; u = lower * 0.5f; r = t + u, truncated to half; one: its codes;
//                     none: four zero halfs
//     soften          t = a * 0.25f; t = t + b * 0.5f; t = t + c * 0.25f with a, b, c rows y-1, y, y+1 of `in`; a neighbour
//                     outside in's current window is row y itself; truncated to half
//     interlace       even rows from `even`, odd rows from `odd`, code for code; outside the provider's current window zero
// Every product is by a power of two and exact for every finite widened half, so a fused multiply-add rounds where the separate
// product and sum do: one build serves both arithmetic flavours (the unit is not in FMA_KERN), bit for bit.
//
// Bound: HBM.  Pure streams: no table, no LDS, no cross-lane traffic.  Algorithmic bytes per output pixel:
//     field_to_frame 4 read + 8 written (only the rows of the kept field are read, each once per segment)
//     soften         8 + 8        interlace 8 + 8 (only the rows each input provides)
// Shape: a one-wave workgroup owns 64 lanes x kPix columns over a segment of consecutive rows and walks down them with the rows it
// still needs in registers (field_to_frame: the previous field row; soften: a three-row window), the next row's load issued before
// the current row is worked out.  A segment re-reads the row (soften: two rows) at its seam.  Two pixels per lane, one 16-byte
// access per row, where every buffer involved puts the same column pairs on 16-byte boundaries (launcher: pairs_align); one pixel
// per lane and 8-byte accesses otherwise.  A pair cut by the window's left or right edge is loaded whole (it lies inside the
// buffer's row) and stored by halves.  Stores are non-temporal: nothing here reads its output again.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "pixel_math.hpp"
#include "stream_common.hpp"

namespace {

using namespace rowstream;

// two channels: upper * 0.5 + lower * 0.5, one rounding in the sum
__device__ __forceinline__ uint32_t mean2(uint32_t upper, uint32_t lower) {
    const float t0 = cvs::h2f(upper & 0xFFFFu) * 0.5f, t1 = cvs::h2f(upper >> 16) * 0.5f;
    const float u0 = cvs::h2f(lower & 0xFFFFu) * 0.5f, u1 = cvs::h2f(lower >> 16) * 0.5f;
    return cvs::f2h_rz2(t0 + u0, t1 + u1);
}
template <int PIX>
__device__ __forceinline__ v4 mean_px(v4 upper, v4 lower) {
    v4 r = { mean2(upper.x, lower.x), mean2(upper.y, lower.y), 0u, 0u };
    if (PIX == 2) { r.z = mean2(upper.z, lower.z); r.w = mean2(upper.w, lower.w); }
    return r;
}

// two channels: (a * 0.25 + b * 0.5) + c * 0.25, two roundings
__device__ __forceinline__ float soft1(float a, float b, float c) {
    float t = a * 0.25f;
    t = t + b * 0.5f;
    t = t + c * 0.25f;
    return t;
}
__device__ __forceinline__ uint32_t soft2(uint32_t a, uint32_t b, uint32_t c) {
    return cvs::f2h_rz2(soft1(cvs::h2f(a & 0xFFFFu), cvs::h2f(b & 0xFFFFu), cvs::h2f(c & 0xFFFFu)),
                        soft1(cvs::h2f(a >> 16), cvs::h2f(b >> 16), cvs::h2f(c >> 16)));
}
template <int PIX>
__device__ __forceinline__ v4 soft_px(v4 a, v4 b, v4 c) {
    v4 r = { soft2(a.x, b.x, c.x), soft2(a.y, b.y, c.y), 0u, 0u };
    if (PIX == 2) { r.z = soft2(a.z, b.z, c.z); r.w = soft2(a.w, b.w, c.w); }
    return r;
}

// `rows`: the rows of in's current window (w's columns lie inside it).  The walk goes over the rows r of the kept field from the
// one at or above y0 to the one at or below y1 + 1: row r - 1 is made from rows r - 2 and r, row r is copied.
template <int PIX>
__global__ __launch_bounds__(kLanes) void k_field_to_frame(cvk_view out, cvk_view in, cvk_rect w, int rows0, int rows1, int field, int xs, int seg) {
    ROWSTREAM_LANE(w, xs, seg)
    const int first = (y0 & 1) == field ? y0 : y0 - 1;
    const v4 zero = { 0u, 0u, 0u, 0u };
    bool have_prev = false, have_cur = first >= rows0 && first <= rows1;
    v4 prev = zero, cur = have_cur ? load_px<PIX>(in, x, first) : zero;
    for (int r = first; r <= y1 + 1; r += 2) {
        const bool have_next = r + 2 <= y1 + 1 && r + 2 >= rows0 && r + 2 <= rows1;     // wave-uniform
        const v4 next = have_next ? load_px<PIX>(in, x, r + 2) : zero;
        if (r - 1 >= y0 && r - 1 <= y1) store_px<PIX>(out, x, r - 1, have_prev && have_cur ? mean_px<PIX>(prev, cur) : (have_prev ? prev : cur), m0, m1);
        if (r >= y0 && r <= y1) store_px<PIX>(out, x, r, cur, m0, m1);
        prev = cur; have_prev = have_cur;
        cur = next; have_cur = have_next;
    }
}

template <int PIX>
__global__ __launch_bounds__(kLanes) void k_soften_fields(cvk_view out, cvk_view in, cvk_rect w, int rows0, int rows1, int xs, int seg) {
    ROWSTREAM_LANE(w, xs, seg)
    v4 cur = load_px<PIX>(in, x, y0);
    v4 prev = y0 - 1 >= rows0 ? load_px<PIX>(in, x, y0 - 1) : cur;
    bool have_next = y0 + 1 <= rows1;
    v4 next = have_next ? load_px<PIX>(in, x, y0 + 1) : cur;
    for (int y = y0; y <= y1; y++) {
        const bool have_after = y < y1 && y + 2 <= rows1;                               // wave-uniform
        v4 after = next;
        if (have_after) after = load_px<PIX>(in, x, y + 2);
        store_px<PIX>(out, x, y, soft_px<PIX>(prev, cur, have_next ? next : cur), m0, m1);
        prev = cur; cur = next;
        next = after; have_next = have_after;
    }
}

// ew / ow: the current windows of `even` and `odd`
template <int PIX>
__global__ __launch_bounds__(kLanes) void k_interlace_fields(cvk_view out, cvk_view even, cvk_view odd, cvk_rect w, cvk_rect ew, cvk_rect ow, int xs, int seg) {
    ROWSTREAM_LANE(w, xs, seg)
    const bool e0 = x >= ew.x0 && x <= ew.x1, e1 = PIX == 2 && x + 1 >= ew.x0 && x + 1 <= ew.x1;
    const bool o0 = x >= ow.x0 && x <= ow.x1, o1 = PIX == 2 && x + 1 >= ow.x0 && x + 1 <= ow.x1;
#pragma unroll 4
    for (int y = y0; y <= y1; y++) {
        const bool is_odd = (y & 1) != 0;
        const cvk_view &src = is_odd ? odd : even;
        const cvk_rect &sw = is_odd ? ow : ew;
        const bool row = y >= sw.y0 && y <= sw.y1;                                      // wave-uniform
        const bool p0 = row && (is_odd ? o0 : e0), p1 = row && (is_odd ? o1 : e1);
        v4 c = { 0u, 0u, 0u, 0u };
        if (PIX == 2 && p0 && p1) c = load_px<2>(src, x, y);
        else {
            if (p0) { const v4 t = load_px<1>(src, x, y); c.x = t.x; c.y = t.y; }
            if (PIX == 2 && p1) { const v4 t = load_px<1>(src, x + 1, y); c.z = t.x; c.w = t.y; }
        }
        store_px<PIX>(out, x, y, c, m0, m1);
    }
}

}  // namespace

extern "C" int cvk_field_to_frame(cvk_view out, cvk_view in, cvk_rect w, cvk_rect in_cur, int field, int cus, void *stream) {
    if (rect_empty(w)) return 0;
    const int xs2 = w.x0 - (int)(((long long)w.x0 - out.fx0) & 1);
    const Shape s = shape(w, pair_view(out, xs2) && pair_view(in, xs2), out.fx0, cus);
    if (s.pix == 2) hipLaunchKernelGGL(k_field_to_frame<2>, s.grid, dim3(kLanes), 0, (hipStream_t)stream, out, in, w, in_cur.y0, in_cur.y1, field, s.xs, s.seg);
    else hipLaunchKernelGGL(k_field_to_frame<1>, s.grid, dim3(kLanes), 0, (hipStream_t)stream, out, in, w, in_cur.y0, in_cur.y1, field, s.xs, s.seg);
    return (int)hipGetLastError();
}

extern "C" int cvk_soften_fields(cvk_view out, cvk_view in, cvk_rect w, cvk_rect in_cur, int cus, void *stream) {
    if (rect_empty(w)) return 0;
    const int xs2 = w.x0 - (int)(((long long)w.x0 - out.fx0) & 1);
    const Shape s = shape(w, pair_view(out, xs2) && pair_view(in, xs2), out.fx0, cus);
    if (s.pix == 2) hipLaunchKernelGGL(k_soften_fields<2>, s.grid, dim3(kLanes), 0, (hipStream_t)stream, out, in, w, in_cur.y0, in_cur.y1, s.xs, s.seg);
    else hipLaunchKernelGGL(k_soften_fields<1>, s.grid, dim3(kLanes), 0, (hipStream_t)stream, out, in, w, in_cur.y0, in_cur.y1, s.xs, s.seg);
    return (int)hipGetLastError();
}

extern "C" int cvk_interlace_fields(cvk_view out, cvk_view even, cvk_view odd, cvk_rect w, cvk_rect even_cur, cvk_rect odd_cur, int cus, void *stream) {
    if (rect_empty(w)) return 0;
    const int xs2 = w.x0 - (int)(((long long)w.x0 - out.fx0) & 1);
    // an input without pixels is never read: its view need not line up
    const bool pairs = pair_view(out, xs2) && (rect_empty(even_cur) || pair_view(even, xs2)) && (rect_empty(odd_cur) || pair_view(odd, xs2));
    const Shape s = shape(w, pairs, out.fx0, cus);
    if (s.pix == 2) hipLaunchKernelGGL(k_interlace_fields<2>, s.grid, dim3(kLanes), 0, (hipStream_t)stream, out, even, odd, w, even_cur, odd_cur, s.xs, s.seg);
    else hipLaunchKernelGGL(k_interlace_fields<1>, s.grid, dim3(kLanes), 0, (hipStream_t)stream, out, even, odd, w, even_cur, odd_cur, s.xs, s.seg);
    return (int)hipGetLastError();
}
