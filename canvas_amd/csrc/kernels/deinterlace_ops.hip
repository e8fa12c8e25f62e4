// deinterlace_ops.hip -- motion-adaptive deinterlace of a woven half RGBA frame, with the frames before and after it.
//
//   k_deinterlace_adaptive<PIX, NEIGHBOURS>   rows of the kept field copied; every other row woven where nothing moved,
//                                             interpolated where something did, a ramp between
// No reference code (the design names the conversion, docs/sphinx/feature-proposal/canvas.rst:283-303).  The contract is
// DESIGN.md "Adaptive deinterlace" and include/canvas_deinterlace.h, restated here.  Row parity is that of the absolute plane
// coordinate.  For a row y of the window with (y & 1) == field: the codes of cur.  For every other row, per pixel (x, y):
//     sp  what k_field_to_frame makes there, per channel in f32: rows y-1 and y+1 of cur, each used if inside cur's current
//         window; both: upper * 0.5f + lower * 0.5f; one: its values; none: zeros
//     wv  cur(x, y)
//     m   the largest fabsf(cur(c, r).ch - n(c, r).ch) over the neighbour frames n, rows r in y-1..y+1, columns c in x-1..x+1 and
//         the four channels, of the samples (c, r) inside cur's and n's current windows; a NaN difference is +inf
//     k   1 where no sample counts; else soft ? ramp((m - threshold) * inv_soft) : (m <= threshold ? 0 : 1), ramp the key's
//     k == 0: the codes of wv; k == 1: what k_field_to_frame writes (the mean truncated, or the one row's codes, or zeros);
//     else per channel e = sp - wv; f = k * e; r = wv + f, truncated to half
// Every operation is rounded on its own (the build never contracts, and the unit is not in FMA_KERN): one build, both flavours.
//
// Bound: HBM.  Algorithmic bytes per output pixel: 8 written + 8 read per frame = 32 with both neighbours, 24 with one.
// Shape: the row stream of stream_common.hpp -- a one-wave workgroup walks down a segment of rows, two pixels per lane in one
// 16-byte access where all the buffers put the same pairs on 16-byte boundaries, one pixel per lane otherwise -- with two
// differences.  (1) Per row r each lane forms D(c, r), the largest difference of its own columns over channels and neighbours
// ("none": -1), once; H(x, r) = max(D(x-1), D(x), D(x+1)) takes the outer two from the neighbouring lanes (__shfl_up /
// __shfl_down), so a wave makes kMade = 62 lanes of columns: lanes 0 and 63 load the column (pair) left and right of the wave's
// run and hand it on, as lanes 0 and 63 of the MPEG-2 kernels do.  All lanes run the same instructions (no lane leaves early: a
// shuffle reads every lane); no LDS, no barrier.  (2) The walk keeps a three-deep ring of cur's rows and of H in registers:
// m(x, y) = max(H(x, y-1), H(x, y), H(x, y+1)), so every row of every frame is read once per segment (plus the two seam rows)
// and each kept row's H serves the made rows above and below it.  Row r + 1's loads are issued before row r is worked out.
// Differences are compared as the bit patterns of their absolute values in signed integers: finite < +inf < NaN in that
// order and "none" (-1) below all, so the maxima are v_max3_i32 and a NaN becomes +inf by one v_min at the end.
// A lane reads a frame only in columns that frame's window (grown by nothing) holds and the window written (grown by one) needs:
// a pair cut by an edge is loaded whole, it lies inside the buffer's row.  Stores are non-temporal.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "pixel_math.hpp"
#include "stream_common.hpp"

namespace {

using namespace rowstream;

constexpr int kMade = kLanes - 2;          // lanes 1 .. 62 make columns
constexpr int kNone = -1;                  // no sample counts
constexpr int kInf = 0x7F800000;

__device__ __forceinline__ float ramp(float t) { return (t < 1.0f) ? ((t > 0.0f) ? t : 0.0f) : 1.0f; }
__device__ __forceinline__ int max3(int a, int b, int c) { return max(max(a, b), c); }

// |a - b| of one channel as a signed integer: its bits with the sign cleared
__device__ __forceinline__ int adiff(uint32_t a, uint32_t b) {
    const float d = cvs::h2f(a) - cvs::h2f(b);
    return (int)(__builtin_bit_cast(uint32_t, d) & 0x7FFFFFFFu);
}
// the four channels of one pixel (lo = g:r, hi = a:b)
__device__ __forceinline__ int pixel_diff(uint32_t alo, uint32_t ahi, uint32_t blo, uint32_t bhi) {
    return max(max(adiff(alo & 0xFFFFu, blo & 0xFFFFu), adiff(alo >> 16, blo >> 16)), max(adiff(ahi & 0xFFFFu, bhi & 0xFFFFu), adiff(ahi >> 16, bhi >> 16)));
}

// the weight of the interpolated candidate from the neighbourhood's largest difference
__device__ __forceinline__ float weight(int m, const cvk_deinterlace_params &p) {
    const float mf = __builtin_bit_cast(float, min(m, kInf));
    const float hard = mf <= p.threshold ? 0.0f : 1.0f;
    const float past = mf - p.threshold;
    const float k = p.soft ? ramp(past * p.inv_soft) : hard;          // p.soft: wave-uniform
    return m < 0 ? 1.0f : k;
}

// two channels of a made row.  up_ok / dn_ok: rows y - 1 / y + 1 lie inside cur's current window (wave-uniform)
__device__ __forceinline__ uint32_t made2(uint32_t up, uint32_t mid, uint32_t dn, bool up_ok, bool dn_ok, float k) {
    const float w0 = cvs::h2f(mid & 0xFFFFu), w1 = cvs::h2f(mid >> 16);
    float s0, s1;
    uint32_t sp;
    if (up_ok && dn_ok) {
        const float t0 = cvs::h2f(up & 0xFFFFu) * 0.5f, t1 = cvs::h2f(up >> 16) * 0.5f;
        const float u0 = cvs::h2f(dn & 0xFFFFu) * 0.5f, u1 = cvs::h2f(dn >> 16) * 0.5f;
        s0 = t0 + u0; s1 = t1 + u1;
        sp = cvs::f2h_rz2(s0, s1);
    } else {
        sp = up_ok ? up : (dn_ok ? dn : 0u);
        s0 = cvs::h2f(sp & 0xFFFFu); s1 = cvs::h2f(sp >> 16);
    }
    const float e0 = s0 - w0, e1 = s1 - w1;
    const float f0 = k * e0, f1 = k * e1;
    const uint32_t blend = cvs::f2h_rz2(w0 + f0, w1 + f1);
    return k == 0.0f ? mid : (k == 1.0f ? sp : blend);
}

template <int PIX>
__device__ __forceinline__ bool columns_inside(const cvk_view &v, int x) { return x >= v.fx0 && x + PIX - 1 <= v.fx1; }

template <int PIX, int NB>
__global__ __launch_bounds__(kLanes) void k_deinterlace_adaptive(cvk_deinterlace_params p) {
    const cvk_rect w = p.w, cw = p.cw;
    const int lane = (int)threadIdx.x;
    const int x = p.xs + PIX * ((int)blockIdx.x * kMade + lane - 1);
    const bool made = lane >= 1 && lane <= kMade;
    const bool m0 = made && x >= w.x0 && x <= w.x1, m1 = PIX == 2 && made && x + 1 >= w.x0 && x + 1 <= w.x1;
    const int y0 = w.y0 + (int)blockIdx.y * p.seg, y1 = min(y0 + p.seg - 1, w.y1);
    // the columns whose differences a made column of this wave reads
    const bool wanted = x + PIX - 1 >= w.x0 - 1 && x <= w.x1 + 1;
    // which of the lane's pixels lie inside cur's window / count against neighbour j
    const bool c0 = x >= cw.x0 && x <= cw.x1, c1 = PIX == 2 && x + 1 >= cw.x0 && x + 1 <= cw.x1;
    const bool load_cur = wanted && (c0 || c1) && columns_inside<PIX>(p.cur, x);
    bool n0[NB], n1[NB], load_n[NB];
#pragma unroll
    for (int j = 0; j < NB; j++) {
        n0[j] = x >= p.v[j].x0 && x <= p.v[j].x1;
        n1[j] = PIX == 2 && x + 1 >= p.v[j].x0 && x + 1 <= p.v[j].x1;
        load_n[j] = load_cur && (n0[j] || n1[j]) && columns_inside<PIX>(p.n[j], x);
    }
    const v4 zero = { 0u, 0u, 0u, 0u };

    // the ring: rows r - 2, r - 1, r of cur and of H once row r has been taken in
    v4 ca = zero, cb = zero, cc = zero;
    int ha0 = kNone, ha1 = kNone, hb0 = kNone, hb1 = kNone, hc0 = kNone, hc1 = kNone;
    // row r as loaded
    int r = y0 - 1;
    bool row_c = r >= cw.y0 && r <= cw.y1;                                             // wave-uniform, as every row test below
    v4 lc = row_c && load_cur ? load_px<PIX>(p.cur, x, r) : zero, ln[NB];
#pragma unroll
    for (int j = 0; j < NB; j++) ln[j] = r >= p.v[j].y0 && r <= p.v[j].y1 && load_n[j] ? load_px<PIX>(p.n[j], x, r) : zero;

    for (; r <= y1 + 1; r++) {
        // the next row's loads, before this row's arithmetic
        const int q = r + 1;
        const bool next_c = q <= y1 + 1 && q >= cw.y0 && q <= cw.y1;
        v4 nc = zero, nn[NB];
        if (next_c && load_cur) nc = load_px<PIX>(p.cur, x, q);
#pragma unroll
        for (int j = 0; j < NB; j++) {
            nn[j] = zero;
            if (q <= y1 + 1 && q >= p.v[j].y0 && q <= p.v[j].y1 && load_n[j]) nn[j] = load_px<PIX>(p.n[j], x, q);
        }

        // D of the lane's columns in row r, then H with the neighbouring lanes' columns
        int d0 = kNone, d1 = kNone;
#pragma unroll
        for (int j = 0; j < NB; j++) {
            const bool row_n = r >= p.v[j].y0 && r <= p.v[j].y1;
            const int e0 = pixel_diff(lc.x, lc.y, ln[j].x, ln[j].y);
            d0 = row_n && n0[j] ? max(d0, e0) : d0;
            if (PIX == 2) {
                const int e1 = pixel_diff(lc.z, lc.w, ln[j].z, ln[j].w);
                d1 = row_n && n1[j] ? max(d1, e1) : d1;
            }
        }
        const int left = __shfl_up(PIX == 2 ? d1 : d0, 1), right = __shfl_down(d0, 1);
        ca = cb; cb = cc; cc = lc;
        ha0 = hb0; hb0 = hc0; ha1 = hb1; hb1 = hc1;
        if (PIX == 2) { hc0 = max3(left, d0, d1); hc1 = max3(d0, d1, right); }
        else hc0 = max3(left, d0, right);

        // row y = r - 1 has its three rows in the ring
        const int y = r - 1;
        if (y >= y0) {
            if ((y & 1) == p.field) store_px<PIX>(p.out, x, y, cb, m0, m1);
            else {
                const bool up_ok = y - 1 >= cw.y0, dn_ok = y + 1 <= cw.y1;
                const float k0 = weight(max3(ha0, hb0, hc0), p);
                v4 o = { made2(ca.x, cb.x, cc.x, up_ok, dn_ok, k0), made2(ca.y, cb.y, cc.y, up_ok, dn_ok, k0), 0u, 0u };
                if (PIX == 2) {
                    const float k1 = weight(max3(ha1, hb1, hc1), p);
                    o.z = made2(ca.z, cb.z, cc.z, up_ok, dn_ok, k1);
                    o.w = made2(ca.w, cb.w, cc.w, up_ok, dn_ok, k1);
                }
                store_px<PIX>(p.out, x, y, o, m0, m1);
            }
        }
        lc = nc;
#pragma unroll
        for (int j = 0; j < NB; j++) ln[j] = nn[j];
    }
}

template <int PIX, int NB>
void launch(const cvk_deinterlace_params &p, dim3 grid, hipStream_t stream) {
    hipLaunchKernelGGL((k_deinterlace_adaptive<PIX, NB>), grid, dim3(kLanes), 0, stream, p);
}

}  // namespace

extern "C" int cvk_deinterlace_adaptive(const cvk_deinterlace_params *dp, int neighbours, int cus, void *stream) {
    cvk_deinterlace_params p = *dp;
    if (rect_empty(p.w)) return 0;
    if (neighbours != 1 && neighbours != 2) return (int)hipErrorInvalidValue;
    const int xs2 = p.w.x0 - (int)(((long long)p.w.x0 - p.out.fx0) & 1);
    bool pairs = pair_view(p.out, xs2) && pair_view(p.cur, xs2);
    for (int j = 0; j < neighbours; j++) pairs = pairs && pair_view(p.n[j], xs2);
    const Shape s = shape(p.w, pairs, p.out.fx0, cus, kMade);
    p.xs = s.xs; p.seg = s.seg;
    hipStream_t st = (hipStream_t)stream;
    if (s.pix == 2) { if (neighbours == 2) launch<2, 2>(p, s.grid, st); else launch<2, 1>(p, s.grid, st); }
    else { if (neighbours == 2) launch<1, 2>(p, s.grid, st); else launch<1, 1>(p, s.grid, st); }
    return (int)hipGetLastError();
}
