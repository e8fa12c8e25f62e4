// temporal_ops.hip -- motion-adaptive temporal denoise of a half RGBA frame with the two or four frames around it in time.
//
//   k_temporal_denoise<PIX, NEIGHBOURS>   each pixel averaged with the same pixel of the neighbouring frames, each neighbour
//                                         weighted by how little moved between it and cur in the 3 x 3 pixels around the pixel
// No reference code.  The contract is DESIGN.md "Temporal denoise" and include/canvas_temporal.h, restated here.  The neighbours
// n[0 .. NEIGHBOURS) come in the contract's order of summation (prev1, next1, prev2, next2, those left out closed up).  Per
// neighbour n and pixel (x, y) of the window written:
//     m_n  the largest fabsf(cur(c, r).ch - n(c, r).ch) over rows r in y-1..y+1, columns c in x-1..x+1 and the selected channels,
//          of the samples (c, r) inside cur's and n's current windows; a NaN difference is +inf
//     v_n  0 where (x, y) lies outside n's window or no sample counts; else soft ? 1 - ramp((m_n - threshold) * inv_soft)
//          : (m_n <= threshold ? 1 : 0), ramp the key's
//     w_n  v_n for a near frame, min(v_n, w of the nearer frame on its side) for a far one
// per selected channel acc = cur.ch, W = 1; for each n in order with w_n > 0: t = w_n * n.ch; acc = acc + t; W = W + w_n;
// inv = 1 / W (one IEEE divide per pixel); o = acc * inv, truncated to half.  Every weight 0: cur's codes, whole; unselected
// channels: cur's codes.  Every operation is rounded on its own (the build never contracts, and the unit is not in FMA_KERN):
// one build, both flavours.
//
// Bound: HBM.  Algorithmic bytes per output pixel: 8 written + 8 read per frame = 32 with two neighbours, 48 with four.
// Shape: deinterlace_ops.hip's row stream over stream_common.hpp -- a one-wave workgroup walks down a segment of rows, two pixels
// per lane in one 16-byte access where all the buffers put the same pairs on 16-byte boundaries, one pixel per lane otherwise;
// per row r each lane forms D_n(c, r), the largest difference of its own columns over the selected channels ("none": -1), and
// H_n(x, r) = max(D_n(x-1), D_n(x), D_n(x+1)) takes the outer two from the neighbouring lanes (__shfl_up / __shfl_down), so a
// wave makes kMade = 62 lanes of columns and lanes 0 and 63 load the column (pair) left and right of the wave's run and hand it
// on.  All lanes run the same instructions; no LDS, no barrier.  Row r + 1's loads are issued before row r is worked out.
// Two differences from the deinterlacer: the three-row ring of H is kept PER NEIGHBOUR (weights are per frame:
// m_n(x, y) = max(H_n(x, y-1), H_n(x, y), H_n(x, y+1))), and each neighbour's pixels are kept one row back beside cur's, because
// the result needs n(x, y) when row y + 1 has been taken in.  Differences are compared as the bit patterns of their absolute
// values in signed integers: finite < +inf < NaN in that order and "none" (-1) below all, so the maxima are v_max3_i32 and a NaN
// becomes +inf by one v_min at the end.  A lane reads a frame only in columns that frame's window holds and the window written
// (grown by one) needs: a pair cut by an edge is loaded whole, it lies inside the buffer's row.  Stores are non-temporal.
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

// the two channels of a dword, widened
__device__ __forceinline__ cvs::f32x2 widen2(uint32_t c) { return cvs::f32x2{ cvs::h2f(c & 0xFFFFu), cvs::h2f(c >> 16) }; }
// the larger |a - b| of the two channels of a dword as a signed integer: the differences' bits under m0 / m1, which clear the sign
// of a selected channel and everything of one that is not (0 then: never above a selected channel's difference)
__device__ __forceinline__ int adiff2(uint32_t a, uint32_t b, uint32_t m0, uint32_t m1) {
    const cvs::f32x2 d = widen2(a) - widen2(b);
    const float d0 = d.x, d1 = d.y;                    // (a bit cast of a vector's element would read the vector's first)
    return max((int)(__builtin_bit_cast(uint32_t, d0) & m0), (int)(__builtin_bit_cast(uint32_t, d1) & m1));
}
struct ChannelMasks { uint32_t r, g, b, a; };          // 0x7FFFFFFF for a selected channel, 0 otherwise; wave-uniform
// the selected channels of one pixel (lo = g:r, hi = a:b)
__device__ __forceinline__ int pixel_diff(uint32_t alo, uint32_t ahi, uint32_t blo, uint32_t bhi, const ChannelMasks &m) {
    return max(adiff2(alo, blo, m.r, m.g), adiff2(ahi, bhi, m.b, m.a));
}

// a neighbour's raw weight from its neighbourhood's largest difference; inside: the pixel itself lies inside the neighbour's window
__device__ __forceinline__ float raw_weight(int m, bool inside, const cvk_temporal_params &p) {
    const float mf = __builtin_bit_cast(float, min(m, kInf));
    const float hard = mf <= p.threshold ? 1.0f : 0.0f;
    const float past = mf - p.threshold;
    const float t = past * p.inv_soft;
    const float v = p.soft ? 1.0f - ramp(t) : hard;                   // p.soft: wave-uniform
    return inside && m >= 0 ? v : 0.0f;
}

// two channels of one pixel: cur's dword c, the neighbours' dwords n[j] and weights w[j]; inv = 1 / W
template <int NB>
__device__ __forceinline__ uint32_t mean2(uint32_t c, const uint32_t (&n)[NB], const float (&w)[NB], float inv) {
    cvs::f32x2 acc = widen2(c);
#pragma unroll
    for (int j = 0; j < NB; j++) {
        const cvs::f32x2 t = w[j] * widen2(n[j]);
        const cvs::f32x2 s = acc + t;
        acc = w[j] > 0.0f ? s : acc;
    }
    const cvs::f32x2 o = acc * inv;
    return cvs::f2h_rz2(o.x, o.y);
}

template <int PIX>
__device__ __forceinline__ bool columns_inside(const cvk_view &v, int x) { return x >= v.fx0 && x + PIX - 1 <= v.fx1; }

template <int PIX, int NB>
__global__ __launch_bounds__(kLanes) void k_temporal_denoise(cvk_temporal_params p) {
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
    const int ch = p.channels;
    const ChannelMasks chm = { (ch & 1) ? 0x7FFFFFFFu : 0u, (ch & 2) ? 0x7FFFFFFFu : 0u, (ch & 4) ? 0x7FFFFFFFu : 0u, (ch & 8) ? 0x7FFFFFFFu : 0u };
    // the bits of a dword that selected channels own
    const uint32_t sel_lo = ((ch & 1) ? 0xFFFFu : 0u) | ((ch & 2) ? 0xFFFF0000u : 0u), sel_hi = ((ch & 4) ? 0xFFFFu : 0u) | ((ch & 8) ? 0xFFFF0000u : 0u);

    // the ring: cur's and each neighbour's row r - 1, and per neighbour H of rows r - 2 and r - 1, once row r has been taken in
    v4 cb = zero, nb[NB];
    int ha0[NB], ha1[NB], hb0[NB], hb1[NB];
#pragma unroll
    for (int j = 0; j < NB; j++) { nb[j] = zero; ha0[j] = ha1[j] = hb0[j] = hb1[j] = kNone; }
    // row r as loaded
    int r = y0 - 1;
    v4 lc = r >= cw.y0 && r <= cw.y1 && load_cur ? load_px<PIX>(p.cur, x, r) : zero, ln[NB];       // (row tests: wave-uniform)
#pragma unroll
    for (int j = 0; j < NB; j++) ln[j] = r >= p.v[j].y0 && r <= p.v[j].y1 && load_n[j] ? load_px<PIX>(p.n[j], x, r) : zero;

    for (; r <= y1 + 1; r++) {
        // the next row's loads, before this row's arithmetic
        const int q = r + 1;
        v4 nc = zero, nn[NB];
        if (q <= y1 + 1 && q >= cw.y0 && q <= cw.y1 && load_cur) nc = load_px<PIX>(p.cur, x, q);
#pragma unroll
        for (int j = 0; j < NB; j++) {
            nn[j] = zero;
            if (q <= y1 + 1 && q >= p.v[j].y0 && q <= p.v[j].y1 && load_n[j]) nn[j] = load_px<PIX>(p.n[j], x, q);
        }

        // per neighbour: D of the lane's columns in row r, H with the neighbouring lanes' columns, m of row y = r - 1
        const int y = r - 1;
        float w0[NB], w1[NB];
#pragma unroll
        for (int j = 0; j < NB; j++) {
            const bool row_n = r >= p.v[j].y0 && r <= p.v[j].y1;
            const int e0 = pixel_diff(lc.x, lc.y, ln[j].x, ln[j].y, chm);
            const int d0 = row_n && n0[j] ? e0 : kNone;
            int d1 = kNone;
            if (PIX == 2) {
                const int e1 = pixel_diff(lc.z, lc.w, ln[j].z, ln[j].w, chm);
                d1 = row_n && n1[j] ? e1 : kNone;
            }
            const int left = __shfl_up(PIX == 2 ? d1 : d0, 1), right = __shfl_down(d0, 1);
            int hc0, hc1 = kNone;
            if (PIX == 2) { hc0 = max3(left, d0, d1); hc1 = max3(d0, d1, right); }
            else hc0 = max3(left, d0, right);
            const bool row_y = y >= p.v[j].y0 && y <= p.v[j].y1;
            w0[j] = raw_weight(max3(ha0[j], hb0[j], hc0), row_y && n0[j], p);
            w1[j] = PIX == 2 ? raw_weight(max3(ha1[j], hb1[j], hc1), row_y && n1[j], p) : 0.0f;
            if (j >= 1) {                                                            // a far frame: capped by the nearer one
                const int near = p.near[j];                                          // wave-uniform; -1, 0 or 1
                const float k0 = near == 0 ? w0[0] : w0[j < 2 ? 0 : 1], k1 = near == 0 ? w1[0] : w1[j < 2 ? 0 : 1];
                w0[j] = near >= 0 ? fminf(w0[j], k0) : w0[j];
                w1[j] = near >= 0 ? fminf(w1[j], k1) : w1[j];
            }
            ha0[j] = hb0[j]; hb0[j] = hc0; ha1[j] = hb1[j]; hb1[j] = hc1;
        }

        // row y: cur's and the neighbours' pixels are one row back
        if (y >= y0) {
            float W0 = 1.0f, W1 = 1.0f;
            bool any0 = false, any1 = false;
            uint32_t t[NB];
#pragma unroll
            for (int j = 0; j < NB; j++) {
                const float s0 = W0 + w0[j], s1 = W1 + w1[j];
                W0 = w0[j] > 0.0f ? s0 : W0;
                W1 = w1[j] > 0.0f ? s1 : W1;
                any0 = any0 || w0[j] > 0.0f;
                any1 = any1 || w1[j] > 0.0f;
            }
            const float i0 = 1.0f / W0;
            v4 o = cb;
#pragma unroll
            for (int j = 0; j < NB; j++) t[j] = nb[j].x;
            const uint32_t lo0 = mean2<NB>(cb.x, t, w0, i0);
#pragma unroll
            for (int j = 0; j < NB; j++) t[j] = nb[j].y;
            const uint32_t hi0 = mean2<NB>(cb.y, t, w0, i0);
            o.x = any0 ? (lo0 & sel_lo) | (cb.x & ~sel_lo) : cb.x;
            o.y = any0 ? (hi0 & sel_hi) | (cb.y & ~sel_hi) : cb.y;
            if (PIX == 2) {
                const float i1 = 1.0f / W1;
#pragma unroll
                for (int j = 0; j < NB; j++) t[j] = nb[j].z;
                const uint32_t lo1 = mean2<NB>(cb.z, t, w1, i1);
#pragma unroll
                for (int j = 0; j < NB; j++) t[j] = nb[j].w;
                const uint32_t hi1 = mean2<NB>(cb.w, t, w1, i1);
                o.z = any1 ? (lo1 & sel_lo) | (cb.z & ~sel_lo) : cb.z;
                o.w = any1 ? (hi1 & sel_hi) | (cb.w & ~sel_hi) : cb.w;
            }
            store_px<PIX>(p.out, x, y, o, m0, m1);
        }
        cb = lc; lc = nc;
#pragma unroll
        for (int j = 0; j < NB; j++) { nb[j] = ln[j]; ln[j] = nn[j]; }
    }
}

template <int PIX, int NB>
void launch(const cvk_temporal_params &p, dim3 grid, hipStream_t stream) {
    hipLaunchKernelGGL((k_temporal_denoise<PIX, NB>), grid, dim3(kLanes), 0, stream, p);
}

template <int PIX>
void launch_n(const cvk_temporal_params &p, int neighbours, dim3 grid, hipStream_t stream) {
    switch (neighbours) {
    case 1: launch<PIX, 1>(p, grid, stream); break;
    case 2: launch<PIX, 2>(p, grid, stream); break;
    case 3: launch<PIX, 3>(p, grid, stream); break;
    default: launch<PIX, 4>(p, grid, stream); break;
    }
}

}  // namespace

extern "C" int cvk_temporal_denoise(const cvk_temporal_params *tp, int neighbours, int cus, void *stream) {
    cvk_temporal_params p = *tp;
    if (rect_empty(p.w)) return 0;
    if (neighbours < 1 || neighbours > 4) return (int)hipErrorInvalidValue;
    for (int j = 0; j < neighbours; j++)
        if (p.near[j] >= j || p.near[j] > 1 || p.near[j] < -1) return (int)hipErrorInvalidValue;
    const int xs2 = p.w.x0 - (int)(((long long)p.w.x0 - p.out.fx0) & 1);
    bool pairs = pair_view(p.out, xs2) && pair_view(p.cur, xs2);
    for (int j = 0; j < neighbours; j++) pairs = pairs && pair_view(p.n[j], xs2);
    const Shape s = shape(p.w, pairs, p.out.fx0, cus, kMade);
    p.xs = s.xs; p.seg = s.seg;
    hipStream_t st = (hipStream_t)stream;
    if (s.pix == 2) launch_n<2>(p, neighbours, s.grid, st); else launch_n<1>(p, neighbours, s.grid, st);
    return (int)hipGetLastError();
}
