// median_ops.hip -- VideoMedianFilter: a 3 x 3 or 5 x 5 median per channel on RGBA device frames (despeckle).
//
//   k_median<FMT, R>   FMT 0: rgba_f32, one pixel per lane; 1: rgba_f16, one pixel per lane; 2: rgba_f16, two per lane
// No reference code: the reference has no rank filter.  The contract is DESIGN.md "Median" and include/canvas_median.h,
// restated here.  With cw the source's current window, n = 2 R + 1, for a pixel (x, y) of the window written:
//     the neighbourhood is the n * n samples source(clamp(x + dx, cw.x0, cw.x1), clamp(y + dy, cw.y0, cw.y1)), |dx|, |dy| <= R
//     (replicated edges; the target's buffer plays no part); per channel they are ordered by a key of their BIT PATTERNS,
//     key(c) = c has its sign bit ? ~c : c | sign bit, compared unsigned: -NaN < -inf < .. < -0 < +0 < .. < +inf < +NaN, a
//     bijection; med[ch] is the sample whose key is the (n * n + 1) / 2-th smallest.
//     channels the mask does not select: source(x, y)'s codes.
//     threshold == 0: the selected channels take med's codes.
//     threshold > 0: d = the largest fabsf(s[ch] - med[ch]) over the SELECTED channels, one subtraction in f32 (halfs widened
//         exactly) rounded on its own; !(d <= threshold) (a NaN d included): all selected channels take med; else the pixel
//         keeps source(x, y) whole.  The decision is per pixel.
// Nothing is rounded: every output code is an input code.  A selection, not arithmetic, so there is one build of the unit (it
// is not in FMA_KERN) and both arithmetic flavours are the same instructions.
//
// Method: the codes become keys once, as they enter the ring; every compare-exchange of the fixed networks of median_net.hpp
// (19 for 9 values, 99 for 25) is one unsigned min and one unsigned max: on f16 frames on a whole dword, two channels at a time
// (v_pk_min_u16 / v_pk_max_u16 on g:r or a:b), on f32 frames v_min_u32 / v_max_u32 per channel.  No float min/max anywhere:
// theirs is not the contract's order.  The median's key is turned back into its code at the end.  A dword whose channels
// are all unselected runs no network and hands nothing between lanes (wave-uniform branch): an alpha-only despeckle of a
// matte works on a:b alone.
// Shape: the row stream of stream_common.hpp -- a one-wave workgroup walks down a segment of rows -- with a register ring of
// the n rows around the row being made.  A lane loads its own PIX columns of a row, at coordinates clamped to cw BEFORE the
// load (so no lane ever reads outside cw, the lanes beyond the window's edges included: they hold the edge column, which is
// the replicated edge their neighbours need), and takes the R columns left and right from the neighbouring lanes by
// __shfl_up / __shfl_down once per row, as the row enters the ring.  The outermost H lanes on each side (H = R with one pixel
// per lane, 1 with two) only load and hand on: kLanes - 2 H lanes make columns.  All lanes run the same instructions; no LDS,
// no barrier.  Row r + 1's loads are issued before row r is worked out.  Stores are non-temporal.
// Bound: 8 B read + 8 B written per f16 pixel (16 + 16 on f32); radius 2 is bound by the VALU (DESIGN.md has the counts).
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "pixel_math.hpp"
#include "stream_common.hpp"
#include "median_net.hpp"

namespace {

using namespace rowstream;

typedef unsigned short us2 __attribute__((ext_vector_type(2)));
typedef short ss2 __attribute__((ext_vector_type(2)));

// FMT 0: one 32-bit key per dword; else two 16-bit keys per dword
template <int FMT>
__device__ __forceinline__ uint32_t to_key(uint32_t c) {
    if (FMT == 0) return c ^ ((uint32_t)((int32_t)c >> 31) | 0x80000000u);
    const uint32_t neg = __builtin_bit_cast(uint32_t, __builtin_bit_cast(ss2, c) >> (short)15);
    return c ^ (neg | 0x80008000u);
}
template <int FMT>
__device__ __forceinline__ uint32_t from_key(uint32_t k) {
    if (FMT == 0) return k ^ (~(uint32_t)((int32_t)k >> 31) | 0x80000000u);
    const uint32_t pos = __builtin_bit_cast(uint32_t, __builtin_bit_cast(ss2, k) >> (short)15);
    return k ^ (~pos | 0x80008000u);
}
template <int FMT>
__device__ __forceinline__ uint32_t kmin(uint32_t a, uint32_t b) {
    if (FMT == 0) return min(a, b);
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(us2, a), __builtin_bit_cast(us2, b)));
}
template <int FMT>
__device__ __forceinline__ uint32_t kmax(uint32_t a, uint32_t b) {
    if (FMT == 0) return max(a, b);
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(us2, a), __builtin_bit_cast(us2, b)));
}

// the median of the n * n keys in v (clobbered)
template <int FMT, int R>
__device__ __forceinline__ uint32_t select(uint32_t (&v)[(2 * R + 1) * (2 * R + 1)]) {
#define CE(a, b) { const uint32_t lo = kmin<FMT>(v[a], v[b]); v[b] = kmax<FMT>(v[a], v[b]); v[a] = lo; }
    if (R == 1) { MEDIAN_NET_9(CE) } else { MEDIAN_NET_25(CE) }
#undef CE
    return v[((2 * R + 1) * (2 * R + 1)) / 2];
}

// |a - b| as a signed integer: its bits with the sign cleared (finite < +inf < NaN in that order)
__device__ __forceinline__ int adiff(float a, float b) {
    const float d = a - b;
    return (int)(__builtin_bit_cast(uint32_t, d) & 0x7FFFFFFFu);
}

template <int FMT> struct Row { uint32_t c[FMT == 2 ? 2 : 1][FMT == 0 ? 4 : 2]; };

// the lane's pixels of row y (inside cw) at the columns xa, xb (inside cw); pair: xb == xa + 1 and both are the lane's own
template <int FMT>
__device__ __forceinline__ Row<FMT> load_row(const cvk_view &v, int xa, bool pair, int y) {
    Row<FMT> r;
    const char *base = static_cast<const char *>(v.data);
    const long long at = (long long)(y - v.fy0) * v.pitch + (xa - v.fx0);
    if (FMT == 0) {
        const v4 t = *reinterpret_cast<const v4 *>(base + at * 16);
        r.c[0][0] = t.x; r.c[0][1] = t.y; r.c[0][2] = t.z; r.c[0][3] = t.w;
    } else if (FMT == 1) {
        const v2 t = *reinterpret_cast<const v2 *>(base + at * 8);
        r.c[0][0] = t.x; r.c[0][1] = t.y;
    } else {
        if (pair) {
            const v4 t = *reinterpret_cast<const v4 *>(base + at * 8);
            r.c[0][0] = t.x; r.c[0][1] = t.y; r.c[1][0] = t.z; r.c[1][1] = t.w;
        } else {                        // both columns clamp to one column of cw: the edge, replicated
            const v2 t = *reinterpret_cast<const v2 *>(base + at * 8);
            r.c[0][0] = t.x; r.c[0][1] = t.y; r.c[1][0] = t.x; r.c[1][1] = t.y;
        }
    }
    return r;
}

template <int FMT, int R>
__global__ __launch_bounds__(kLanes) void k_median(cvk_median_params p) {
    constexpr int PIX = FMT == 2 ? 2 : 1, W = FMT == 0 ? 4 : 2, N = 2 * R + 1, COLS = N + PIX - 1;
    constexpr int H = PIX == 2 ? 1 : R, MADE = kLanes - 2 * H;
    const cvk_rect w = p.w, cw = p.cw;
    const int lane = (int)threadIdx.x;
    const int x = p.xs + PIX * ((int)blockIdx.x * MADE + lane - H);
    const bool made = lane >= H && lane < kLanes - H;
    const bool m0 = made && x >= w.x0 && x <= w.x1, m1 = PIX == 2 && made && x + 1 >= w.x0 && x + 1 <= w.x1;
    const int y0 = w.y0 + (int)blockIdx.y * p.seg, y1 = min(y0 + p.seg - 1, w.y1);
    // the columns loaded: the lane's own, clamped to cw
    const int xa = min(max(x, cw.x0), cw.x1), xb = min(max(x + 1, cw.x0), cw.x1);
    const bool pair = PIX == 2 && xa == x && xb == x + 1;          // (otherwise xa == xb: at most one of the two lies inside)
    // which channels of dword k are filtered (wave-uniform)
    uint32_t chm[W];
#pragma unroll
    for (int k = 0; k < W; k++) {
        if (FMT == 0) chm[k] = (p.channels >> k) & 1 ? 0xFFFFFFFFu : 0u;
        else chm[k] = ((p.channels >> (2 * k)) & 1 ? 0x0000FFFFu : 0u) | ((p.channels >> (2 * k + 1)) & 1 ? 0xFFFF0000u : 0u);
    }
    const int gate = (int)__builtin_bit_cast(uint32_t, p.threshold);      // a finite threshold > 0 as its bits: ordered as ints

    // ring[j][c]: the keys of column x - R + c in row y - R + j, rows and columns clamped to cw
    uint32_t ring[N][COLS][W];
#pragma unroll
    for (int j = 0; j < N; j++)
#pragma unroll
        for (int c = 0; c < COLS; c++)
#pragma unroll
            for (int k = 0; k < W; k++) ring[j][c][k] = 0u;

    Row<FMT> next = load_row<FMT>(p.in, xa, pair, min(max(y0 - R, cw.y0), cw.y1));
    for (int q = y0 - R; q <= y1 + R; q++) {
        const Row<FMT> row = next;
        if (q < y1 + R) next = load_row<FMT>(p.in, xa, pair, min(max(q + 1, cw.y0), cw.y1));       // wave-uniform

        // row q enters the ring: its keys, and the neighbouring lanes' columns of the filtered dwords
#pragma unroll
        for (int j = 0; j + 1 < N; j++)
#pragma unroll
            for (int c = 0; c < COLS; c++)
#pragma unroll
                for (int k = 0; k < W; k++) ring[j][c][k] = ring[j + 1][c][k];
#pragma unroll
        for (int k = 0; k < W; k++) {
            uint32_t own[PIX];
#pragma unroll
            for (int i = 0; i < PIX; i++) own[i] = to_key<FMT>(row.c[i][k]);
#pragma unroll
            for (int i = 0; i < PIX; i++) ring[N - 1][R + i][k] = own[i];
            if (chm[k]) {
#pragma unroll
                for (int c = 0; c < COLS; c++) {
                    const int o = c - R;                                   // the column's offset from x
                    if (o >= 0 && o < PIX) continue;
                    const int i = ((o % PIX) + PIX) % PIX, d = (o - i) / PIX;       // pixel i of the lane d to the right
                    ring[N - 1][c][k] = d < 0 ? __shfl_up(own[i], (unsigned)(-d)) : __shfl_down(own[i], (unsigned)d);
                }
            }
        }

        const int y = q - R;
        if (y < y0) continue;
        // row y has its n rows in the ring
        uint32_t out[PIX][W];
#pragma unroll
        for (int i = 0; i < PIX; i++) {
            uint32_t src[W], med[W];
            bool beyond = !p.gated;
#pragma unroll
            for (int k = 0; k < W; k++) {
                src[k] = from_key<FMT>(ring[R][R + i][k]);
                med[k] = src[k];
                if (chm[k]) {
                    uint32_t v[N * N];
#pragma unroll
                    for (int j = 0; j < N; j++)
#pragma unroll
                        for (int c = 0; c < N; c++) v[j * N + c] = ring[j][i + c][k];
                    med[k] = from_key<FMT>(select<FMT, R>(v));
                    if (p.gated) {
                        if (FMT == 0) beyond = beyond || adiff(__uint_as_float(src[k]), __uint_as_float(med[k])) > gate;
                        else {
                            const bool lo = adiff(cvs::h2f(src[k] & 0xFFFFu), cvs::h2f(med[k] & 0xFFFFu)) > gate;
                            const bool hi = adiff(cvs::h2f(src[k] >> 16), cvs::h2f(med[k] >> 16)) > gate;
                            beyond = beyond || ((chm[k] & 0xFFFFu) && lo) || ((chm[k] >> 16) && hi);
                        }
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < W; k++) out[i][k] = beyond ? (med[k] & chm[k]) | (src[k] & ~chm[k]) : src[k];
        }
        if (FMT == 0) {
            char *t = static_cast<char *>(p.out.data) + ((long long)(y - p.out.fy0) * p.out.pitch + (x - p.out.fx0)) * 16;
            if (m0) __builtin_nontemporal_store(v4{ out[0][0], out[0][1], out[0][W - 2], out[0][W - 1] }, reinterpret_cast<v4 *>(t));
        } else {
            const v4 o = { out[0][0], out[0][1], out[PIX - 1][0], out[PIX - 1][1] };
            store_px<PIX>(p.out, x, y, o, m0, m1);
        }
    }
}

template <int FMT>
void launch(const cvk_median_params &p, dim3 grid, hipStream_t st) {
    if (p.radius == 1) hipLaunchKernelGGL((k_median<FMT, 1>), grid, dim3(kLanes), 0, st, p);
    else hipLaunchKernelGGL((k_median<FMT, 2>), grid, dim3(kLanes), 0, st, p);
}

}  // namespace

extern "C" int cvk_median(const cvk_median_params *mp, int half, int cus, void *stream) {
    cvk_median_params p = *mp;
    if (rect_empty(p.w)) return 0;
    if (p.radius != 1 && p.radius != 2) return (int)hipErrorInvalidValue;
    const int xs2 = p.w.x0 - (int)(((long long)p.w.x0 - p.out.fx0) & 1);
    const bool pairs = half && pair_view(p.out, xs2) && pair_view(p.in, xs2);
    const Shape s = shape(p.w, pairs, p.out.fx0, cus, kLanes - 2 * (pairs ? 1 : p.radius));
    p.xs = s.xs; p.seg = s.seg;
    hipStream_t st = (hipStream_t)stream;
    if (!half) launch<0>(p, s.grid, st);
    else if (s.pix == 2) launch<2>(p, s.grid, st);
    else launch<1>(p, s.grid, st);
    return (int)hipGetLastError();
}
