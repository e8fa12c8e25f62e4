// lut3d_ops.hip -- VideoLut3DFilter: a 3D colour lookup table applied by tetrahedral interpolation on un-premultiplied RGBA
// device frames.
//
// No reference code (the reference has no colour tool beyond gain/offset and the 3x3 matrix).  The contract is DESIGN.md
// "3D LUT", restated here.  Lattice L: n^3 nodes of 4 floats (R, G, B, unused) on a 16-byte boundary, red fastest: the node of
// lattice index (ir, ig, ib) is at ir + n*(ig + n*ib).  The host (host/lut3d.c) hands over n, dmin[c] and
// scale[c] = (float)(n-1) / (domain_max[c] - domain_min[c]).  Per pixel s of the window, in f32 (a half widened exactly):
//     for c in r, g, b:
//         t   = (s.c - dmin[c]) * scale[c]
//         t   = (t > 0) ? ((t < (float)(n-1)) ? t : (float)(n-1)) : 0          NaN -> 0, -Inf -> 0, +Inf -> n-1
//         i_c = min((int)t, n-2) ;  f_c = t - (float)i_c                       0 <= f_c <= 1
//     order the channels by descending f; a tie goes to r before g, and g before b (a stable sort on (-f, channel))
//         -> axes e1, e2, e3 with f1 >= f2 >= f3
//     V0 = L[i] ; V1 = L[i + e1] ; V2 = L[i + e1 + e2] ; V3 = L[i + (1,1,1)]
//     w0 = 1 - f1 ; w1 = f1 - f2 ; w2 = f2 - f3 ; w3 = f3
//     out.c = ((V0.c*w0 + V1.c*w1) + V2.c*w2) + V3.c*w3                        for c in r, g, b
//     out.a = s.a, code for code (NaN included)                                f16 targets truncated once at the store
// Every operation is rounded on its own in BOTH arithmetic flavours (the stance of key_ops.hip and matte_ops.hip), so there is
// one build of the unit: it is not in FMA_KERN.
//
// The vertex order as selects.  With rg = fr >= fg, rb = fr >= fb, gb = fg >= fb (a tie is "before"), r is first when rg && rb,
// g when !rg && gb, else b; r is last when !rg && !rb, g when rg && !gb, else b.  V1 is one step along the first axis and V2
// is V3 less one step along the last, so two three-way selects of the node strides (1, n, n*n) give both offsets; f1, f2, f3
// are the maximum, the median and the minimum of three finite numbers, whatever the order of equals.
//
// Bound: HBM for the pixel stream (8 + 8 B / px on f16 frames, 16 + 16 on f32) beside four data-dependent 16-byte vertex loads
// per pixel.  The lattice is 16*n^3 bytes: 79 KB at n = 17, 575 KB at 33, 4.4 MB at 65.  Neighbouring pixels of a picture share
// or neighbour their cells, so most vertex loads of a wave hit the same few lines; noise is the worst case.
// Two kernels, the same lanes, columns, row segments and arithmetic in both (walk()):
//   n > 17   k_lut3d: key_ops.hip's shape (stream_common.hpp) -- a one-wave workgroup owns 64 lanes x PIX columns over a segment
//            of consecutive rows; the lattice is read through the caches.
//   n <= 17  k_lut3d_lds: the lattice staged in LDS (78,608 of the 160 KiB at n = 17) by persistent workgroups of eight waves
//            that walk the blocks of the first kernel's grid.  Measured on 4K noise at n = 17: 29 us against 98 (f16) and 51
//            against 143 (f32), 29 against 39 and 51 against 52 on a ramp or a flat frame (DESIGN.md "3D LUT", Measured).
// One 16-byte access per lane and row: an f32 pixel, or two half pixels where base, pitch and window parity of both frames
// allow (pair_view), else one half pixel in 8 bytes.  The next row's pixel load is issued before the current row is worked out,
// and the vertex loads of a row (four, eight on the pair path) are all issued before the first is used.  Stores are
// non-temporal.  In place (target = source frame) needs nothing special: a lane reads the pixels it writes, each before it
// writes it, and no other lane touches them.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "pixel_math.hpp"
#include "stream_common.hpp"

namespace {

using namespace rowstream;

typedef float f4 __attribute__((ext_vector_type(4)));

// where a pixel's colour falls in the lattice: the four node indices and the four weights
struct Cell { int v0, v1, v2, v3; float w0, w1, w2, w3; };

struct Axis { int i; float f; };

__device__ __forceinline__ Axis axis_of(float s, float dmin, float scale, float nm1, int n) {
    float t = (s - dmin) * scale;
    t = (t > 0.0f) ? ((t < nm1) ? t : nm1) : 0.0f;
    Axis a;
    a.i = min((int)t, n - 2);
    a.f = t - (float)a.i;
    return a;
}

__device__ __forceinline__ Cell cell_of(const cvk_lut3d_params &lp, float r, float g, float b) {
    const int n = lp.n, nn = n * n;                                            // wave-uniform
    const float nm1 = (float)(n - 1);
    const Axis ar = axis_of(r, lp.dmin[0], lp.scale[0], nm1, n), ag = axis_of(g, lp.dmin[1], lp.scale[1], nm1, n), ab = axis_of(b, lp.dmin[2], lp.scale[2], nm1, n);
    const bool rg = ar.f >= ag.f, rb = ar.f >= ab.f, gb = ag.f >= ab.f;
    const int first = (rg && rb) ? 1 : ((!rg && gb) ? n : nn);
    const int last = (!rg && !rb) ? 1 : ((rg && !gb) ? n : nn);
    const float f1 = fmaxf(fmaxf(ar.f, ag.f), ab.f), f3 = fminf(fminf(ar.f, ag.f), ab.f), f2 = __builtin_amdgcn_fmed3f(ar.f, ag.f, ab.f);
    Cell c;
    c.v0 = ar.i + n * (ag.i + n * ab.i);
    c.v1 = c.v0 + first;
    c.v3 = c.v0 + (1 + n + nn);
    c.v2 = c.v3 - last;
    c.w0 = 1.0f - f1; c.w1 = f1 - f2; c.w2 = f2 - f3; c.w3 = f3;
    return c;
}

struct Verts { f4 a, b, c, d; };

template <class L>
__device__ __forceinline__ Verts fetch(L lattice, const Cell &c) {
    return Verts{ lattice[c.v0], lattice[c.v1], lattice[c.v2], lattice[c.v3] };
}

__device__ __forceinline__ float blend(float a, float b, float c, float d, const Cell &k) {
    return ((a * k.w0 + b * k.w1) + c * k.w2) + d * k.w3;
}

// HALF: 0 = rgba_f32 frames, one pixel per lane; 1 = rgba_f16, one pixel per lane; 2 = rgba_f16, two pixels per lane
template <int HALF>
__device__ __forceinline__ v4 load_row(const cvk_view &v, int x, int y) {
    if (HALF) return load_px<HALF>(v, x, y);
    return *reinterpret_cast<const v4 *>(static_cast<const char *>(v.data) + ((long long)(y - v.fy0) * v.pitch + (x - v.fx0)) * 16);
}

// one half pixel as its two dwords (lo = g:r, hi = a:b)
__device__ __forceinline__ Cell cell_f16(const cvk_lut3d_params &lp, uint32_t lo, uint32_t hi) {
    return cell_of(lp, cvs::h2f(lo & 0xFFFFu), cvs::h2f(lo >> 16), cvs::h2f(hi & 0xFFFFu));
}
__device__ __forceinline__ v2 out_f16(const Cell &k, const Verts &q, uint32_t hi) {
    const float r = blend(q.a.x, q.b.x, q.c.x, q.d.x, k), g = blend(q.a.y, q.b.y, q.c.y, q.d.y, k), b = blend(q.a.z, q.b.z, q.c.z, q.d.z, k);
    return v2{ cvs::f2h_rz2(r, g), cvs::f2h_rz(b) | (hi & 0xFFFF0000u) };
}

// the rows y0 .. y1 of one lane's columns; L: the lattice in global memory (const f4 *) or staged in LDS (f4 *)
template <int HALF, class L>
__device__ __forceinline__ void walk(const cvk_lut3d_params &lp, L lattice, const cvk_view &out, const cvk_view &in, int x, bool m0, bool m1, int y0, int y1) {
    constexpr int PIX = HALF == 2 ? 2 : 1;
    v4 cur = load_row<HALF>(in, x, y0);
    for (int y = y0; y <= y1; y++) {
        v4 next = cur;
        if (y < y1) next = load_row<HALF>(in, x, y + 1);                // wave-uniform
        if (HALF) {
            // A pair cut by the window's edge holds a pixel outside the window; it lies inside the buffer's row, its colour
            // is clamped into the lattice like any other, and its result is not stored.
            const Cell k0 = cell_f16(lp, cur.x, cur.y);
            const Verts q0 = fetch(lattice, k0);
            if (PIX == 2) {
                const Cell k1 = cell_f16(lp, cur.z, cur.w);
                const Verts q1 = fetch(lattice, k1);
                const v2 p0 = out_f16(k0, q0, cur.y), p1 = out_f16(k1, q1, cur.w);
                store_px<PIX>(out, x, y, v4{ p0.x, p0.y, p1.x, p1.y }, m0, m1);
            } else {
                const v2 p0 = out_f16(k0, q0, cur.y);
                store_px<PIX>(out, x, y, v4{ p0.x, p0.y, 0u, 0u }, m0, m1);
            }
        } else {
            const Cell k = cell_of(lp, __uint_as_float(cur.x), __uint_as_float(cur.y), __uint_as_float(cur.z));
            const Verts q = fetch(lattice, k);
            const v4 c = { __float_as_uint(blend(q.a.x, q.b.x, q.c.x, q.d.x, k)), __float_as_uint(blend(q.a.y, q.b.y, q.c.y, q.d.y, k)),
                           __float_as_uint(blend(q.a.z, q.b.z, q.c.z, q.d.z, k)), cur.w };
            char *p = static_cast<char *>(out.data) + ((long long)(y - out.fy0) * out.pitch + (x - out.fx0)) * 16;
            __builtin_nontemporal_store(c, reinterpret_cast<v4 *>(p));
        }
        cur = next;
    }
}

// n > kLdsMaxN: one-wave workgroups, the lattice through the caches
template <int HALF>
__global__ __launch_bounds__(kLanes) void k_lut3d(cvk_lut3d_params lp, cvk_view out, cvk_view in, cvk_rect w, int xs, int seg) {
    constexpr int PIX = HALF == 2 ? 2 : 1;
    ROWSTREAM_LANE(w, xs, seg)
    walk<HALF>(lp, reinterpret_cast<const f4 *>(lp.lattice), out, in, x, m0, m1, y0, y1);
}

// n <= kLdsMaxN: the whole lattice (at most 17^3 nodes, 78,608 bytes of the 160 KiB) staged in LDS by persistent workgroups of
// eight waves; wave v of workgroup g then takes the one-wave blocks g*8 + v, + 8*gridDim.x, ... of the grid k_lut3d would have
// run (chunks x segs, the same lanes, columns and row segments).  Two workgroups fit a CU: 16 waves, as rowstream::shape sizes it.
constexpr int kLdsMaxN = 17, kLdsNodes = kLdsMaxN * kLdsMaxN * kLdsMaxN, kLdsWaves = 8;

template <int HALF>
__global__ __launch_bounds__(kLanes * kLdsWaves) void k_lut3d_lds(cvk_lut3d_params lp, cvk_view out, cvk_view in, cvk_rect w, int xs, int seg, int chunks, int segs) {
    constexpr int PIX = HALF == 2 ? 2 : 1;
    __shared__ f4 lattice[kLdsNodes];
    {
        const f4 *__restrict__ g = reinterpret_cast<const f4 *>(lp.lattice);
        const int nodes = lp.n * lp.n * lp.n;                            // <= kLdsNodes: the launcher looked
        for (int k = (int)threadIdx.x; k < nodes; k += kLanes * kLdsWaves) lattice[k] = g[k];
    }
    __syncthreads();
    const int lane = (int)threadIdx.x & (kLanes - 1), wave = (int)threadIdx.x / kLanes;
    const int blocks = chunks * segs;                                    // < 2^30: the launcher looked
    for (int b = (int)blockIdx.x * kLdsWaves + wave; b < blocks; b += (int)gridDim.x * kLdsWaves) {
        const int bx = b % chunks, by = b / chunks;
        const int x = xs + PIX * (bx * kLanes + lane);
        const bool m0 = x >= w.x0 && x <= w.x1, m1 = PIX == 2 && x + 1 >= w.x0 && x + 1 <= w.x1;
        if (!m0 && !m1) continue;
        const int y0 = w.y0 + by * seg, y1 = min(y0 + seg - 1, w.y1);
        walk<HALF>(lp, lattice, out, in, x, m0, m1, y0, y1);
    }
}

template <int HALF>
int launch(const cvk_lut3d_params &lp, const cvk_view &out, const cvk_view &in, const cvk_rect &w, const Shape &s, int cus, hipStream_t st) {
    const long long blocks = (long long)s.grid.x * s.grid.y;
    if (lp.n <= kLdsMaxN && blocks < (1ll << 30)) {
        const long long most = 2ll * (cus > 0 ? cus : 256), need = (blocks + kLdsWaves - 1) / kLdsWaves;
        hipLaunchKernelGGL((k_lut3d_lds<HALF>), dim3((unsigned)(need < most ? need : most)), dim3(kLanes * kLdsWaves), 0, st, lp, out, in, w, s.xs, s.seg,
                           (int)s.grid.x, (int)s.grid.y);
    } else {
        hipLaunchKernelGGL((k_lut3d<HALF>), s.grid, dim3(kLanes), 0, st, lp, out, in, w, s.xs, s.seg);
    }
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int cvk_lut3d(const cvk_lut3d_params *lp, cvk_view out, cvk_view in, cvk_rect w, int half, int cus, void *stream) {
    if (rect_empty(w)) return 0;
    const int xs2 = w.x0 - (int)(((long long)w.x0 - out.fx0) & 1);
    const Shape s = shape(w, half && pair_view(out, xs2) && pair_view(in, xs2), out.fx0, cus);
    if (!half) return launch<0>(*lp, out, in, w, s, cus, (hipStream_t)stream);
    return s.pix == 2 ? launch<2>(*lp, out, in, w, s, cus, (hipStream_t)stream) : launch<1>(*lp, out, in, w, s, cus, (hipStream_t)stream);
}
