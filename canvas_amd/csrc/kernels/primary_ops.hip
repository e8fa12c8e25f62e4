// primary_ops.hip -- VideoColorCorrectFilter: per-channel 1D curves, a 3 x 4 matrix and per-channel 1D curves again, fused into one
// pass over un-premultiplied RGBA device frames.
//
// No reference code (the reference has no colour tool beyond gain/offset and the 3x3 matrix).  The contract is DESIGN.md
// "Primary colour correction", restated here.  A curve set T: three tables of K floats, planar (R | G | B), on a 16-byte boundary.
// The host (host/primary.c) hands over K, dmin[c] and scale[c] = (float)(K-1) / (domain_max[c] - domain_min[c]) per present set.
// Per pixel s of the window, in f32 (a half widened exactly):
//     curve(T, c, s):  t = (s - dmin[c]) * scale[c]
//                      t = (t > 0) ? ((t < (float)(K-1)) ? t : (float)(K-1)) : 0       NaN -> 0, -Inf -> 0, +Inf -> K-1
//                      i = min((int)t, K-2) ;  f = t - (float)i
//                      return T[c][i] * (1 - f) + T[c][i+1] * f
//     v = s.rgb ;  pre: v.c = curve(pre, c, v.c) ;  matrix: v.c = ((m[4c]*v.r + m[4c+1]*v.g) + m[4c+2]*v.b) + m[4c+3], from the
//     three values before the stage ;  post: v.c = curve(post, c, v.c) ;  out.rgb = v ;  out.a = s.a, code for code
// Every operation is rounded on its own in BOTH arithmetic flavours (the stance of lut3d_ops.hip), so there is one build of the
// unit: it is not in FMA_KERN.  f16 targets are truncated once at the store.
//
// Shape: k_lut3d_lds's.  Persistent workgroups stage the present tables into LDS once -- 12 * (Kpre + Kpost) bytes, 98 328 of the
// 160 KiB at the most, so every legal call fits and there is no path through the caches -- and their waves then walk the one-wave
// blocks of the row stream's grid (stream_common.hpp: 64 lanes x PIX columns over a segment of consecutive rows).  Which stages
// are present is a template parameter: an absent stage has no LDS, no staging loop and no instruction.  Two workgroups of eight
// waves per CU where two copies of the tables fit the CU's LDS (up to 81 920 bytes each), else one of sixteen: sixteen waves a CU
// either way, as rowstream::shape sizes its segments.  One 16-byte access per lane and row: an f32 pixel, or two half pixels
// where base, pitch and window parity of both frames allow (pair_view), else one half pixel in 8 bytes.  The next row's pixel load
// is issued before the current row is worked out.  Stores are non-temporal.  In place needs nothing special: a lane reads the
// pixels it writes, each before it writes it, and no other lane touches them.
//
// The gathers.  The three channels of a pixel have three different indices, so an interleaved (r, g, b per node) table would
// fetch three nodes to use a third of each; planar tables are kept.  A lane reads T[i] and T[i+1], neighbours of any parity: two
// 4-byte reads (one ds_read2_b32), 32 banks of 4 bytes, lanes in two groups of 32.  On a smooth picture neighbouring lanes hit
// the same or neighbouring nodes (broadcast, or neighbouring banks); on noise 32 lanes fall on 32 banks at random and the fullest
// bank holds 3 to 4 of them.  Pairs (T[i], T[i+1]) stored as aligned 8-byte entries would halve the instruction's cycles and
// spread a group over 64 banks, at twice the LDS: six tables of 4096 pairs are 196 608 bytes, more than the CU has, so the form
// was rejected on that arithmetic before any timing.  DESIGN.md "Primary colour correction" has what was measured.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "pixel_math.hpp"
#include "stream_common.hpp"

namespace {

using namespace rowstream;

typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int kWavesTwo = 8, kWavesOne = 16;               // waves of a workgroup where two / one workgroup runs on a CU
constexpr unsigned kLdsCu = 160u << 10;

__device__ __forceinline__ float curve(const float *t, int k, float dmin, float scale, float s) {
    const float km1 = (float)(k - 1);                                    // wave-uniform
    float u = (s - dmin) * scale;
    u = (u > 0.0f) ? ((u < km1) ? u : km1) : 0.0f;
    const int i = min((int)u, k - 2);
    const float f = u - (float)i;
    return t[i] * (1.0f - f) + t[i + 1] * f;
}

struct Rgb { float r, g, b; };

// pre / post: the staged tables in LDS
template <bool PRE, bool MAT, bool POST>
__device__ __forceinline__ Rgb grade(const cvk_primary_params &pp, const float *pre, const float *post, Rgb v) {
    if (PRE) {
        v.r = curve(pre, pp.kpre, pp.pre_min[0], pp.pre_scale[0], v.r);
        v.g = curve(pre + pp.kpre, pp.kpre, pp.pre_min[1], pp.pre_scale[1], v.g);
        v.b = curve(pre + 2 * pp.kpre, pp.kpre, pp.pre_min[2], pp.pre_scale[2], v.b);
    }
    if (MAT) {
        const float *m = pp.m;
        const float r = ((m[0] * v.r + m[1] * v.g) + m[2] * v.b) + m[3];
        const float g = ((m[4] * v.r + m[5] * v.g) + m[6] * v.b) + m[7];
        const float b = ((m[8] * v.r + m[9] * v.g) + m[10] * v.b) + m[11];
        v = Rgb{ r, g, b };
    }
    if (POST) {
        v.r = curve(post, pp.kpost, pp.post_min[0], pp.post_scale[0], v.r);
        v.g = curve(post + pp.kpost, pp.kpost, pp.post_min[1], pp.post_scale[1], v.g);
        v.b = curve(post + 2 * pp.kpost, pp.kpost, pp.post_min[2], pp.post_scale[2], v.b);
    }
    return v;
}

// HALF: 0 = rgba_f32 frames, one pixel per lane; 1 = rgba_f16, one pixel per lane; 2 = rgba_f16, two pixels per lane
template <int HALF>
__device__ __forceinline__ v4 load_row(const cvk_view &v, int x, int y) {
    if (HALF) return load_px<HALF>(v, x, y);
    return *reinterpret_cast<const v4 *>(static_cast<const char *>(v.data) + ((long long)(y - v.fy0) * v.pitch + (x - v.fx0)) * 16);
}

// one half pixel as its two dwords (lo = g:r, hi = a:b)
template <bool PRE, bool MAT, bool POST>
__device__ __forceinline__ v2 grade_f16(const cvk_primary_params &pp, const float *pre, const float *post, uint32_t lo, uint32_t hi) {
    const Rgb c = grade<PRE, MAT, POST>(pp, pre, post, Rgb{ cvs::h2f(lo & 0xFFFFu), cvs::h2f(lo >> 16), cvs::h2f(hi & 0xFFFFu) });
    return v2{ cvs::f2h_rz2(c.r, c.g), cvs::f2h_rz(c.b) | (hi & 0xFFFF0000u) };
}

// the rows y0 .. y1 of one lane's columns
template <int HALF, bool PRE, bool MAT, bool POST>
__device__ __forceinline__ void walk(const cvk_primary_params &pp, const float *pre, const float *post, const cvk_view &out, const cvk_view &in, int x, bool m0, bool m1,
                                     int y0, int y1) {
    constexpr int PIX = HALF == 2 ? 2 : 1;
    v4 cur = load_row<HALF>(in, x, y0);
    for (int y = y0; y <= y1; y++) {
        v4 next = cur;
        if (y < y1) next = load_row<HALF>(in, x, y + 1);                // wave-uniform
        if (HALF) {
            // A pair cut by the window's edge holds a pixel outside the window; it lies inside the buffer's row, its colour is
            // clamped into the tables like any other, and its result is not stored.
            const v2 p0 = grade_f16<PRE, MAT, POST>(pp, pre, post, cur.x, cur.y);
            if (PIX == 2) {
                const v2 p1 = grade_f16<PRE, MAT, POST>(pp, pre, post, cur.z, cur.w);
                store_px<PIX>(out, x, y, v4{ p0.x, p0.y, p1.x, p1.y }, m0, m1);
            } else {
                store_px<PIX>(out, x, y, v4{ p0.x, p0.y, 0u, 0u }, m0, m1);
            }
        } else {
            const Rgb c = grade<PRE, MAT, POST>(pp, pre, post, Rgb{ __uint_as_float(cur.x), __uint_as_float(cur.y), __uint_as_float(cur.z) });
            const v4 o = { __float_as_uint(c.r), __float_as_uint(c.g), __float_as_uint(c.b), cur.w };
            char *p = static_cast<char *>(out.data) + ((long long)(y - out.fy0) * out.pitch + (x - out.fx0)) * 16;
            __builtin_nontemporal_store(o, reinterpret_cast<v4 *>(p));
        }
        cur = next;
    }
}

// `count` floats from a 16-byte aligned device table into LDS at any 4-byte offset: 16-byte loads, the tail float by float
__device__ __forceinline__ void stage(float *lds, const float *__restrict__ table, int count) {
    const f4 *__restrict__ g = reinterpret_cast<const f4 *>(table);
    const int quads = count >> 2;
    for (int k = (int)threadIdx.x; k < quads; k += (int)blockDim.x) {
        const f4 q = g[k];
        lds[4 * k + 0] = q.x; lds[4 * k + 1] = q.y; lds[4 * k + 2] = q.z; lds[4 * k + 3] = q.w;
    }
    for (int k = 4 * quads + (int)threadIdx.x; k < count; k += (int)blockDim.x) lds[k] = table[k];
}

// Wave v of workgroup g takes the one-wave blocks g*W + v, + W*gridDim.x, ... of the grid chunks x segs (W waves a workgroup).
template <int HALF, bool PRE, bool MAT, bool POST>
__global__ __launch_bounds__(kLanes * kWavesOne) void k_primary(cvk_primary_params pp, cvk_view out, cvk_view in, cvk_rect w, int xs, int seg, int chunks, int segs) {
    constexpr int PIX = HALF == 2 ? 2 : 1;
    extern __shared__ __align__(16) float lds[];
    float *pre = lds, *post = lds + (PRE ? 3 * pp.kpre : 0);
    if (PRE) stage(pre, pp.pre, 3 * pp.kpre);
    if (POST) stage(post, pp.post, 3 * pp.kpost);
    if (PRE || POST) __syncthreads();
    const int lane = (int)threadIdx.x & (kLanes - 1), wave = (int)threadIdx.x / kLanes, waves = (int)blockDim.x / kLanes;
    const long long blocks = (long long)chunks * segs;
    for (long long b = (long long)blockIdx.x * waves + wave; b < blocks; b += (long long)gridDim.x * waves) {
        const int bx = (int)(b % chunks), by = (int)(b / chunks);
        const int x = xs + PIX * (bx * kLanes + lane);
        const bool m0 = x >= w.x0 && x <= w.x1, m1 = PIX == 2 && x + 1 >= w.x0 && x + 1 <= w.x1;
        if (!m0 && !m1) continue;
        const int y0 = w.y0 + by * seg, y1 = min(y0 + seg - 1, w.y1);
        walk<HALF, PRE, MAT, POST>(pp, pre, post, out, in, x, m0, m1, y0, y1);
    }
}

template <int HALF, bool PRE, bool MAT, bool POST>
int launch(const cvk_primary_params &pp, const cvk_view &out, const cvk_view &in, const cvk_rect &w, const Shape &s, int cus, hipStream_t st) {
    const size_t bytes = (size_t)12 * (size_t)((PRE ? pp.kpre : 0) + (POST ? pp.kpost : 0));
    // more dynamic LDS than a launch may ask for by default (the CU has 160 KiB): the instance is told first
    if (bytes > (48u << 10)) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_primary<HALF, PRE, MAT, POST>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsCu);
        if (e != hipSuccess) return (int)e;
    }
    const bool two = 2 * bytes <= kLdsCu;
    const int waves = two ? kWavesTwo : kWavesOne;
    const long long blocks = (long long)s.grid.x * s.grid.y;
    const long long most = (two ? 2ll : 1ll) * (cus > 0 ? cus : 256), need = (blocks + waves - 1) / waves;
    hipLaunchKernelGGL((k_primary<HALF, PRE, MAT, POST>), dim3((unsigned)(need < most ? need : most)), dim3(kLanes * waves), bytes, st, pp, out, in, w, s.xs, s.seg,
                       (int)s.grid.x, (int)s.grid.y);
    return (int)hipGetLastError();
}

template <int HALF>
int pick(const cvk_primary_params &pp, const cvk_view &out, const cvk_view &in, const cvk_rect &w, const Shape &s, int cus, hipStream_t st) {
    switch ((pp.kpre ? 4 : 0) | (pp.matrix ? 2 : 0) | (pp.kpost ? 1 : 0)) {
    case 1: return launch<HALF, false, false, true>(pp, out, in, w, s, cus, st);
    case 2: return launch<HALF, false, true, false>(pp, out, in, w, s, cus, st);
    case 3: return launch<HALF, false, true, true>(pp, out, in, w, s, cus, st);
    case 4: return launch<HALF, true, false, false>(pp, out, in, w, s, cus, st);
    case 5: return launch<HALF, true, false, true>(pp, out, in, w, s, cus, st);
    case 6: return launch<HALF, true, true, false>(pp, out, in, w, s, cus, st);
    case 7: return launch<HALF, true, true, true>(pp, out, in, w, s, cus, st);
    }
    return (int)hipErrorInvalidValue;                                   // no stage: host/primary.c has refused it
}

}  // namespace

extern "C" int cvk_primary(const cvk_primary_params *pp, cvk_view out, cvk_view in, cvk_rect w, int half, int cus, void *stream) {
    if (rect_empty(w)) return 0;
    const int xs2 = w.x0 - (int)(((long long)w.x0 - out.fx0) & 1);
    const Shape s = shape(w, half && pair_view(out, xs2) && pair_view(in, xs2), out.fx0, cus);
    if (!half) return pick<0>(*pp, out, in, w, s, cus, (hipStream_t)stream);
    return s.pix == 2 ? pick<2>(*pp, out, in, w, s, cus, (hipStream_t)stream) : pick<1>(*pp, out, in, w, s, cus, (hipStream_t)stream);
}
