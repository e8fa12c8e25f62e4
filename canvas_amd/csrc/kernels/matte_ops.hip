// matte_ops.hip -- VideoMatteFilter: clip, choke and feather of the alpha channel of un-premultiplied RGBA device frames, fused.
//
// No reference code; the contract is DESIGN.md "Matte refine", restated here.  S = the source's current window, `w` the window
// written (S clipped to the target's buffer).  The host (host/matte.c) hands over black and inv = 1 / (white - black) (read only
// where `levels` says the stage is on), r = |choke| and whether the matte grows, the taps and c = (ntaps - 1) / 2.  In f32 (a half
// widened exactly), every operation rounded on its own in BOTH arithmetic flavours (one build of the unit: not in FMA_KERN):
//     a0 = s.a, a NaN counting as 0
//     a1 = levels ? ramp((a0 - black) * inv) : a0            ramp(t) = (t < 1) ? ((t > 0) ? t : 0) : 1
//     a2 = min (shrink) / max (grow) of a1 over the (2r + 1)^2 square clipped to S;  r == 0: a1
//     h  = t after: t = 0; for k ascending: if (x + k - c, y) in S: t = t + a2(x + k - c, y) * taps[k]
//     a3 = t after: t = 0; for k ascending: if (x, y + k - c) in S: t = t + h(x, y + k - c) * taps[k]         ntaps == 0: a2
//     out = show ? (a3, a3, a3, 1) : (s.r, s.g, s.b code for code, a3)                                   f16 truncated once at the store
// a1 holds no NaN, so minimum and maximum do not depend on the order they are formed in (the sign of a zero apart, which the
// contract leaves open): the square's minimum is formed as a row minimum followed by a column minimum, and a maximum as the
// minimum of the negated values, negated back (exact), so that one code path serves both signs of choke.  Samples outside S
// are staged as +Inf, the identity of the minimum: they are skipped, not taken as transparent.  The feather tests coordinates,
// not values, and never reads such a sample into a sum that is used.
//
// Shape: a 256-lane workgroup owns a tile of tw x th output pixels (host/matte.c plans it from R = r + c) and stages the alpha of
// the tile plus a halo of R on every side as f32 in LDS, 4 B per sample, in two images of (tw + 2R) x (th + 2R) that the passes
// write alternately:  stage -> A;  row minimum A -> B;  column minimum B -> A (a2);  horizontal feather A -> B;  the vertical
// feather reads B and goes straight to the store.  Each pass covers only the margin the later passes still need.  One launch for
// every legal parameter set, no frame in HBM in between.  choke == 0 and ntaps == 0 skip their two passes (workgroup-uniform);
// levels, grow and show are uniform selects: three instances in all, by pixel layout.
// Colour is not staged: in the last pass a lane reads its own pixels (16 bytes: an f32 pixel, or two half pixels where base, pitch
// and window parity of both frames allow -- stream_common.hpp pair_view -- else one half pixel in 8 bytes) and stores them
// with the new alpha, non-temporally.  Halo alpha that neighbouring tiles stage again comes through L2.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "pixel_math.hpp"
#include "stream_common.hpp"

namespace {

using namespace rowstream;

constexpr int kThreads = 256;

__device__ __forceinline__ float ramp(float t) { return (t < 1.0f) ? ((t > 0.0f) ? t : 0.0f) : 1.0f; }

// every (x, y) of the rectangle x0 .. x0 + w - 1, y0 .. y0 + h - 1 once, dealt to the lanes row-major (w >= 64: a lane moves at
// most four rows per step)
template <class F>
__device__ __forceinline__ void sweep(int x0, int w, int y0, int h, F f) {
    int y = (int)threadIdx.x / w, x = (int)threadIdx.x - y * w;
    while (y < h) {
        f(x0 + x, y0 + y);
        x += kThreads;
        while (x >= w) { x -= w; y++; }
    }
}

// HALF: 0 = rgba_f32 frames, one pixel per lane; 1 = rgba_f16, one pixel per lane; 2 = rgba_f16, two pixels per lane
template <int HALF>
__global__ __launch_bounds__(kThreads) void k_matte_refine(cvk_matte_params mp) {
    constexpr int PIX = HALF == 2 ? 2 : 1;
    extern __shared__ float lds[];
    const int r = mp.r, nt = mp.ntaps, c = nt > 0 ? (nt - 1) / 2 : 0, R = r + c;
    const int pw = mp.tw + 2 * R, ph = mp.th + 2 * R;
    float *A = lds, *B = lds + pw * ph;
    const int tx0 = mp.xs + (int)blockIdx.x * mp.tw, ty0 = mp.w.y0 + (int)blockIdx.y * mp.th;
    const int ox = tx0 - R, oy = ty0 - R;                      // frame coordinates of image sample (0, 0)
    const cvk_rect S = mp.s;
    const bool grow = mp.grow != 0;                            // uniform

    // stage a1 (negated where the matte grows); outside S: the minimum's identity
    sweep(0, pw, 0, ph, [&](int x, int y) {
        const int gx = ox + x, gy = oy + y;
        float a = __builtin_inff();
        if (gx >= S.x0 && gx <= S.x1 && gy >= S.y0 && gy <= S.y1) {
            const long long at = (long long)(gy - mp.in.fy0) * mp.in.pitch + (gx - mp.in.fx0);
            if (HALF) a = cvs::h2f(static_cast<const uint16_t *>(mp.in.data)[at * 4 + 3]);
            else a = static_cast<const float *>(mp.in.data)[at * 4 + 3];
            a = (a == a) ? a : 0.0f;
            if (mp.levels) a = ramp((a - mp.black) * mp.inv);  // uniform
            a = grow ? -a : a;
        }
        A[y * pw + x] = a;
    });
    __syncthreads();

    if (r > 0) {                                               // uniform
        sweep(r, pw - 2 * r, 0, ph, [&](int x, int y) {
            const float *p = A + y * pw + x;
            float v = p[-r];
            for (int i = 1 - r; i <= r; i++) { const float s = p[i]; v = s < v ? s : v; }
            B[y * pw + x] = v;
        });
        __syncthreads();
        sweep(r, pw - 2 * r, r, ph - 2 * r, [&](int x, int y) {
            const float *p = B + y * pw + x;
            float v = p[-r * pw];
            for (int j = 1 - r; j <= r; j++) { const float s = p[j * pw]; v = s < v ? s : v; }
            A[y * pw + x] = grow ? -v : v;
        });
        __syncthreads();
    }

    if (nt > 0) {                                              // uniform
        sweep(R, mp.tw, r, ph - 2 * r, [&](int x, int y) {
            const float *p = A + y * pw + (x - c);
            const int g0 = ox + x - c;                         // the frame column of tap 0
            float t = 0.0f;
            for (int k = 0; k < nt; k++) {
                const float q = p[k] * mp.taps[k];
                const float u = t + q;
                t = (g0 + k >= S.x0 && g0 + k <= S.x1) ? u : t;
            }
            B[y * pw + x] = t;
        });
        __syncthreads();
    }

    // the vertical feather and the pixels
    sweep(0, mp.tw / PIX, 0, mp.th, [&](int ix, int iy) {
        const int x = tx0 + ix * PIX, y = ty0 + iy;
        if (y > mp.w.y1) return;
        const bool m0 = x >= mp.w.x0 && x <= mp.w.x1, m1 = PIX == 2 && x + 1 >= mp.w.x0 && x + 1 <= mp.w.x1;
        if (!m0 && !m1) return;
        v4 px;
        if (HALF) px = load_px<PIX>(mp.in, x, y);
        else px = *reinterpret_cast<const v4 *>(static_cast<const char *>(mp.in.data) + ((long long)(y - mp.in.fy0) * mp.in.pitch + (x - mp.in.fx0)) * 16);
        float a3[PIX];
#pragma unroll
        for (int e = 0; e < PIX; e++) {
            const int lx = R + ix * PIX + e, ly = R + iy;
            if (nt > 0) {
                const float *p = B + (ly - c) * pw + lx;
                const int g0 = y - c;                          // the frame row of tap 0
                float t = 0.0f;
                for (int k = 0; k < nt; k++) {
                    const float q = p[k * pw] * mp.taps[k];
                    const float u = t + q;
                    t = (g0 + k >= S.y0 && g0 + k <= S.y1) ? u : t;
                }
                a3[e] = t;
            } else {
                a3[e] = A[ly * pw + lx];
            }
        }
        if (HALF) {
            v4 o = px;
            if (mp.show) {                                     // uniform
                o.x = cvs::f2h_rz2(a3[0], a3[0]); o.y = cvs::f2h_rz2(a3[0], 1.0f);
                if (PIX == 2) { o.z = cvs::f2h_rz2(a3[1], a3[1]); o.w = cvs::f2h_rz2(a3[1], 1.0f); }
            } else {
                o.y = (px.y & 0xFFFFu) | (cvs::f2h_rz(a3[0]) << 16);
                if (PIX == 2) o.w = (px.w & 0xFFFFu) | (cvs::f2h_rz(a3[1]) << 16);
            }
            store_px<PIX>(mp.out, x, y, o, m0, m1);
        } else {
            const uint32_t a = __float_as_uint(a3[0]);
            const v4 o = mp.show ? v4{ a, a, a, 0x3F800000u } : v4{ px.x, px.y, px.z, a };
            char *p = static_cast<char *>(mp.out.data) + ((long long)(y - mp.out.fy0) * mp.out.pitch + (x - mp.out.fx0)) * 16;
            __builtin_nontemporal_store(o, reinterpret_cast<v4 *>(p));
        }
    });
}

template <int HALF>
int launch(const cvk_matte_params &mp, size_t bytes, hipStream_t st) {
    // more dynamic LDS than a launch may ask for by default (the CU has 160 KiB): the instance is told first
    if (bytes > (48u << 10)) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_matte_refine<HALF>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)CVK_MATTE_MAX_LDS);
        if (e != hipSuccess) return (int)e;
    }
    const long long cols = (long long)mp.w.x1 - mp.xs + 1, rows = (long long)mp.w.y1 - mp.w.y0 + 1;
    const long long tiles = (rows + mp.th - 1) / mp.th;
    // a window of any height: bands of at most kMaxGridY rows of tiles, one launch each (a tile stages its own halo from S,
    // which stays the whole source window, so a band is the same kernel on a window that starts further down)
    for (long long first = 0; first < tiles; first += kMaxGridY) {
        const long long n = tiles - first < kMaxGridY ? tiles - first : kMaxGridY;
        cvk_matte_params band = mp;
        band.w.y0 = (int)(mp.w.y0 + first * mp.th);
        const long long last = (long long)band.w.y0 + n * mp.th - 1;
        band.w.y1 = last < mp.w.y1 ? (int)last : mp.w.y1;
        const dim3 grid((unsigned)((cols + mp.tw - 1) / mp.tw), (unsigned)n, 1);
        hipLaunchKernelGGL((k_matte_refine<HALF>), grid, dim3(kThreads), bytes, st, band);
        const int rc = (int)hipGetLastError();
        if (rc != 0) return rc;
    }
    return 0;
}

}  // namespace

extern "C" size_t cvk_matte_lds_bytes(int tw, int th, int halo) { return (size_t)2 * (size_t)(tw + 2 * halo) * (size_t)(th + 2 * halo) * sizeof(float); }

extern "C" int cvk_matte_refine(const cvk_matte_params *in, int half, void *stream) {
    cvk_matte_params mp = *in;
    if (rect_empty(mp.w)) return 0;
    const int c = mp.ntaps > 0 ? (mp.ntaps - 1) / 2 : 0;
    if (mp.r < 0 || mp.r > 16 || mp.ntaps < 0 || mp.ntaps > 25 || (mp.ntaps > 0 && !(mp.ntaps & 1)) || mp.tw < 64 || (mp.tw & 1) || mp.th < 1) return (int)hipErrorInvalidValue;
    const size_t bytes = cvk_matte_lds_bytes(mp.tw, mp.th, mp.r + c);
    if (bytes > CVK_MATTE_MAX_LDS) return (int)hipErrorInvalidValue;
    const int xs2 = mp.w.x0 - (int)(((long long)mp.w.x0 - mp.out.fx0) & 1);
    const bool pairs = half && pair_view(mp.out, xs2) && pair_view(mp.in, xs2);
    mp.xs = pairs ? xs2 : mp.w.x0;
    hipStream_t st = (hipStream_t)stream;
    if (!half) return launch<0>(mp, bytes, st);
    return pairs ? launch<2>(mp, bytes, st) : launch<1>(mp, bytes, st);
}
