// transform_ops.hip -- VideoTransformFilter: an affine warp of un-premultiplied RGBA device frames, the bilinear filter weighted
// by alpha.
//
// No reference code; the contract is DESIGN.md "Affine transform" and the comment of include/canvas_hip.h.  S = the source's
// current window, `w` the window written, m the TARGET -> SOURCE coefficients, coordinates ABSOLUTE.  In f32, every operation
// rounded on its own:
//     x, y = (float) of the target pixel's coordinates;  u = (m0*x + m1*y) + m2;  v = (m3*x + m4*y) + m5
// then the nearest or the bilinear filter of warp_sample.hpp, which states the arithmetic from (u, v) on and why no address is
// ever formed outside S.  Every coordinate of S is within +-2^23 (host/transform.c refuses others).
//
// Shape: the reads follow a rotated footprint, so a wave that owned 64 pixels of one row would touch up to 64 source rows.  A
// 256-lane workgroup owns a tw x th tile of target pixels instead (tw * th == 256, planned in host/transform.c; lanes run along x
// first, so a wave covers 64 / tw rows of the tile when tw < 64): under any angle the wave's source footprint is a compact patch
// that the 32 KiB L1 serves, and stores stay lane-contiguous along x.  Taps come straight from global memory: one 16-byte load
// per f32 tap, one 8-byte load per half tap.  The other form of the half taps -- the two horizontally adjacent ones in one 16-byte
// load at 8-byte alignment from the pair's column clamped to S.x0 .. S.x1 - 1, the lane sorting out which half is which (PAIR) --
// exists in the diagnostic build only: it measured 1.7 to 1.9 times slower when the plan was chosen, and no slower as it is
// written now (DESIGN.md "Affine transform", Measured, and its note of 2026-10-20); the built plan has not been changed.
// One pixel per lane, stores non-temporal.  Four instances: f32 / f16 x nearest / bilinear (the Catmull-Rom filter's two are in
// warp_cubic_ops.hip: this object holds exactly these four).
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "warp_coords.hpp"
#include "warp_sample.hpp"

namespace {

using namespace warp;
using rowstream::rect_empty;

typedef v4 v4_align8 __attribute__((aligned(8)));

// (the pixel of a lane, u and v and the addresses: warp_coords.hpp, shared with the Catmull-Rom kernel of warp_cubic_ops.hip)
template <int HALF>
__device__ __forceinline__ char *address(const cvk_view &f, int i, int j) { return affine_address<HALF>(f, i, j); }

template <int HALF, int BILINEAR, int PAIR>
__global__ __launch_bounds__(kThreads) void k_transform(cvk_transform_params tp) {
    int x, y;
    if (!affine_pixel(tp, x, y)) return;
    float u, v;
    affine_uv(tp.m, x, y, u, v);
    const Window s(tp.s);
    v4 o;
    if (HALF && BILINEAR && PAIR) {
        // S is at least two columns wide (the launcher's condition): the pair (ip, ip + 1) lies inside S, and holds both taps
        // in order when the left tap is its first pixel; otherwise one tap is outside S and the other is the pair's far pixel
        const Taps t(u, v, s);
        const float fip = clampf(t.fi, s.x0, s.x1 - 1.0f);
        const int ip = (int)fip;
        const bool ordered = t.fi == fip;
        const v4 r0 = *reinterpret_cast<const v4_align8 *>(address<1>(tp.in, ip, s.row(t.fj)));
        const v4 r1 = *reinterpret_cast<const v4_align8 *>(address<1>(tp.in, ip, s.row(t.fj + 1.0f)));
        const Px lo0 = from_half(r0.x, r0.y), hi0 = from_half(r0.z, r0.w), lo1 = from_half(r1.x, r1.y), hi1 = from_half(r1.z, r1.w);
        o = blend<1>(t, ordered ? lo0 : hi0, ordered ? hi0 : lo0, ordered ? lo1 : hi1, ordered ? hi1 : lo1);
    } else {
        o = sample<HALF, BILINEAR>(u, v, s, [&](int i, int j) { return address<HALF>(tp.in, i, j); });
    }
    store<HALF>(address<HALF>(tp.out, x, y), o);
}

template <int HALF, int BILINEAR, int PAIR>
int launch(const cvk_transform_params &tp, hipStream_t st) { return launch_bands(k_transform<HALF, BILINEAR, PAIR>, tp, tp.tw, tp.th, st); }

}  // namespace

extern "C" int cvk_transform(const cvk_transform_params *in, int half, void *stream) {
    const cvk_transform_params &tp = *in;
    if (rect_empty(tp.w)) return 0;
    const int refused = transform_params_refused(tp, kThreads);
    if (refused != 0) return refused;
    hipStream_t st = (hipStream_t)stream;
    if (!tp.bilinear) return half ? launch<1, 0, 0>(tp, st) : launch<0, 0, 0>(tp, st);
    if (!half) return launch<0, 1, 0>(tp, st);
#ifdef CVS_DIAG
    if (tp.pair_loads && tp.s.x1 > tp.s.x0) return launch<1, 1, 1>(tp, st);                // a one-column S has no pair
#endif
    return launch<1, 1, 0>(tp, st);
}
