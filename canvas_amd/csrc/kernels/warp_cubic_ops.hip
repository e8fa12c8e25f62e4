// warp_cubic_ops.hip -- the Catmull-Rom filter of VideoTransformFilter and VideoCornerPinFilter: the third value of `filter` of
// cvs_transform_* and cvs_perspective_*, in a unit of its own so that transform_ops.hip and perspective_ops.hip keep holding
// exactly their four instances.
//
// No reference code; the contract is DESIGN.md "Catmull-Rom warps" and the head of warp_sample.hpp, which states the arithmetic
// from (u, v) on and the clamp rule (the result never leaves the range of the 4 x 4 samples it was made from).  u, v, the pixel
// of a lane, the addresses and the launchers' checks are those of the two warps, from warp_coords.hpp.  One build for both
// arithmetic flavours (not in FMA_KERN): every product and sum is rounded on its own.
//
// Shape, as the bilinear kernels: the 32 x 8 tile of a 256-lane workgroup, lanes along x first, one pixel per lane, taps
// straight from global memory through L1 (sixteen 8-byte loads per half pixel, sixteen 16-byte loads per f32 pixel), read row by
// row in the source but hoisted by hipcc above the arithmetic, all sixteen in flight and all sixteen pixels live (DESIGN.md has
// the registers), non-temporal stores, bands of kMaxGridY rows of tiles per launch.  A
// tap outside S loads the clamped address and a select drops it: no divergence at a layer's edge, and no address outside S.
// The other form of the half taps -- two 16-byte loads per tap row at 8-byte alignment, each holding two adjacent columns, the
// lane sorting out which half is which -- exists in the diagnostic build only (CVS_TRANSFORM_PLAN=...p), as for the bilinear
// kernel; DESIGN.md "Catmull-Rom warps", Measured.  Four instances: k_transform_cubic / k_perspective_cubic x f32 / f16.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "warp_coords.hpp"
#include "warp_sample.hpp"

namespace {

using namespace warp;
using rowstream::rect_empty;

template <int HALF>
__global__ __launch_bounds__(kThreads) void k_transform_cubic(cvk_transform_params tp) {
    int x, y;
    if (!affine_pixel(tp, x, y)) return;
    float u, v;
    affine_uv(tp.m, x, y, u, v);
    const v4 o = cubic<HALF>(u, v, Window(tp.s), [&](int i, int j) { return affine_address<HALF>(tp.in, i, j); });
    store<HALF>(affine_address<HALF>(tp.out, x, y), o);
}

template <int HALF>
__global__ __launch_bounds__(kThreads) void k_perspective_cubic(cvk_perspective_params pp) {
    int x, y;
    if (!pinned_pixel(pp, x, y)) return;
    float u, v;
    const bool front = pinned_uv(pp.h, x, y, u, v);
    const v4 o = cubic<HALF>(u, v, Window(pp.s), [&](int i, int j) { return pinned_address<HALF>(pp.in, pp.sdx, pp.sdy, i, j); });
    store<HALF>(pinned_address<HALF>(pp.out, pp.tdx, pp.tdy, x, y), front ? o : v4{ 0u, 0u, 0u, 0u });
}

#ifdef CVS_DIAG
typedef v4 v4_align8 __attribute__((aligned(8)));

// S is at least two columns wide (the launcher's condition).  The clamped columns of taps 0 and 1 both lie in the pair that
// starts at min(col[0], S.x1 - 1), those of taps 2 and 3 in the pair that starts at min(col[2], S.x1 - 1): each tap is the
// pair's first pixel when its column is the pair's, else its second
__global__ __launch_bounds__(kThreads) void k_transform_cubic_pair(cvk_transform_params tp) {
    int x, y;
    if (!affine_pixel(tp, x, y)) return;
    float u, v;
    affine_uv(tp.m, x, y, u, v);
    const int last = tp.s.x1 - 1;
    const v4 o = cubic_rows<1>(u, v, Window(tp.s), [&](const int (&col)[4], int j, Px (&p)[4]) {
        const int pa = col[0] < last ? col[0] : last, pb = col[2] < last ? col[2] : last;
        const v4 ra = *reinterpret_cast<const v4_align8 *>(affine_address<1>(tp.in, pa, j));
        const v4 rb = *reinterpret_cast<const v4_align8 *>(affine_address<1>(tp.in, pb, j));
        const Px alo = from_half(ra.x, ra.y), ahi = from_half(ra.z, ra.w), blo = from_half(rb.x, rb.y), bhi = from_half(rb.z, rb.w);
        p[0] = col[0] == pa ? alo : ahi;
        p[1] = col[1] == pa ? alo : ahi;
        p[2] = col[2] == pb ? blo : bhi;
        p[3] = col[3] == pb ? blo : bhi;
    });
    store<1>(affine_address<1>(tp.out, x, y), o);
}
#endif

}  // namespace

extern "C" int cvk_transform_cubic(const cvk_transform_params *in, int half, void *stream) {
    const cvk_transform_params &tp = *in;
    if (rect_empty(tp.w)) return 0;
    const int refused = transform_params_refused(tp, kThreads);
    if (refused != 0) return refused;
    hipStream_t st = (hipStream_t)stream;
#ifdef CVS_DIAG
    if (half && tp.pair_loads && tp.s.x1 > tp.s.x0) return launch_bands(k_transform_cubic_pair, tp, tp.tw, tp.th, st);   // a one-column S has no pair
#endif
    return half ? launch_bands(k_transform_cubic<1>, tp, tp.tw, tp.th, st) : launch_bands(k_transform_cubic<0>, tp, tp.tw, tp.th, st);
}

extern "C" int cvk_perspective_cubic(const cvk_perspective_params *in, int half, void *stream) {
    const cvk_perspective_params &pp = *in;
    if (rect_empty(pp.w)) return 0;
    const int refused = perspective_params_refused(pp);
    if (refused != 0) return refused;
    hipStream_t st = (hipStream_t)stream;
    return half ? launch_bands(k_perspective_cubic<1>, pp, kPinTileW, kPinTileH, st) : launch_bands(k_perspective_cubic<0>, pp, kPinTileW, kPinTileH, st);
}
