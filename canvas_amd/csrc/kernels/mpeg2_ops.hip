// mpeg2_ops.hip -- the MPEG-2 export edge: half RGBA -> planar 8-bit Y'CbCr 4:2:0, interlaced chroma siting.
//
//   k_mpeg2_subsample   src/cprocess/video_subsample.c:189-526 (video_subsample_mpeg2_gl, GLSL only there), restated
//                       with every rounding fixed (DESIGN.md "MPEG-2 4:2:0 subsample"):
//     P(x, y)   the frame's half RGBA inside the window `w` (current_window clipped to the raster), else 0; column -1
//               reads column 0 (the rectangle texture's clamp-to-edge); alpha ignored.
//     encode    r, g, b through the linear -> Rec.709 half table, widened to f32; Rec.601 matrix, every product and sum
//               rounded on its own (no FMA in either arithmetic flavour: this unit is built once):
//                 Y = (r*0.299 + g*0.587) + b*0.114, Cb = (r*-0.168736 + g*-0.331264) + b*0.5, Cr = (r*0.5 + g*-0.418688) + b*-0.081312
//     chroma    chroma row 2k (field 0): near luma row 4k, far 4k+2; row 2k+1 (field 1): near 4k+3, far 4k+1; columns
//               2cx-1, 2cx, 2cx+1; C = 3/16 n- + 6/16 n0 + 3/16 n+ + 1/16 f- + 2/16 f0 + 1/16 f+, left to right.
//     quantise  q = Y*(219/255) + 16/255 or C*(224/255) + 128/255; byte = rint(clamp(q, 0, 1) * 255), NaN -> 0.
// One lane owns one chroma column cx over one group of four luma rows (4k..4k+3): four 16-byte loads of the pixel pairs
// (2cx, 2cx+1), eight luma bytes, Cb and Cr of both fields.  The column 2cx-1 comes from the left lane's encode
// (__shfl_up); lane 0 of every wave computes the column pair left of the wave's first one for that purpose only, so a
// wave produces 63 chroma columns per unit of work and every lane runs the same instructions.
// The 128 KiB table: staged into LDS or gathered from L2, by the raster's size; the launch is persistent, strided over the units
// (table_placement.hpp).
// Algorithmic bytes: 8 read + 1.5 written per source pixel; measured and what bounds it: DESIGN.md 4.5.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "ycc_edge.hpp"

namespace {

using cvs::kTable; using cvs::kTableL2; using cvs::kTableLds; using cvs::kTableLdsUnstaged;
using cvs::v4; using cvs::v4a8; using cvs::Ycc; using cvs::fetch_pair;
constexpr int kCols = 63;
// Rec.601 R'G'B' -> Y'CbCr, as literals so that they fold into the instructions
constexpr cvs::Mat9 kRec601 = { 0.299f, 0.587f, 0.114f, -0.168736f, -0.331264f, 0.5f, 0.5f, -0.418688f, -0.081312f };

// byte = rint(clamp(Y*(219/255) + 16/255, 0, 1) * 255), likewise C with 224 and 128 (cvs::quantise)
__device__ __forceinline__ uint32_t luma_byte(float y) { return cvs::quantise(y, 219.0f / 255.0f, 16.0f / 255.0f, 255.0f, 0u, 255u); }
__device__ __forceinline__ uint32_t chroma_byte(float c) { return cvs::quantise(c, 224.0f / 255.0f, 128.0f / 255.0f, 255.0f, 0u, 255u); }

__device__ __forceinline__ float chroma(float nm, float n0, float np, float fm, float f0, float fp) {
    float c = (3.0f / 16.0f) * nm;
    c = c + (6.0f / 16.0f) * n0;
    c = c + (3.0f / 16.0f) * np;
    c = c + (1.0f / 16.0f) * fm;
    c = c + (2.0f / 16.0f) * f0;
    c = c + (1.0f / 16.0f) * fp;
    return c;
}

// the four pixel pairs (2cx, 2cx + 1) x rows 4k .. 4k + 3 of one lane; a block wholly inside `w` (every lane of a frame
// whose window covers the raster) takes four unconditional loads, issued together
__device__ __forceinline__ void fetch_block(const cvk_view &f, const cvk_rect &w, int cx, int k, int cw, v4 px[4]) {
    const int x0 = 2 * cx, y0 = 4 * k;
    if (cx >= 0 && cx < cw && x0 >= w.x0 && x0 + 1 <= w.x1 && y0 >= w.y0 && y0 + 3 <= w.y1) {
        const uint2 *p = reinterpret_cast<const uint2 *>(f.data) + (ptrdiff_t)(y0 - f.fy0) * (ptrdiff_t)f.pitch + (x0 - f.fx0);
#pragma unroll
        for (int r = 0; r < 4; r++) px[r] = __builtin_nontemporal_load(reinterpret_cast<const v4a8 *>(p + (ptrdiff_t)r * f.pitch));
    } else {
#pragma unroll
        for (int r = 0; r < 4; r++) px[r] = cx >= 0 && cx < cw ? fetch_pair(f, w, x0, y0 + r) : v4{ 0u, 0u, 0u, 0u };
    }
}

// units: (luma row group k, run of kCols chroma columns); `chunks` runs per row group, `units` = chunks * height / 4.
// A wave's unit is wave-uniform; the next unit's loads are issued before the current one is worked out, the first unit's
// before the table is staged.
template <int TABLE, int LANES>
__global__ __launch_bounds__(LANES) void k_mpeg2_subsample(cvk_dv_planes pl, cvk_view frame, cvk_rect w, int width, int chunks, int units,
                                                           const uint16_t *__restrict__ lut) {
    constexpr int kWaves = LANES / 64;
    __shared__ __attribute__((aligned(16))) uint16_t lds[kTable];
    const uint16_t *t = TABLE == kTableL2 ? lut : lds;
    const int lane = (int)(threadIdx.x & 63u), cw = width >> 1, stride = (int)gridDim.x * kWaves;
    int u = (int)blockIdx.x * kWaves + (int)(threadIdx.x >> 6);
    v4 px[4] = { { 0u, 0u, 0u, 0u }, { 0u, 0u, 0u, 0u }, { 0u, 0u, 0u, 0u }, { 0u, 0u, 0u, 0u } };
    if (u < units) {
        const int k = u / chunks;
        fetch_block(frame, w, (u - k * chunks) * kCols + lane - 1, k, cw, px);
    }
    if (TABLE == kTableLds || (TABLE == kTableLdsUnstaged && units < 0)) {     // (the unstaged form: a copy that never runs)
        cvs::stage_table<LANES>(lds, lut);
        __syncthreads();
    }
    for (; u < units; u += stride) {
        const int k = u / chunks, cx = (u - k * chunks) * kCols + lane - 1;
        const bool live = cx >= 0 && cx < cw;
        const int x0 = 2 * cx, y0 = 4 * k;
        v4 nx[4] = { { 0u, 0u, 0u, 0u }, { 0u, 0u, 0u, 0u }, { 0u, 0u, 0u, 0u }, { 0u, 0u, 0u, 0u } };
        if (u + stride < units) {
            const int kn = (u + stride) / chunks;
            fetch_block(frame, w, (u + stride - kn * chunks) * kCols + lane - 1, kn, cw, nx);
        }
        Ycc e0[4], e1[4];          // columns x0, x0 + 1 of rows y0 .. y0 + 3
#pragma unroll
        for (int r = 0; r < 4; r++) {
            e0[r] = cvs::encode<TABLE>(px[r].x, px[r].y, kRec601, t);
            e1[r] = cvs::encode<TABLE>(px[r].z, px[r].w, kRec601, t);
        }
#pragma unroll
        for (int r = 0; r < 4; r++) px[r] = nx[r];
        float lcb[4], lcr[4];      // column x0 - 1: the left lane's x0 + 1, or column 0 itself at the left edge
#pragma unroll
        for (int r = 0; r < 4; r++) {
            lcb[r] = __shfl_up(e1[r].cb, 1);
            lcr[r] = __shfl_up(e1[r].cr, 1);
            if (cx == 0) { lcb[r] = e0[r].cb; lcr[r] = e0[r].cr; }
        }
        if (!live || lane == 0) continue;
#pragma unroll
        for (int r = 0; r < 4; r++)
            cvs::store_two<false>(pl.y + (size_t)(y0 + r) * (size_t)pl.sy + (size_t)x0, luma_byte(e0[r].y), luma_byte(e1[r].y));
        // field 0: near row 0, far row 2; field 1: near row 3, far row 1 (of the group)
        const size_t c0 = (size_t)(2 * k), c1 = c0 + 1;
        pl.cb[c0 * (size_t)pl.scb + cx] = (uint8_t)chroma_byte(chroma(lcb[0], e0[0].cb, e1[0].cb, lcb[2], e0[2].cb, e1[2].cb));
        pl.cr[c0 * (size_t)pl.scr + cx] = (uint8_t)chroma_byte(chroma(lcr[0], e0[0].cr, e1[0].cr, lcr[2], e0[2].cr, e1[2].cr));
        pl.cb[c1 * (size_t)pl.scb + cx] = (uint8_t)chroma_byte(chroma(lcb[3], e0[3].cb, e1[3].cb, lcb[1], e0[1].cb, e1[1].cb));
        pl.cr[c1 * (size_t)pl.scr + cx] = (uint8_t)chroma_byte(chroma(lcr[3], e0[3].cr, e1[3].cr, lcr[1], e0[1].cr, e1[1].cr));
    }
}

template <int TABLE, int LANES>
static void launch(const cvk_dv_planes *pl, cvk_view frame, cvk_rect w, int width, long long chunks, long long units, const uint16_t *lut, long long most,
                   hipStream_t s) {
    hipLaunchKernelGGL((k_mpeg2_subsample<TABLE, LANES>), cvs::table_grid<LANES>(units, most), dim3(LANES), 0, s, *pl, frame, w, width, (int)chunks,
                       (int)units, lut);
}

}  // namespace

extern "C" int cvk_mpeg2_subsample(const cvk_dv_planes *pl, cvk_view frame, cvk_rect w, int width, int height, const uint16_t *lut, int cus, void *stream) {
    if (width < 2 || (width & 1) || height < 4 || (height & 3)) return (int)hipErrorInvalidValue;
    const long long chunks = ((long long)(width / 2) + kCols - 1) / kCols, pixels = (long long)width * (long long)height;
    cvs::StripPlan p;      // a unit is one row group: strips of 1
    if (!cvs::plan_strips(chunks, height / 4, pixels, true, cus > 0 ? cus : 256, 1, &p)) return (int)hipErrorInvalidValue;
    hipStream_t s = (hipStream_t)stream;
#ifdef CVS_DIAG
    if (cvs::table_placement(pixels) == kTableLdsUnstaged)
        launch<kTableLdsUnstaged, cvs::kTableLdsLanes>(pl, frame, w, width, chunks, p.units, lut, p.most, s);
    else
#endif
    cvs::with_table(p.table, [&](auto TABLE, auto LANES) { launch<TABLE(), LANES()>(pl, frame, w, width, chunks, p.units, lut, p.most, s); });
    return (int)hipGetLastError();
}
