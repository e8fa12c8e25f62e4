// mpeg2_recon_ops.hip -- the MPEG-2 4:2:0 import edge: planar 8-bit Y'CbCr 4:2:0 -> half RGBA, interlaced or progressive siting.
//
//   k_mpeg2_reconstruct   no reference code (its decoder hands out 4:2:0 images, src/libav/AVVideoDecoder.c:75-97, and
//                         src/cprocess/video_reconstruct.c knows DV only); the contract is DESIGN.md "MPEG-2 4:2:0
//                         reconstruction", restated here:
//     decode    yf = ((float)Y - 16) / 219, c = ((float)C - 128) / 224, correctly rounded (video_reconstruct.c:32-39); a
//               256-entry table per kind, built in LDS by every workgroup with the same division
//     vertical  per chroma column k, v = near*wn + far*wf (two products, one sum), far row clamped to the plane:
//                 interlaced  f = y & 1, l = y >> 1, j = l >> 1, chroma field row j = plane row 2j + f, field rows clamped to
//                             [0, H/4 - 1]; f0 l even: j 7/8, j-1 1/8; f0 l odd: j 5/8, j+1 3/8; f1 l even: j 5/8, j-1 3/8;
//                             f1 l odd: j 7/8, j+1 1/8 (the inverse of k_mpeg2_subsample's siting: field 0 at field line
//                             2j + 1/4, field 1 at 2j + 3/4)
//                 progressive c = y >> 1: y = 2c: c 3/4, c-1 1/4; y = 2c+1: c 3/4, c+1 1/4; rows clamped to [0, H/2 - 1]
//     horizontal x = 2k: v(k); x = 2k+1: (v(k) + v(k+1)) * 0.5, k+1 clamped to W/2 - 1 (chroma co-sited with even columns)
//     matrix    r = (yf*m0 + cb*m1) + cr*m2, likewise g and b (video_reconstruct.c:114-122), every product and sum rounded on
//               its own: no FMA in either arithmetic flavour (the unit is built once, not in FMA_KERN)
//     store     f2h_rz2 of r, g, b and 1.0, all four codes through the Rec.709 -> linear (scene) half table
//               (video_reconstruct.c:128-131); the separate flavour's table in both flavours
// One lane owns one chroma column k, i.e. the luma column pair (2k, 2k+1), over consecutive luma row groups (4j .. 4j+3).
// v(k+1) comes from the right-hand lane (__shfl_down); lane 63 of every wave only loads the column right of the wave's run to
// hand it on, so a wave writes 63 column pairs per row and every lane runs the same instructions.  The launch is persistent; a
// wave's unit is a strip of consecutive row groups of one 63-column run.  A group needs two new
// chroma rows per plane (interlaced: field row j+1 of each field; progressive: rows 2j+1, 2j+2); the rest stay in a register
// ring, and the next group's bytes are loaded before the current group is worked out.  One 16-byte store per row and lane
// where the pixel pair is aligned and inside the window, 8-byte stores otherwise.
// The 128 KiB table: staged into LDS or gathered from L2, by the raster's size (table_placement.hpp).
// Algorithmic bytes: 1.5 read + 8 written per pixel.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "ycc_edge.hpp"

namespace {

using cvs::kTable; using cvs::kTableL2; using cvs::kTableLds; using cvs::clampi; using cvs::Mat9;
constexpr int kCols = 63, kMaxStrip = 16;
enum { kInterlaced = 0, kProgressive = 1 };
// the chroma rows a group keeps: interlaced {field 0: j-1, j, j+1; field 1: j-1, j, j+1}, progressive {2j-1, 2j, 2j+1, 2j+2}
template <int SITING> struct Ring { static constexpr int n = SITING == kInterlaced ? 6 : 4; };

// plane row of ring slot s for group j; slots 0..2 / 3..5 are field rows j-1 .. j+1 of field 0 / 1 (interlaced)
template <int SITING>
__device__ __forceinline__ int ring_row(int j, int s, int height) {
    if (SITING == kInterlaced) {
        const int f = s >= 3 ? 1 : 0;
        return 2 * clampi(j - 1 + (s - 3 * f), 0, height / 4 - 1) + f;
    }
    return clampi(2 * j - 1 + s, 0, height / 2 - 1);
}

// the two slots a group adds when it moves from j - 1 to j (the rest shift down): the last slot of each field, or the last two
template <int SITING> __device__ __forceinline__ int new_slot(int i) { return SITING == kInterlaced ? (i == 0 ? 2 : 5) : 2 + i; }

template <int SITING>
__device__ __forceinline__ void shift_ring(float (&c)[Ring<SITING>::n]) {
    if (SITING == kInterlaced) {
        c[0] = c[1]; c[1] = c[2];
        c[3] = c[4]; c[4] = c[5];
    } else {
        c[0] = c[2]; c[1] = c[3];
    }
}

// luma bytes (x, x + 1) of row y as one 16-bit value (lo = x)
__device__ __forceinline__ uint32_t load_luma(const cvk_dv_planes &pl, int y, int x, bool even) {
    const uint8_t *p = pl.y + (size_t)y * (size_t)pl.sy + (size_t)x;
    if (even) return *reinterpret_cast<const uint16_t *>(p);
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8);
}

struct GroupBytes { uint32_t y[4]; uint32_t cb[2], cr[2]; };

// what group j needs beyond its ring: four luma pairs (rows clamped into the raster) and the two new chroma rows
template <int SITING>
__device__ __forceinline__ void load_group(const cvk_dv_planes &pl, int j, int x, int k, int height, bool even, GroupBytes &g) {
#pragma unroll
    for (int r = 0; r < 4; r++) g.y[r] = load_luma(pl, min(4 * j + r, height - 1), x, even);
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int row = ring_row<SITING>(j, new_slot<SITING>(i), height);
        g.cb[i] = pl.cb[(size_t)row * (size_t)pl.scb + (size_t)k];
        g.cr[i] = pl.cr[(size_t)row * (size_t)pl.scr + (size_t)k];
    }
}

// v of luma row 4j + r from the ring: {near slot, far slot, near weight, far weight}
template <int SITING>
__device__ __forceinline__ float vertical(const float (&c)[Ring<SITING>::n], int r) {
    if (SITING == kInterlaced) {
        switch (r) {
        case 0: return c[1] * (7.0f / 8.0f) + c[0] * (1.0f / 8.0f);
        case 1: return c[4] * (5.0f / 8.0f) + c[3] * (3.0f / 8.0f);
        case 2: return c[1] * (5.0f / 8.0f) + c[2] * (3.0f / 8.0f);
        default: return c[4] * (7.0f / 8.0f) + c[5] * (1.0f / 8.0f);
        }
    }
    switch (r) {
    case 0: return c[1] * 0.75f + c[0] * 0.25f;
    case 1: return c[1] * 0.75f + c[2] * 0.25f;
    case 2: return c[2] * 0.75f + c[1] * 0.25f;
    default: return c[2] * 0.75f + c[3] * 0.25f;
    }
}

// units: (strip of `strip` row groups, run of kCols chroma columns) over the window's groups [ja, jb] and columns [ka, ...];
// `chunks` runs per strip, so the waves of neighbouring units write neighbouring parts of the same rows.  A wave's unit is
// wave-uniform.
template <int SITING, int TABLE, int LANES>
__global__ __launch_bounds__(LANES) void k_mpeg2_reconstruct(cvk_view frame, cvk_rect w, cvk_dv_planes pl, Mat9 m, int width, int height, int ka,
                                                             int ja, int jb, int strip, int chunks, int units, const uint16_t *__restrict__ lut) {
    constexpr int kWaves = LANES / 64, NR = Ring<SITING>::n;
    __shared__ __attribute__((aligned(16))) uint16_t lds[kTable];
    __shared__ float dec_y[256], dec_c[256];
    const uint16_t *t = TABLE == kTableL2 ? lut : lds;
    if (TABLE == kTableLds) cvs::stage_table<LANES>(lds, lut);      // (the wait is the __syncthreads() below)
    cvs::build_decode<256, LANES>(dec_y, dec_c, 16.0f, 219.0f, 128.0f, 224.0f);
    __syncthreads();
    const uint32_t alpha = t[0x3C00u];                     // f2h_rz(1.0f)
    const int lane = (int)(threadIdx.x & 63u), cw = width >> 1, stride = (int)gridDim.x * kWaves;
    const bool even = ((reinterpret_cast<uintptr_t>(pl.y) | (uintptr_t)pl.sy) & 1u) == 0;
    for (int u = (int)blockIdx.x * kWaves + (int)(threadIdx.x >> 6); u < units; u += stride) {
        const int s = u / chunks;
        const int k = ka + (u - s * chunks) * kCols + lane;
        const int kl = min(k, cw - 1);                     // the column this lane reads (k + 1 past the right edge reads W/2 - 1)
        const int x = 2 * k, xl = 2 * kl;
        const bool in0 = lane < kCols && x >= w.x0 && x <= w.x1, in1 = lane < kCols && x + 1 >= w.x0 && x + 1 <= w.x1;
        const int j0 = ja + s * strip, j1 = min(j0 + strip - 1, jb);
        float cb[NR], cr[NR];
#pragma unroll
        for (int i = 0; i < NR; i++) {
            const int row = ring_row<SITING>(j0, i, height);
            cb[i] = dec_c[pl.cb[(size_t)row * (size_t)pl.scb + (size_t)kl]];
            cr[i] = dec_c[pl.cr[(size_t)row * (size_t)pl.scr + (size_t)kl]];
        }
        GroupBytes cur;
        load_group<SITING>(pl, j0, xl, kl, height, even, cur);
        for (int j = j0; j <= j1; j++) {
            GroupBytes nxt = cur;
            if (j < j1) load_group<SITING>(pl, j + 1, xl, kl, height, even, nxt);
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int y = 4 * j + r;
                if (y < w.y0 || y > w.y1) continue;      // wave-uniform
                const float vb = vertical<SITING>(cb, r), vr = vertical<SITING>(cr, r);
                const float vb1 = __shfl_down(vb, 1), vr1 = __shfl_down(vr, 1);
                const float hb = (vb + vb1) * 0.5f, hr = (vr + vr1) * 0.5f;
                const uint2 p0 = cvs::pixel<TABLE>(dec_y[cur.y[r] & 0xFFu], vb, vr, m, t, alpha);
                const uint2 p1 = cvs::pixel<TABLE>(dec_y[cur.y[r] >> 8], hb, hr, m, t, alpha);
                uint2 *o = reinterpret_cast<uint2 *>(frame.data) + (ptrdiff_t)(y - frame.fy0) * (ptrdiff_t)frame.pitch + (x - frame.fx0);
                cvs::store_pixel_pair<true>(o, p0, p1, in0, in1);
            }
            cur = nxt;
            if (j < j1) {
                shift_ring<SITING>(cb);
                shift_ring<SITING>(cr);
#pragma unroll
                for (int i = 0; i < 2; i++) {
                    cb[new_slot<SITING>(i)] = dec_c[cur.cb[i]];
                    cr[new_slot<SITING>(i)] = dec_c[cur.cr[i]];
                }
            }
        }
    }
}

template <int SITING, int TABLE, int LANES>
static void launch(cvk_view frame, cvk_rect w, const cvk_dv_planes *pl, const Mat9 &m, int width, int height, int ka, int ja, int jb, long long chunks,
                   const cvs::StripPlan &p, const uint16_t *lut, hipStream_t s) {
    hipLaunchKernelGGL((k_mpeg2_reconstruct<SITING, TABLE, LANES>), cvs::table_grid<LANES>(p.units, p.most), dim3(LANES), 0, s, frame, w, *pl, m, width,
                       height, ka, ja, jb, (int)p.strip, (int)chunks, (int)p.units, lut);
}

}  // namespace

extern "C" int cvk_mpeg2_reconstruct(cvk_view frame, cvk_rect w, const cvk_dv_planes *pl, int width, int height, int progressive, const float mat[9],
                                     const uint16_t *lut, int cus, void *stream) {
    if (width < 2 || (width & 1) || height < 2 || (height & 1) || (!progressive && (height & 3))) return (int)hipErrorInvalidValue;
    if (w.x1 < w.x0 || w.y1 < w.y0) return 0;
    if (w.x0 < 0 || w.y0 < 0 || w.x1 >= width || w.y1 >= height) return (int)hipErrorInvalidValue;
    const int ka = w.x0 >> 1, ja = w.y0 >> 2, jb = w.y1 >> 2;
    const long long chunks = ((long long)(w.x1 >> 1) - ka + kCols) / kCols, groups = (long long)jb - ja + 1;
    cvs::StripPlan p;      // strips of row groups
    if (!cvs::plan_strips(chunks, groups, (long long)width * (long long)height, true, cus > 0 ? cus : 256, kMaxStrip, &p)) return (int)hipErrorInvalidValue;
    const Mat9 m = cvs::mat9(mat);
    hipStream_t s = (hipStream_t)stream;
    cvs::with_table(p.table, [&](auto TABLE, auto LANES) {
        if (progressive) launch<kProgressive, TABLE(), LANES()>(frame, w, pl, m, width, height, ka, ja, jb, chunks, p, lut, s);
        else launch<kInterlaced, TABLE(), LANES()>(frame, w, pl, m, width, height, ka, ja, jb, chunks, p, lut, s);
    });
    return (int)hipGetLastError();
}
