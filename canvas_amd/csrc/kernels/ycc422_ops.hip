// ycc422_ops.hip -- the 4:2:2 export edge: half RGBA -> planar 8/10-bit, UYVY or v210 Y'CbCr (include/canvas_ycc422.h).
//
//   k_ycc422_subsample   no reference code; the MPEG-2 export edge (mpeg2_ops.hip) without its vertical part, with every rounding
//                        fixed (DESIGN.md "4:2:2 Y'CbCr edges"):
//     P(x, y)   the frame's half RGBA inside the window `w` (current_window clipped to the raster), else 0; column -1 reads
//               column 0; alpha ignored.
//     encode    r, g, b through the linear -> Rec.709 half table, widened to f32; the Rec.601 or Rec.709 matrix, every product
//               and sum rounded on its own (no FMA in either arithmetic flavour: this unit is built once):
//                 Y = (r*m0 + g*m1) + b*m2, Cb = (r*m3 + g*m4) + b*m5, Cr = (r*m6 + g*m7) + b*m8
//     luma      from every pixel.   chroma of pair k: C = 0.25*E(2k-1) + 0.5*E(2k) + 0.25*E(2k+1), left to right.
//     quantise  q = Y*(219s/max) + 16s/max or C*(224s/max) + 128s/max, s = 1, max = 255 (8-bit) or s = 4, max = 1023 (10-bit);
//               code = rint(clamp(q, 0, 1) * max), half to even, NaN -> 0; 10-bit: the code clamped to [4, 1019].
// A row-local stream.  One lane owns one pixel pair of the byte layouts (one 16-byte load; neighbouring lanes read neighbouring
// pixels and write neighbouring samples, as at the MPEG-2 edge) or one v210 group (six pixels, three chroma pairs, three 16-byte
// loads, one 16-byte store), over a strip of consecutive rows.  E(2k-1) of a lane's first pair is the left lane's last pixel
// (__shfl_up); lane 0 of every wave computes the group left of the wave's first one for that purpose only, so a wave produces 63
// lanes' worth per row and every lane runs the same instructions.  Every sample of the raster is written and no byte beyond: a
// lane right of the row's last pair stores nothing; a v210 group is always written whole, the fields beyond the width and bits
// 30-31 as 0.
// The 128 KiB table: staged into LDS or gathered from L2, by the raster's size; the launch is persistent, strided over the units
// (strip of rows, run of 63 lanes), and the next row's pixels are loaded before the current row is worked out, the first unit's
// first row before the table is staged (table_placement.hpp).
// Algorithmic bytes per pixel: 8 read; 2 (PLANAR8, UYVY), 4 (PLANAR10), 2.67 (v210) written.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "ycc_edge.hpp"

namespace {

using cvs::kTable; using cvs::kTableL2; using cvs::kTableLds;
using cvs::v4; using cvs::aligned; using cvs::fetch_pair; using cvs::Mat9; using cvs::Ycc; using cvs::tent;
constexpr int kRun = 63, kMaxStrip = 64;
enum { kP8 = CVK_422_PLANAR8, kP10 = CVK_422_PLANAR10, kUyvy = CVK_422_UYVY, kV210 = CVK_422_V210 };
template <int L> struct Lay {
    static constexpr int pairs = L == kV210 ? 3 : 1;                          // chroma pairs (pixel pairs) per lane
    static constexpr bool ten = L == kP10 || L == kV210;
};

// the P pixel pairs of lane group g of row y (a group left of the row or right of it: zeros)
template <int P>
__device__ __forceinline__ void fetch_group(const cvk_view &f, const cvk_rect &w, int g, int y, v4 (&px)[P]) {
#pragma unroll
    for (int i = 0; i < P; i++) px[i] = g >= 0 ? fetch_pair(f, w, 2 * ((long long)g * P + i), y) : v4{ 0u, 0u, 0u, 0u };
}

// studio range (cvs::quantise); the 10-bit codes 0-3 and 1020-1023 are reserved
template <bool TEN>
__device__ __forceinline__ uint32_t code_of(float v, bool chroma) {
    constexpr float s = TEN ? 4.0f : 1.0f, top = TEN ? 1023.0f : 255.0f;
    const float scale = chroma ? (224.0f * s) / top : (219.0f * s) / top, offset = chroma ? (128.0f * s) / top : (16.0f * s) / top;
    return cvs::quantise(v, scale, offset, top, TEN ? 4u : 0u, TEN ? 1019u : 255u);
}

// the codes of lane group g (a pair of the row, or a v210 group whose pairs below cw are the row's) into row y of the image
template <int L>
__device__ __forceinline__ void store_group(const cvk_ycc_image &im, int y, int g, int cw, const uint32_t (&yc)[2 * Lay<L>::pairs],
                                            const uint32_t (&bc)[Lay<L>::pairs], const uint32_t (&rc)[Lay<L>::pairs]) {
    uint8_t *row = im.p[0] + (size_t)y * (size_t)im.stride[0];
    if constexpr (L == kV210) {
        uint32_t yv[6], bv[3], rv[3];
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const bool in = 3LL * g + i < cw;
            yv[2 * i] = in ? yc[2 * i] : 0u; yv[2 * i + 1] = in ? yc[2 * i + 1] : 0u;
            bv[i] = in ? bc[i] : 0u; rv[i] = in ? rc[i] : 0u;
        }
        // word 0: Cb0 Y0 Cr0   word 1: Y1 Cb1 Y2   word 2: Cr1 Y3 Cb2   word 3: Y4 Cr2 Y5
        const v4 v = { bv[0] | (yv[0] << 10) | (rv[0] << 20), yv[1] | (bv[1] << 10) | (yv[2] << 20), rv[1] | (yv[3] << 10) | (bv[2] << 20),
                       yv[4] | (rv[2] << 10) | (yv[5] << 20) };
        uint8_t *p = row + (size_t)g * 16;
        if (aligned(p, 16)) __builtin_nontemporal_store(v, reinterpret_cast<v4 *>(p));
        else {
            uint32_t *q = reinterpret_cast<uint32_t *>(p);
            q[0] = v.x; q[1] = v.y; q[2] = v.z; q[3] = v.w;
        }
    } else if constexpr (L == kUyvy) {
        uint8_t *p = row + (size_t)g * 4;
        const uint32_t wd = bc[0] | (yc[0] << 8) | (rc[0] << 16) | (yc[1] << 24);
        if (aligned(p, 4)) __builtin_nontemporal_store(wd, reinterpret_cast<uint32_t *>(p));
        else {
#pragma unroll
            for (int b = 0; b < 4; b++) p[b] = (uint8_t)(wd >> (8 * b));
        }
    } else if constexpr (L == kP10) {
        uint16_t *py = reinterpret_cast<uint16_t *>(row) + 2 * (size_t)g;
        if (aligned(py, 4)) __builtin_nontemporal_store(yc[0] | (yc[1] << 16), reinterpret_cast<uint32_t *>(py));
        else { py[0] = (uint16_t)yc[0]; py[1] = (uint16_t)yc[1]; }
        reinterpret_cast<uint16_t *>(im.p[1] + (size_t)y * (size_t)im.stride[1])[g] = (uint16_t)bc[0];
        reinterpret_cast<uint16_t *>(im.p[2] + (size_t)y * (size_t)im.stride[2])[g] = (uint16_t)rc[0];
    } else {
        cvs::store_two<false>(row + 2 * (size_t)g, yc[0], yc[1]);
        (im.p[1] + (size_t)y * (size_t)im.stride[1])[g] = (uint8_t)bc[0];
        (im.p[2] + (size_t)y * (size_t)im.stride[2])[g] = (uint8_t)rc[0];
    }
}

// units: (strip of `strip` rows, run of kRun lane groups); `chunks` runs per strip.  A wave's unit is wave-uniform.
template <int L, int TABLE, int LANES>
__global__ __launch_bounds__(LANES) void k_ycc422_subsample(cvk_ycc_image im, cvk_view frame, cvk_rect w, Mat9 m, int width, int height, int strip,
                                                            int chunks, int units, const uint16_t *__restrict__ lut) {
    constexpr int kWaves = LANES / 64, P = Lay<L>::pairs;
    constexpr bool TEN = Lay<L>::ten;
    __shared__ __attribute__((aligned(16))) uint16_t lds[TABLE == kTableLds ? kTable : 8];
    const uint16_t *t = TABLE == kTableL2 ? lut : lds;
    const int lane = (int)(threadIdx.x & 63u), cw = width >> 1, groups = (cw + P - 1) / P, stride = (int)gridDim.x * kWaves;
    int u = (int)blockIdx.x * kWaves + (int)(threadIdx.x >> 6);
    v4 px[P];
#pragma unroll
    for (int i = 0; i < P; i++) px[i] = v4{ 0u, 0u, 0u, 0u };
    if (u < units) {                                       // the first unit's first row: before the table is staged
        const int sr = u / chunks;
        fetch_group<P>(frame, w, (u - sr * chunks) * kRun + lane - 1, sr * strip, px);
    }
    if (TABLE == kTableLds) {
        cvs::stage_table<LANES>(lds, lut);
        __syncthreads();
    }
    for (bool first = true; u < units; u += stride, first = false) {
        const int sr = u / chunks, g = (u - sr * chunks) * kRun + lane - 1;
        const int y0 = sr * strip, y1 = min(y0 + strip - 1, height - 1);
        if (!first) fetch_group<P>(frame, w, g, y0, px);
        for (int y = y0; y <= y1; y++) {
            v4 nx[P];
#pragma unroll
            for (int i = 0; i < P; i++) nx[i] = v4{ 0u, 0u, 0u, 0u };
            if (y < y1) fetch_group<P>(frame, w, g, y + 1, nx);
            Ycc e[2 * P];              // columns 2 (gP + i), 2 (gP + i) + 1
#pragma unroll
            for (int i = 0; i < P; i++) {
                e[2 * i] = cvs::encode<TABLE>(px[i].x, px[i].y, m, t);
                e[2 * i + 1] = cvs::encode<TABLE>(px[i].z, px[i].w, m, t);
            }
#pragma unroll
            for (int i = 0; i < P; i++) px[i] = nx[i];
            // column 2 g P - 1: the left lane's last pixel, or column 0 itself at the left edge
            float lb = __shfl_up(e[2 * P - 1].cb, 1), lr = __shfl_up(e[2 * P - 1].cr, 1);
            if (g == 0) { lb = e[0].cb; lr = e[0].cr; }
            if (g < 0 || g >= groups || lane == 0) continue;
            uint32_t yc[2 * P], bc[P], rc[P];
#pragma unroll
            for (int i = 0; i < P; i++) {
                yc[2 * i] = code_of<TEN>(e[2 * i].y, false);
                yc[2 * i + 1] = code_of<TEN>(e[2 * i + 1].y, false);
                const Ycc &left = e[max(2 * i - 1, 0)];        // (pair 0's left column is the neighbour lane's)
                bc[i] = code_of<TEN>(tent(i ? left.cb : lb, e[2 * i].cb, e[2 * i + 1].cb), true);
                rc[i] = code_of<TEN>(tent(i ? left.cr : lr, e[2 * i].cr, e[2 * i + 1].cr), true);
            }
            store_group<L>(im, y, g, cw, yc, bc, rc);
        }
    }
}

template <int L, int TABLE, int LANES>
static void launch(const cvk_ycc_image *im, cvk_view frame, cvk_rect w, const Mat9 &m, int width, int height, long long chunks, const cvs::StripPlan &p,
                   const uint16_t *lut, hipStream_t s) {
    hipLaunchKernelGGL((k_ycc422_subsample<L, TABLE, LANES>), cvs::table_grid<LANES>(p.units, p.most), dim3(LANES), 0, s, *im, frame, w, m, width, height,
                       (int)p.strip, (int)chunks, (int)p.units, lut);
}

template <int L>
static int dispatch(const cvk_ycc_image *im, cvk_view frame, cvk_rect w, const Mat9 &m, int width, int height, const uint16_t *lut, long long cus,
                    hipStream_t s) {
    constexpr int P = Lay<L>::pairs;
    const long long groups = ((long long)(width / 2) + P - 1) / P, chunks = (groups + kRun - 1) / kRun;
    cvs::StripPlan p;      // strips of rows
    if (!cvs::plan_strips(chunks, height, (long long)width * (long long)height, true, cus, kMaxStrip, &p)) return (int)hipErrorInvalidValue;
    cvs::with_table(p.table, [&](auto TABLE, auto LANES) { launch<L, TABLE(), LANES()>(im, frame, w, m, width, height, chunks, p, lut, s); });
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int cvk_ycc422_subsample(const cvk_ycc_image *im, cvk_view frame, cvk_rect w, int width, int height, int layout, const float mat[9],
                                    const uint16_t *lut, int cus, void *stream) {
    if (width < 2 || (width & 1) || height < 1) return (int)hipErrorInvalidValue;
    if (w.x1 >= w.x0 && w.y1 >= w.y0 && (w.x0 < 0 || w.y0 < 0 || w.x1 >= width || w.y1 >= height)) return (int)hipErrorInvalidValue;
    const Mat9 m = cvs::mat9(mat);
    const long long n = cus > 0 ? cus : 256;
    hipStream_t s = (hipStream_t)stream;
    switch (layout) {
    case kP8: return dispatch<kP8>(im, frame, w, m, width, height, lut, n, s);
    case kP10: return dispatch<kP10>(im, frame, w, m, width, height, lut, n, s);
    case kUyvy: return dispatch<kUyvy>(im, frame, w, m, width, height, lut, n, s);
    case kV210: return dispatch<kV210>(im, frame, w, m, width, height, lut, n, s);
    default: return (int)hipErrorInvalidValue;
    }
}
