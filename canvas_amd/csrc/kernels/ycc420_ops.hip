// ycc420_ops.hip -- the 4:2:0 export edge: half RGBA -> planar 8/10-bit, NV12 or P010 Y'CbCr, progressive (include/canvas_ycc420.h).
//
//   k_ycc420_subsample   no reference code; the 4:2:2 export edge (ycc422_ops.hip) with a vertical step in front of its chroma
//                        filter, every rounding fixed (DESIGN.md "4:2:0 Y'CbCr edges"; fetch, encode, quantise, tent: ycc_edge.hpp):
//     P(x, y)   the frame's half RGBA inside the window `w` (current_window clipped to the raster), else 0; column -1 reads
//               column 0 and row -1 row 0; alpha ignored.
//     encode    r, g, b through the linear -> Rec.709 half table where there is one, widened to f32; the matrix, every product
//               and sum rounded on its own (no FMA in either arithmetic flavour: this unit is built once):
//                 Y = (r*m0 + g*m1) + b*m2, Cb = (r*m3 + g*m4) + b*m5, Cr = (r*m6 + g*m7) + b*m8
//     luma      from every pixel.   chroma of block (c, k), from the colour differences E, vertical step first:
//                 left      V = (E(2c) + E(2c+1)) * 0.5;                     C = 0.25*V(2k-1) + 0.5*V(2k) + 0.25*V(2k+1)
//                 centre    the same V;                                      C = (V(2k) + V(2k+1)) * 0.5
//                 top-left  V = 0.25*E(2c-1) + 0.5*E(2c) + 0.25*E(2c+1);     C as for left siting
//               each left to right.
//     quantise  q = Y*y_scale + y_offset or C*c_scale + c_offset (full range: scale 1, which is q = Y and q = C + offset bit for
//               bit); code = rint(clamp(q, 0, 1) * top), half to even, NaN -> 0, then clamped to [lo, hi] (10-bit studio range:
//               [4, 1019]).  PLANAR10 writes bits 10-15 as 0, P010 bits 0-5.
// One lane owns one chroma block: the pixel pairs (2k, 2k+1) of rows 2c and 2c+1 (two 16-byte loads), over a strip of consecutive
// chroma rows.  V(2k-1) is the left lane's V(2k+1) (__shfl_up); lane 0 of every wave computes the block left of the wave's first
// one for that purpose only, so a wave produces 63 blocks per row pair and every lane runs the same instructions.  Top-left siting
// needs E(2c-1): the colour differences of the pair's lower row stay in registers for the next pair, so each frame row is loaded
// once per strip (the row above a strip's first once more).  Range and siting are launch-uniform arguments; the siting's branches
// are wave-uniform.  Every sample of the raster is written and no byte beyond; NV12 and P010 write a block's Cb and Cr with one 16-
// or 32-bit store where it is aligned.
// The 128 KiB table: staged into LDS or gathered from L2, by the raster's size; or absent.  The launch is persistent, strided over
// the units (strip of chroma rows, run of 63 lanes), and the next pair's pixels are loaded before the current pair is worked out,
// the first unit's first pair before the table is staged (table_placement.hpp).
// Algorithmic bytes per pixel: 8 read; 1.5 (8-bit) or 3 (10-bit) written.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "ycc_edge.hpp"

namespace {

using cvs::kTable; using cvs::kTableL2; using cvs::kTableLds; using cvs::kTableNone;
using cvs::v4; using cvs::Mat9; using cvs::Ycc; using cvs::encode; using cvs::tent; using cvs::store_two;
constexpr int kRun = 63, kMaxStrip = 32;
enum { kP8 = CVK_420_PLANAR8, kP10 = CVK_420_PLANAR10, kNv12 = CVK_420_NV12, kP010 = CVK_420_P010 };
template <int L> struct Lay {
    static constexpr bool ten = L == kP10 || L == kP010;
    static constexpr bool semi = L == kNv12 || L == kP010;            // Cb and Cr interleaved in plane 1
    static constexpr int shift = L == kP010 ? 6 : 0;                  // where a code sits in its sample
};

// the pixel pair (2k, 2k + 1) of row y (cvs::fetch_pair); zero too where the block is left of the raster (k < 0: lane 0 at the
// left edge)
__device__ __forceinline__ v4 block_row(const cvk_view &f, const cvk_rect &w, int k, int y) {
    if (k < 0) return v4{ 0u, 0u, 0u, 0u };
    return cvs::fetch_pair(f, w, 2LL * k, y);
}

struct Coef {
    Mat9 m;
    float y_scale, y_offset, c_scale, c_offset, top;
    uint32_t lo, hi;
    int siting;
};

__device__ __forceinline__ uint32_t luma_code(float v, const Coef &m) { return cvs::quantise(v, m.y_scale, m.y_offset, m.top, m.lo, m.hi); }
__device__ __forceinline__ uint32_t chroma_code(float v, const Coef &m) { return cvs::quantise(v, m.c_scale, m.c_offset, m.top, m.lo, m.hi); }

// units: (strip of `strip` chroma rows, run of kRun blocks); `chunks` runs per strip.  A wave's unit is wave-uniform.
template <int L, int TABLE, int LANES>
__global__ __launch_bounds__(LANES) void k_ycc420_subsample(cvk_ycc_image im, cvk_view frame, cvk_rect w, Coef m, int width, int height, int strip,
                                                            int chunks, int units, const uint16_t *__restrict__ lut) {
    constexpr int kWaves = LANES / 64, B = Lay<L>::ten ? 2 : 1, SH = Lay<L>::shift;
    constexpr bool TEN = Lay<L>::ten;
    __shared__ __attribute__((aligned(16))) uint16_t lds[TABLE == kTableLds ? kTable : 8];
    const uint16_t *t = TABLE == kTableLds ? lds : lut;
    const int lane = (int)(threadIdx.x & 63u), cw = width >> 1, ch = height >> 1, stride = (int)gridDim.x * kWaves;
    int u = (int)blockIdx.x * kWaves + (int)(threadIdx.x >> 6);
    v4 p0 = { 0u, 0u, 0u, 0u }, p1 = { 0u, 0u, 0u, 0u };
    if (u < units) {                                       // the first unit's first pair: before the table is staged
        const int s = u / chunks, k = (u - s * chunks) * kRun + lane - 1;
        p0 = block_row(frame, w, k, 2 * s * strip);
        p1 = block_row(frame, w, k, 2 * s * strip + 1);
    }
    if (TABLE == kTableLds) {
        cvs::stage_table<LANES>(lds, lut);
        __syncthreads();
    }
    for (bool fresh = true; u < units; u += stride, fresh = false) {
        const int s = u / chunks, k = (u - s * chunks) * kRun + lane - 1;
        const int c0 = s * strip, c1 = min(c0 + strip - 1, ch - 1);
        if (!fresh) {
            p0 = block_row(frame, w, k, 2 * c0);
            p1 = block_row(frame, w, k, 2 * c0 + 1);
        }
        // E(2c - 1) of both columns: the row above the strip, row -1 reading row 0 (top-left siting only; wave-uniform)
        float ab0 = 0.0f, ar0 = 0.0f, ab1 = 0.0f, ar1 = 0.0f;
        if (m.siting == CVK_420_TOPLEFT) {
            const v4 pa = block_row(frame, w, k, max(2 * c0 - 1, 0));
            const Ycc a0 = encode<TABLE>(pa.x, pa.y, m.m, t), a1 = encode<TABLE>(pa.z, pa.w, m.m, t);
            ab0 = a0.cb; ar0 = a0.cr; ab1 = a1.cb; ar1 = a1.cr;
        }
        for (int c = c0; c <= c1; c++) {
            v4 n0 = { 0u, 0u, 0u, 0u }, n1 = { 0u, 0u, 0u, 0u };
            if (c < c1) {
                n0 = block_row(frame, w, k, 2 * c + 2);
                n1 = block_row(frame, w, k, 2 * c + 3);
            }
            // rows 2c (e0) and 2c + 1 (e1), columns 2k (x) and 2k + 1 (y)
            const Ycc e0x = encode<TABLE>(p0.x, p0.y, m.m, t), e0y = encode<TABLE>(p0.z, p0.w, m.m, t);
            const Ycc e1x = encode<TABLE>(p1.x, p1.y, m.m, t), e1y = encode<TABLE>(p1.z, p1.w, m.m, t);
            p0 = n0; p1 = n1;
            float vbx, vrx, vby, vry;      // V of columns 2k and 2k + 1
            if (m.siting == CVK_420_TOPLEFT) {
                vbx = tent(ab0, e0x.cb, e1x.cb); vrx = tent(ar0, e0x.cr, e1x.cr);
                vby = tent(ab1, e0y.cb, e1y.cb); vry = tent(ar1, e0y.cr, e1y.cr);
                ab0 = e1x.cb; ar0 = e1x.cr; ab1 = e1y.cb; ar1 = e1y.cr;
            } else {
                vbx = (e0x.cb + e1x.cb) * 0.5f; vrx = (e0x.cr + e1x.cr) * 0.5f;
                vby = (e0y.cb + e1y.cb) * 0.5f; vry = (e0y.cr + e1y.cr) * 0.5f;
            }
            // V(2k - 1): the left lane's V(2k + 1), or column 0 itself at the left edge
            float lb = __shfl_up(vby, 1), lr = __shfl_up(vry, 1);
            if (k == 0) { lb = vbx; lr = vrx; }
            if (k < 0 || k >= cw || lane == 0) continue;
            const float cbv = m.siting == CVK_420_CENTER ? (vbx + vby) * 0.5f : tent(lb, vbx, vby);
            const float crv = m.siting == CVK_420_CENTER ? (vrx + vry) * 0.5f : tent(lr, vrx, vry);
            const uint32_t bc = chroma_code(cbv, m) << SH, rc = chroma_code(crv, m) << SH;
            uint8_t *py = im.p[0] + (size_t)(2 * c) * (size_t)im.stride[0] + (size_t)(2 * B) * (size_t)k;
            store_two<TEN>(py, luma_code(e0x.y, m) << SH, luma_code(e0y.y, m) << SH);
            store_two<TEN>(py + (size_t)im.stride[0], luma_code(e1x.y, m) << SH, luma_code(e1y.y, m) << SH);
            if constexpr (Lay<L>::semi) store_two<TEN>(im.p[1] + (size_t)c * (size_t)im.stride[1] + (size_t)(2 * B) * (size_t)k, bc, rc);
            else {
                uint8_t *pb = im.p[1] + (size_t)c * (size_t)im.stride[1] + (size_t)B * (size_t)k;
                uint8_t *pr = im.p[2] + (size_t)c * (size_t)im.stride[2] + (size_t)B * (size_t)k;
                if constexpr (TEN) { *reinterpret_cast<uint16_t *>(pb) = (uint16_t)bc; *reinterpret_cast<uint16_t *>(pr) = (uint16_t)rc; }
                else { *pb = (uint8_t)bc; *pr = (uint8_t)rc; }
            }
        }
    }
}

template <int L, int TABLE, int LANES>
static void launch(const cvk_ycc_image *im, cvk_view frame, cvk_rect w, const Coef &m, int width, int height, long long chunks, const cvs::StripPlan &p,
                   const uint16_t *lut, hipStream_t s) {
    hipLaunchKernelGGL((k_ycc420_subsample<L, TABLE, LANES>), cvs::table_grid<LANES>(p.units, p.most), dim3(LANES), 0, s, *im, frame, w, m, width, height,
                       (int)p.strip, (int)chunks, (int)p.units, lut);
}

template <int L>
static int dispatch(const cvk_ycc_image *im, cvk_view frame, cvk_rect w, const Coef &m, int width, int height, const uint16_t *lut, long long cus,
                    hipStream_t s) {
    const long long chunks = ((long long)(width / 2) + kRun - 1) / kRun;
    cvs::StripPlan p;      // strips of chroma rows
    if (!cvs::plan_strips(chunks, height / 2, (long long)width * (long long)height, lut != nullptr, cus, kMaxStrip, &p)) return (int)hipErrorInvalidValue;
    if (p.table == kTableNone) launch<L, kTableNone, cvs::kTableL2Lanes>(im, frame, w, m, width, height, chunks, p, lut, s);
    else cvs::with_table(p.table, [&](auto TABLE, auto LANES) { launch<L, TABLE(), LANES()>(im, frame, w, m, width, height, chunks, p, lut, s); });
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int cvk_ycc420_subsample(const cvk_ycc_image *im, cvk_view frame, cvk_rect w, int width, int height, int layout, const cvk_ycc420_encode *e,
                                    const uint16_t *lut, int cus, void *stream) {
    if (width < 2 || (width & 1) || height < 2 || (height & 1)) return (int)hipErrorInvalidValue;
    if (w.x1 >= w.x0 && w.y1 >= w.y0 && (w.x0 < 0 || w.y0 < 0 || w.x1 >= width || w.y1 >= height)) return (int)hipErrorInvalidValue;
    if (e->siting < CVK_420_LEFT || e->siting > CVK_420_TOPLEFT) return (int)hipErrorInvalidValue;
    const Coef m = { cvs::mat9(e->mat), e->y_scale, e->y_offset, e->c_scale, e->c_offset, e->top, e->lo, e->hi, e->siting };
    const long long n = cus > 0 ? cus : 256;
    hipStream_t s = (hipStream_t)stream;
    switch (layout) {
    case kP8: return dispatch<kP8>(im, frame, w, m, width, height, lut, n, s);
    case kP10: return dispatch<kP10>(im, frame, w, m, width, height, lut, n, s);
    case kNv12: return dispatch<kNv12>(im, frame, w, m, width, height, lut, n, s);
    case kP010: return dispatch<kP010>(im, frame, w, m, width, height, lut, n, s);
    default: return (int)hipErrorInvalidValue;
    }
}
