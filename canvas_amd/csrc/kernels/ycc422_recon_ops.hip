// ycc422_recon_ops.hip -- the 4:2:2 import edge: planar 8/10-bit, UYVY or v210 Y'CbCr -> half RGBA (include/canvas_ycc422.h).
//
//   k_ycc422_reconstruct   no reference code (its decoder hands 4:2:2 images out untouched, src/libav/AVVideoDecoder.c:72-91, and
//                          neither reconstruction filter reads them); the contract is DESIGN.md "4:2:2 Y'CbCr edges", restated:
//     decode     yf = ((float)Y - 16s) / (219s), c = ((float)C - 128s) / (224s), s = 1 (8-bit) or 4 (10-bit), correctly rounded; a
//                256- or 1024-entry table per kind, built in LDS by every workgroup with the same division.  PLANAR10 codes are
//                masked to bits 0-9, v210 fields likewise (bits 30-31 of a word and the fields beyond the width are never used)
//     horizontal x = 2k: v(k); x = 2k+1: (v(k) + v(k+1)) * 0.5, k+1 clamped to W/2 - 1 (chroma co-sited with even columns)
//     matrix     r = (yf*m0 + cb*m1) + cr*m2, likewise g and b, every product and sum rounded on its own: no FMA in either
//                arithmetic flavour (the unit is built once, not in FMA_KERN)
//     store      f2h_rz of r, g, b and 1.0, all four codes through the Rec.709 -> linear (scene) half table; the separate flavour's
//                table in both flavours
// A row-local stream: nothing couples two rows.  One lane owns one pixel pair of the byte layouts (PLANAR8: 2 + 1 + 1 bytes,
// PLANAR10: 4 + 2 + 2, UYVY: 4: neighbouring lanes read neighbouring samples and write neighbouring pixels, as at the MPEG-2 edge)
// or one v210 group (16 bytes: six pixels, three chroma pairs), over a strip of consecutive rows.  v(k+1) of a lane's last pair is
// the right-hand lane's first (__shfl_down); lane 63 of every wave only loads the column right of the wave's run to hand it on, so
// a wave writes 63 lanes' worth per row and every lane runs the same instructions.  Reads past the width are never made: a lane
// reads its pair at min(k, W/2 - 1), which is also what the right-hand clamp of k+1 asks for; a v210 lane reads the row's last
// group at most and picks its pairs out of it.  The launch is persistent; a wave's unit is (strip of rows, run of 63 lanes) and
// the next row's samples are loaded before the current row is worked out, the first unit's first row before the tables are built.
// One 16-byte store per pixel pair where it is aligned and inside the window (non-temporal for the byte layouts), 8-byte stores
// otherwise.
// The 128 KiB table: staged into LDS or gathered from L2, by the raster's size (table_placement.hpp).
// Algorithmic bytes read per pixel: 2 (PLANAR8, UYVY), 4 (PLANAR10), 2.67 (v210); 8 written.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "ycc_edge.hpp"

namespace {

using cvs::kTable; using cvs::kTableL2; using cvs::kTableLds; using cvs::v4; using cvs::aligned; using cvs::Mat9;
constexpr int kRun = 63, kMaxStrip = 64;
enum { kP8 = CVK_422_PLANAR8, kP10 = CVK_422_PLANAR10, kUyvy = CVK_422_UYVY, kV210 = CVK_422_V210 };
template <int L> struct Lay {
    static constexpr int pairs = L == kV210 ? 3 : 1;                          // chroma pairs (pixel pairs) per lane
    static constexpr int codes = L == kP10 || L == kV210 ? 1024 : 256;        // sample codes
    static constexpr int words = L == kV210 ? 4 : (L == kP10 ? 2 : 1);        // dwords a lane's samples make
};

// The samples of lane group g of row y as dwords:
//   PLANAR8   r[0] = Y'0 | Y'1 << 8 | Cb << 16 | Cr << 24      PLANAR10  r[0] = Y'0 | Y'1 << 16, r[1] = Cb | Cr << 16
//   UYVY      r[0] = Cb | Y'0 << 8 | Cr << 16 | Y'1 << 24      V210      the group's four words
// each read at the pair (the group) clamped to the row's last.
template <int L>
__device__ __forceinline__ void load_raw(const cvk_ycc_image &im, int y, int g, int cw, uint32_t (&r)[Lay<L>::words]) {
    const uint8_t *row = im.p[0] + (size_t)y * (size_t)im.stride[0];
    if constexpr (L == kV210) {
        const uint8_t *p = row + (size_t)min(g, (cw + 2) / 3 - 1) * 16;
        if (aligned(p, 16)) {
            const v4 v = __builtin_nontemporal_load(reinterpret_cast<const v4 *>(p));
            r[0] = v.x; r[1] = v.y; r[2] = v.z; r[3] = v.w;
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++) r[i] = reinterpret_cast<const uint32_t *>(p)[i];
        }
    } else if constexpr (L == kUyvy) {
        const uint8_t *p = row + (size_t)min(g, cw - 1) * 4;
        if (aligned(p, 4)) r[0] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t *>(p));
        else r[0] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
    } else {
        const size_t k = (size_t)min(g, cw - 1);
        const uint8_t *rb = im.p[1] + (size_t)y * (size_t)im.stride[1], *rr = im.p[2] + (size_t)y * (size_t)im.stride[2];
        if constexpr (L == kP10) {
            const uint16_t *py = reinterpret_cast<const uint16_t *>(row) + 2 * k;
            r[0] = aligned(py, 4) ? __builtin_nontemporal_load(reinterpret_cast<const uint32_t *>(py)) : ((uint32_t)py[0] | ((uint32_t)py[1] << 16));
            r[1] = (uint32_t)reinterpret_cast<const uint16_t *>(rb)[k] | ((uint32_t)reinterpret_cast<const uint16_t *>(rr)[k] << 16);
        } else {
            r[0] = cvs::load_two<false>(row + 2 * k) | ((uint32_t)rb[k] << 16) | ((uint32_t)rr[k] << 24);
        }
    }
}

__device__ __forceinline__ uint32_t field(uint32_t word, int n) { return (word >> (10 * n)) & 0x3FFu; }
__device__ __forceinline__ float pick3(int j, float a, float b, float c) { return j == 0 ? a : (j == 1 ? b : c); }

// decoded luma of the lane's 2P pixels and chroma of its P pairs; v210: pair 3g + i read at min(3g + i, W/2 - 1)
template <int L>
__device__ __forceinline__ void decode(const uint32_t (&r)[Lay<L>::words], int g, int cw, const float *dy, const float *dc,
                                       float (&yf)[2 * Lay<L>::pairs], float (&cb)[Lay<L>::pairs], float (&cr)[Lay<L>::pairs]) {
    if constexpr (L == kV210) {
        // word 0: Cb0 Y0 Cr0   word 1: Y1 Cb1 Y2   word 2: Cr1 Y3 Cb2   word 3: Y4 Cr2 Y5
        yf[0] = dy[field(r[0], 1)]; yf[1] = dy[field(r[1], 0)]; yf[2] = dy[field(r[1], 2)];
        yf[3] = dy[field(r[2], 1)]; yf[4] = dy[field(r[3], 0)]; yf[5] = dy[field(r[3], 2)];
        const float b0 = dc[field(r[0], 0)], b1 = dc[field(r[1], 1)], b2 = dc[field(r[2], 2)];
        const float r0 = dc[field(r[0], 2)], r1 = dc[field(r[2], 0)], r2 = dc[field(r[3], 1)];
        // the group that was loaded is min(g, last group): pair 3g + i, clamped to the row's last pair, within that group
        const int gl = min(g, (cw + 2) / 3 - 1);
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const int j = (int)(min(3LL * g + i, (long long)cw - 1) - 3LL * gl);
            cb[i] = pick3(j, b0, b1, b2);
            cr[i] = pick3(j, r0, r1, r2);
        }
    } else if constexpr (L == kUyvy) {
        cb[0] = dc[r[0] & 0xFFu]; yf[0] = dy[(r[0] >> 8) & 0xFFu];
        cr[0] = dc[(r[0] >> 16) & 0xFFu]; yf[1] = dy[r[0] >> 24];
    } else if constexpr (L == kP10) {
        yf[0] = dy[r[0] & 0x3FFu]; yf[1] = dy[(r[0] >> 16) & 0x3FFu];
        cb[0] = dc[r[1] & 0x3FFu]; cr[0] = dc[(r[1] >> 16) & 0x3FFu];
    } else {
        yf[0] = dy[r[0] & 0xFFu]; yf[1] = dy[(r[0] >> 8) & 0xFFu];
        cb[0] = dc[(r[0] >> 16) & 0xFFu]; cr[0] = dc[r[0] >> 24];
    }
}

// units: (strip of `strip` rows, run of kRun lane groups) over the window's rows [w.y0, w.y1] and groups from ga; `chunks` runs per
// strip, so the waves of neighbouring units write neighbouring parts of the same rows.  A wave's unit is wave-uniform.
template <int L, int TABLE, int LANES>
__global__ __launch_bounds__(LANES) void k_ycc422_reconstruct(cvk_view frame, cvk_rect w, cvk_ycc_image im, Mat9 m, int width, int ga, int strip,
                                                              int chunks, int units, const uint16_t *__restrict__ lut) {
    constexpr int kWaves = LANES / 64, P = Lay<L>::pairs, N = Lay<L>::codes, NW = Lay<L>::words;
    constexpr float s = N / 256;
    __shared__ __attribute__((aligned(16))) uint16_t lds[TABLE == kTableLds ? kTable : 8];
    __shared__ float dec_y[N], dec_c[N];
    const uint16_t *t = TABLE == kTableL2 ? lut : lds;
    const int lane = (int)(threadIdx.x & 63u), cw = width >> 1, stride = (int)gridDim.x * kWaves;
    int u = (int)blockIdx.x * kWaves + (int)(threadIdx.x >> 6);
    uint32_t cur[NW];
#pragma unroll
    for (int i = 0; i < NW; i++) cur[i] = 0u;
    if (u < units) {                                       // the first unit's first row: before the tables are built
        const int sr = u / chunks;
        load_raw<L>(im, w.y0 + sr * strip, ga + (u - sr * chunks) * kRun + lane, cw, cur);
    }
    if (TABLE == kTableLds) cvs::stage_table<LANES>(lds, lut);      // (the wait is the __syncthreads() below)
    cvs::build_decode<N, LANES>(dec_y, dec_c, 16.0f * s, 219.0f * s, 128.0f * s, 224.0f * s);
    __syncthreads();
    const uint32_t alpha = t[0x3C00u];                     // f2h_rz(1.0f)
    for (bool first = true; u < units; u += stride, first = false) {
        const int sr = u / chunks, g = ga + (u - sr * chunks) * kRun + lane;
        const int y0 = w.y0 + sr * strip, y1 = min(y0 + strip - 1, w.y1);
        if (!first) load_raw<L>(im, y0, g, cw, cur);
        for (int y = y0; y <= y1; y++) {
            uint32_t nxt[NW];
#pragma unroll
            for (int i = 0; i < NW; i++) nxt[i] = cur[i];
            if (y < y1) load_raw<L>(im, y + 1, g, cw, nxt);
            float yf[2 * P], cb[P], cr[P];
            decode<L>(cur, g, cw, dec_y, dec_c, yf, cb, cr);
            const float nb = __shfl_down(cb[0], 1), nr = __shfl_down(cr[0], 1);      // v(k + 1) of the lane's last pair
            uint2 *o = reinterpret_cast<uint2 *>(frame.data) + (ptrdiff_t)(y - frame.fy0) * (ptrdiff_t)frame.pitch;
#pragma unroll
            for (int i = 0; i < P; i++) {
                constexpr int kLast = P - 1;
                const long long x = 2 * ((long long)g * P + i);
                const float vb = cb[i], vr = cr[i], vb1 = i < kLast ? cb[min(i + 1, kLast)] : nb, vr1 = i < kLast ? cr[min(i + 1, kLast)] : nr;
                const float hb = (vb + vb1) * 0.5f, hr = (vr + vr1) * 0.5f;
                const uint2 p0 = cvs::pixel<TABLE>(yf[2 * i], vb, vr, m, t, alpha);
                const uint2 p1 = cvs::pixel<TABLE>(yf[2 * i + 1], hb, hr, m, t, alpha);
                const bool in0 = lane < kRun && x >= w.x0 && x <= w.x1, in1 = lane < kRun && x + 1 >= w.x0 && x + 1 <= w.x1;
                // non-temporal where neighbouring lanes write neighbouring pairs; a v210 lane's three pairs lie 48 bytes from its
                // neighbour's, and plain stores let L2 put the lines together before they leave
                cvs::store_pixel_pair<P == 1>(o + (x - frame.fx0), p0, p1, in0, in1);
            }
#pragma unroll
            for (int i = 0; i < NW; i++) cur[i] = nxt[i];
        }
    }
}

template <int L, int TABLE, int LANES>
static void launch(cvk_view frame, cvk_rect w, const cvk_ycc_image *im, const Mat9 &m, int width, int ga, long long chunks, const cvs::StripPlan &p,
                   const uint16_t *lut, hipStream_t s) {
    hipLaunchKernelGGL((k_ycc422_reconstruct<L, TABLE, LANES>), cvs::table_grid<LANES>(p.units, p.most), dim3(LANES), 0, s, frame, w, *im, m, width, ga,
                       (int)p.strip, (int)chunks, (int)p.units, lut);
}

template <int L>
static int dispatch(cvk_view frame, cvk_rect w, const cvk_ycc_image *im, const Mat9 &m, int width, int height, const uint16_t *lut, long long cus,
                    hipStream_t s) {
    constexpr int P = Lay<L>::pairs;
    const int ga = w.x0 / (2 * P);
    const long long chunks = ((long long)(w.x1 / (2 * P)) - ga + kRun) / kRun, rows = (long long)w.y1 - w.y0 + 1;
    cvs::StripPlan p;      // strips of rows
    if (!cvs::plan_strips(chunks, rows, (long long)width * (long long)height, true, cus, kMaxStrip, &p)) return (int)hipErrorInvalidValue;
    cvs::with_table(p.table, [&](auto TABLE, auto LANES) { launch<L, TABLE(), LANES()>(frame, w, im, m, width, ga, chunks, p, lut, s); });
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int cvk_ycc422_reconstruct(cvk_view frame, cvk_rect w, const cvk_ycc_image *im, int width, int height, int layout, const float mat[9],
                                      const uint16_t *lut, int cus, void *stream) {
    if (width < 2 || (width & 1) || height < 1) return (int)hipErrorInvalidValue;
    if (w.x1 < w.x0 || w.y1 < w.y0) return 0;
    if (w.x0 < 0 || w.y0 < 0 || w.x1 >= width || w.y1 >= height) return (int)hipErrorInvalidValue;
    const Mat9 m = cvs::mat9(mat);
    const long long n = cus > 0 ? cus : 256;
    hipStream_t s = (hipStream_t)stream;
    switch (layout) {
    case kP8: return dispatch<kP8>(frame, w, im, m, width, height, lut, n, s);
    case kP10: return dispatch<kP10>(frame, w, im, m, width, height, lut, n, s);
    case kUyvy: return dispatch<kUyvy>(frame, w, im, m, width, height, lut, n, s);
    case kV210: return dispatch<kV210>(frame, w, im, m, width, height, lut, n, s);
    default: return (int)hipErrorInvalidValue;
    }
}
