// ycc420_recon_ops.hip -- the 4:2:0 import edge: planar 8/10-bit, NV12 or P010 Y'CbCr -> half RGBA (include/canvas_ycc420.h).
//
//   k_ycc420_reconstruct   no reference code; the progressive form of k_mpeg2_reconstruct (mpeg2_recon_ops.hip) with the layout a
//                          template parameter and range, matrix and siting kernel arguments.  The contract is DESIGN.md "4:2:0
//                          Y'CbCr edges", restated (decode tables, matrix, store: ycc_edge.hpp):
//     decode     f = ((float)code - off) / div, correctly rounded; studio: off 16s / 128s, div 219s / 224s; full range: off 0 /
//                128s, div max; s = 1, max = 255 (8-bit) or s = 4, max = 1023 (10-bit).  A 256- or 1024-entry table per kind,
//                built in LDS by every workgroup with the same division.  PLANAR10 codes are bits 0-9, P010 codes bits 6-15
//     vertical   c = y >> 1; left and centre siting: c * 0.75 + (c - 1) * 0.25 on even rows, c * 0.75 + (c + 1) * 0.25 on odd ones;
//                top-left: p[c] on even rows, (p[c] + p[c + 1]) * 0.5 on odd ones; rows clamped to [0, H/2 - 1]
//     horizontal k = x >> 1; left and top-left siting: v(k) on even columns, (v(k) + v(k + 1)) * 0.5 on odd ones; centre:
//                v(k) * 0.75 + v(k - 1) * 0.25 on even columns, v(k) * 0.75 + v(k + 1) * 0.25 on odd ones; columns clamped
//     matrix     r = (yf*m0 + cb*m1) + cr*m2, likewise g and b, every product and sum rounded on its own: no FMA in either
//                arithmetic flavour (the unit is built once, not in FMA_KERN)
//     store      f2h_rz of r, g, b and 1.0; with a table, all four codes through it (the separate flavour's in both flavours)
// Both steps run as near * wn + far * wf with the weights handed in (cvk_ycc420_decode): weights 1 and 0 give the near value itself
// and 0.5, 0.5 give (a + b) * 0.5 bit for bit, since decoded chroma is finite, never -0 and far from the denormals.
// One lane owns one chroma column k, i.e. the luma column pair (2k, 2k + 1), over a strip of consecutive chroma rows c, i.e. luma
// row pairs (2c, 2c + 1).  v(k + 1) comes from the right-hand lane (__shfl_down): lane 63 of every wave only loads the column
// right of the wave's run to hand it on.  Centre siting needs v(k - 1) too (__shfl_up): lane 0 then loads the column left of the
// run and a wave writes 62 column pairs per row, 63 otherwise; every lane runs the same instructions.  A row pair needs one new
// chroma row (c + 1); rows c - 1 and c stay in a register ring, decoded, so each chroma row is loaded once per strip (twice at
// its ends).  The next pair's samples are loaded before the current pair is worked out.  The interleaved chroma of NV12
// and P010 is one 16- or 32-bit load per lane where it is aligned, sample by sample otherwise; one 16-byte store per row and lane
// where the pixel pair is aligned and inside the window, 8-byte stores otherwise.
// The 128 KiB table: staged into LDS or gathered from L2, by the raster's size (table_placement.hpp); or absent.
// Algorithmic bytes per pixel: 1.5 (8-bit) or 3 (10-bit) read, 8 written.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "ycc_edge.hpp"

namespace {

using cvs::kTable; using cvs::kTableL2; using cvs::kTableLds; using cvs::kTableNone;
using cvs::clampi; using cvs::load_two; using cvs::Mat9;
constexpr int kMaxStrip = 32;
enum { kP8 = CVK_420_PLANAR8, kP10 = CVK_420_PLANAR10, kNv12 = CVK_420_NV12, kP010 = CVK_420_P010 };
template <int L> struct Lay {
    static constexpr bool ten = L == kP10 || L == kP010;
    static constexpr bool semi = L == kNv12 || L == kP010;            // Cb and Cr interleaved in plane 1
    static constexpr int codes = ten ? 1024 : 256;
};

// luma columns (2k, 2k + 1) of row y
template <int L>
__device__ __forceinline__ uint32_t load_luma(const cvk_ycc_image &im, int y, int k) {
    constexpr int B = Lay<L>::ten ? 2 : 1;
    return load_two<Lay<L>::ten>(im.p[0] + (size_t)y * (size_t)im.stride[0] + (size_t)(2 * B) * (size_t)k);
}

// Cb and Cr of chroma row c, column k, packed like a luma pair
template <int L>
__device__ __forceinline__ uint32_t load_chroma(const cvk_ycc_image &im, int c, int k) {
    constexpr int B = Lay<L>::ten ? 2 : 1;
    if constexpr (Lay<L>::semi) return load_two<Lay<L>::ten>(im.p[1] + (size_t)c * (size_t)im.stride[1] + (size_t)(2 * B) * (size_t)k);
    const uint8_t *pb = im.p[1] + (size_t)c * (size_t)im.stride[1] + (size_t)B * (size_t)k;
    const uint8_t *pr = im.p[2] + (size_t)c * (size_t)im.stride[2] + (size_t)B * (size_t)k;
    if constexpr (Lay<L>::ten) return (uint32_t)*reinterpret_cast<const uint16_t *>(pb) | ((uint32_t)*reinterpret_cast<const uint16_t *>(pr) << 16);
    return (uint32_t)pb[0] | ((uint32_t)pr[0] << 8);
}

// the codes of a packed pair
template <int L> __device__ __forceinline__ uint32_t first(uint32_t r) { return L == kP8 || L == kNv12 ? (r & 0xFFu) : (L == kP10 ? (r & 0x3FFu) : ((r >> 6) & 0x3FFu)); }
template <int L> __device__ __forceinline__ uint32_t second(uint32_t r) { return L == kP8 || L == kNv12 ? ((r >> 8) & 0xFFu) : (L == kP10 ? ((r >> 16) & 0x3FFu) : (r >> 22)); }

struct Raw { uint32_t y0, y1, c; };           // luma pairs of rows 2c and 2c + 1, and the chroma of row c + 1 (clamped)

template <int L>
__device__ __forceinline__ void load_pair(const cvk_ycc_image &im, int c, int k, int ch, Raw &r) {
    r.y0 = load_luma<L>(im, 2 * c, k);
    r.y1 = load_luma<L>(im, 2 * c + 1, k);
    r.c = load_chroma<L>(im, min(c + 1, ch - 1), k);
}

struct Coef {
    Mat9 m;
    float y_off, y_div, c_off, c_div;
    float ve_n, ve_f, vo_n, vo_f, he_n, he_f, ho_n, ho_f;
};

// units: (strip of `strip` chroma rows, run of `run` chroma columns) over the window's chroma rows [ca, cb] and columns from ka;
// `chunks` runs per strip, so the waves of neighbouring units write neighbouring parts of the same rows.  A wave's unit is
// wave-uniform.  lead: 1 where lane 0 holds the column left of the run (centre siting), else 0; lanes lead .. lead + run - 1 write.
template <int L, int TABLE, int LANES>
__global__ __launch_bounds__(LANES) void k_ycc420_reconstruct(cvk_view frame, cvk_rect w, cvk_ycc_image im, Coef m, int width, int height, int ka,
                                                              int ca, int cb, int run, int lead, int strip, int chunks, int units,
                                                              const uint16_t *__restrict__ lut) {
    constexpr int kWaves = LANES / 64, N = Lay<L>::codes;
    __shared__ __attribute__((aligned(16))) uint16_t lds[TABLE == kTableLds ? kTable : 8];
    __shared__ float dec_y[N], dec_c[N];
    const uint16_t *t = TABLE == kTableLds ? lds : lut;
    const int lane = (int)(threadIdx.x & 63u), cw = width >> 1, ch = height >> 1, stride = (int)gridDim.x * kWaves;
    int u = (int)blockIdx.x * kWaves + (int)(threadIdx.x >> 6);
    Raw cur = { 0u, 0u, 0u };
    if (u < units) {                                       // the first unit's first pair: before the tables are built
        const int s = u / chunks;
        load_pair<L>(im, ca + s * strip, clampi(ka + (u - s * chunks) * run + lane - lead, 0, cw - 1), ch, cur);
    }
    if (TABLE == kTableLds) cvs::stage_table<LANES>(lds, lut);      // (the wait is the __syncthreads() below)
    cvs::build_decode<N, LANES>(dec_y, dec_c, m.y_off, m.y_div, m.c_off, m.c_div);
    __syncthreads();
    uint32_t alpha = 0x3C00u;                              // f2h_rz(1.0f)
    if constexpr (TABLE != kTableNone) alpha = t[0x3C00u];
    for (bool fresh = true; u < units; u += stride, fresh = false) {
        const int s = u / chunks;
        const int k = ka + (u - s * chunks) * run + lane - lead;
        const int kl = clampi(k, 0, cw - 1);               // the column this lane reads (k - 1 and k + 1 past an edge read the edge)
        const long long x = 2LL * k;
        const bool live = lane >= lead && lane < lead + run;
        const bool in0 = live && x >= w.x0 && x <= w.x1, in1 = live && x + 1 >= w.x0 && x + 1 <= w.x1;
        const int c0 = ca + s * strip, c1 = min(c0 + strip - 1, cb);
        // the ring: rows c - 1 and c, decoded
        const uint32_t ra = load_chroma<L>(im, max(c0 - 1, 0), kl), rm = load_chroma<L>(im, c0, kl);
        if (!fresh) load_pair<L>(im, c0, kl, ch, cur);
        float ub = dec_c[first<L>(ra)], ur = dec_c[second<L>(ra)], mb = dec_c[first<L>(rm)], mr = dec_c[second<L>(rm)];
        for (int c = c0; c <= c1; c++) {
            Raw nxt = cur;
            if (c < c1) load_pair<L>(im, c + 1, kl, ch, nxt);
            const float db = dec_c[first<L>(cur.c)], dr = dec_c[second<L>(cur.c)];
#pragma unroll
            for (int r = 0; r < 2; r++) {
                const int y = 2 * c + r;
                if (y < w.y0 || y > w.y1) continue;      // wave-uniform
                const float vb = r ? mb * m.vo_n + db * m.vo_f : mb * m.ve_n + ub * m.ve_f;
                const float vr = r ? mr * m.vo_n + dr * m.vo_f : mr * m.ve_n + ur * m.ve_f;
                const float nb = __shfl_down(vb, 1), nr = __shfl_down(vr, 1);
                // v(k - 1) only where its weight is not 0 (wave-uniform): a cross-lane move goes through the LDS hardware, which
                // the table gathers already keep busy
                float lb = vb, lr = vr;
                if (lead) { lb = __shfl_up(vb, 1); lr = __shfl_up(vr, 1); }
                const float eb = vb * m.he_n + lb * m.he_f, er = vr * m.he_n + lr * m.he_f;
                const float ob = vb * m.ho_n + nb * m.ho_f, orr = vr * m.ho_n + nr * m.ho_f;
                const uint32_t luma = r ? cur.y1 : cur.y0;
                const uint2 p0 = cvs::pixel<TABLE>(dec_y[first<L>(luma)], eb, er, m.m, t, alpha);
                const uint2 p1 = cvs::pixel<TABLE>(dec_y[second<L>(luma)], ob, orr, m.m, t, alpha);
                uint2 *o = reinterpret_cast<uint2 *>(frame.data) + (ptrdiff_t)(y - frame.fy0) * (ptrdiff_t)frame.pitch + (x - frame.fx0);
                cvs::store_pixel_pair<true>(o, p0, p1, in0, in1);
            }
            ub = mb; ur = mr; mb = db; mr = dr;
            cur = nxt;
        }
    }
}

template <int L, int TABLE, int LANES>
static void launch(cvk_view frame, cvk_rect w, const cvk_ycc_image *im, const Coef &m, int width, int height, int ka, int ca, int cb, int run, int lead,
                   long long chunks, const cvs::StripPlan &p, const uint16_t *lut, hipStream_t s) {
    hipLaunchKernelGGL((k_ycc420_reconstruct<L, TABLE, LANES>), cvs::table_grid<LANES>(p.units, p.most), dim3(LANES), 0, s, frame, w, *im, m, width, height,
                       ka, ca, cb, run, lead, (int)p.strip, (int)chunks, (int)p.units, lut);
}

template <int L>
static int dispatch(cvk_view frame, cvk_rect w, const cvk_ycc_image *im, const Coef &m, int width, int height, bool left_column, const uint16_t *lut,
                    long long cus, hipStream_t s) {
    const int ka = w.x0 >> 1, ca = w.y0 >> 1, cb = w.y1 >> 1, lead = left_column ? 1 : 0, run = 63 - lead;
    const long long chunks = ((long long)(w.x1 >> 1) - ka + run) / run, rows = (long long)cb - ca + 1;
    cvs::StripPlan p;      // strips of chroma rows
    if (!cvs::plan_strips(chunks, rows, (long long)width * (long long)height, lut != nullptr, cus, kMaxStrip, &p)) return (int)hipErrorInvalidValue;
    if (p.table == kTableNone) launch<L, kTableNone, cvs::kTableL2Lanes>(frame, w, im, m, width, height, ka, ca, cb, run, lead, chunks, p, lut, s);
    else
        cvs::with_table(p.table, [&](auto TABLE, auto LANES) {
            launch<L, TABLE(), LANES()>(frame, w, im, m, width, height, ka, ca, cb, run, lead, chunks, p, lut, s);
        });
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int cvk_ycc420_reconstruct(cvk_view frame, cvk_rect w, const cvk_ycc_image *im, int width, int height, int layout, const cvk_ycc420_decode *d,
                                      const uint16_t *lut, int cus, void *stream) {
    if (width < 2 || (width & 1) || height < 2 || (height & 1)) return (int)hipErrorInvalidValue;
    if (w.x1 < w.x0 || w.y1 < w.y0) return 0;
    if (w.x0 < 0 || w.y0 < 0 || w.x1 >= width || w.y1 >= height) return (int)hipErrorInvalidValue;
    const Coef m = { cvs::mat9(d->mat), d->y_off, d->y_div, d->c_off, d->c_div,
                     d->ve[0], d->ve[1], d->vo[0], d->vo[1], d->he[0], d->he[1], d->ho[0], d->ho[1] };
    const long long n = cus > 0 ? cus : 256;
    const bool lc = d->left_column != 0;
    hipStream_t s = (hipStream_t)stream;
    switch (layout) {
    case kP8: return dispatch<kP8>(frame, w, im, m, width, height, lc, lut, n, s);
    case kP10: return dispatch<kP10>(frame, w, im, m, width, height, lc, lut, n, s);
    case kNv12: return dispatch<kNv12>(frame, w, im, m, width, height, lc, lut, n, s);
    case kP010: return dispatch<kP010>(frame, w, im, m, width, height, lc, lut, n, s);
    default: return (int)hipErrorInvalidValue;
    }
}
