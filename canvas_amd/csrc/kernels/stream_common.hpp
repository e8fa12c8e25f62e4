// stream_common.hpp -- pieces shared by the row streams (field_ops.hip, key_ops.hip, deinterlace_ops.hip): a one-wave workgroup owns 64 lanes x PIX
// columns over a segment of consecutive rows and walks down them.  Half RGBA pixels are 8 bytes; two per lane are one 16-byte
// access where every buffer involved puts the same column pairs on 16-byte boundaries (pair_view), one per lane otherwise.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"

namespace rowstream {

constexpr int kLanes = 64, kMinSeg = 8, kMaxSeg = 64, kWavesPerCu = 16;
// the most workgroups the launchers that fold put along y: within hipDeviceProp_t::maxGridSize[1] (65 536 on gfx950).  A window
// with more rows of workgroups than that is folded -- longer segments, a walk in the kernel, or one launch per band -- never
// refused (include/canvas_hip.h, the extent contract; DESIGN.md "Extents" has what the runtime does beyond it, and which
// launchers rest on that).
constexpr long long kMaxGridY = 65535;
typedef uint32_t v4 __attribute__((ext_vector_type(4)));
typedef uint32_t v2 __attribute__((ext_vector_type(2)));

// PIX pixels of one row as dwords (lo = g:r, hi = a:b per pixel); the second pixel's dwords stay zero when PIX == 1
template <int PIX>
__device__ __forceinline__ v4 load_px(const cvk_view &v, int x, int y) {
    const char *p = static_cast<const char *>(v.data) + ((long long)(y - v.fy0) * v.pitch + (x - v.fx0)) * 8;
    if (PIX == 2) return *reinterpret_cast<const v4 *>(p);
    const v2 t = *reinterpret_cast<const v2 *>(p);
    return v4{ t.x, t.y, 0u, 0u };
}

// m0 / m1: the first / second pixel lies inside the window
template <int PIX>
__device__ __forceinline__ void store_px(const cvk_view &v, int x, int y, v4 c, bool m0, bool m1) {
    char *p = static_cast<char *>(v.data) + ((long long)(y - v.fy0) * v.pitch + (x - v.fx0)) * 8;
    if (PIX == 2 && m0 && m1) { __builtin_nontemporal_store(c, reinterpret_cast<v4 *>(p)); return; }
    if (m0) __builtin_nontemporal_store(v2{ c.x, c.y }, reinterpret_cast<v2 *>(p));
    if (PIX == 2 && m1) __builtin_nontemporal_store(v2{ c.z, c.w }, reinterpret_cast<v2 *>(p) + 1);
}

// what every kernel starts with: the lane's columns and the segment's rows.  `w` is the window written, `xs` the column of lane
// 0 of the first workgroup (w.x0, or the pair boundary left of it), `seg` the rows per segment.
#define ROWSTREAM_LANE(w, xs, seg)                                                                  \
    const int x = (xs) + PIX * (int)(blockIdx.x * rowstream::kLanes + threadIdx.x);                 \
    const bool m0 = x >= (w).x0 && x <= (w).x1, m1 = PIX == 2 && x + 1 >= (w).x0 && x + 1 <= (w).x1; \
    if (!m0 && !m1) return;                                                                         \
    const int y0 = (w).y0 + (int)blockIdx.y * (seg), y1 = min(y0 + (seg) - 1, (w).y1);

// Two pixels per lane need every view to put the pairs (xs + 2k, xs + 2k + 1) on 16-byte boundaries in every row: base aligned,
// even pitch, xs - fx0 even.  xs is the pair boundary of `out` at or left of the window; the inputs must share its parity.
inline bool pair_view(const cvk_view &v, int xs) {
    return (reinterpret_cast<uintptr_t>(v.data) & 15u) == 0 && (v.pitch & 1) == 0 && (((long long)xs - v.fx0) & 1) == 0;
}

struct Shape { int pix, xs, seg; dim3 grid; };

// segments: enough one-wave workgroups for kWavesPerCu waves on every CU where the window has the rows for it, never shorter than
// kMinSeg rows (a kernel with a vertical window reads its seam rows twice).  `made`: the lanes of a wave that make columns (fewer
// than kLanes where the outermost lanes only load a neighbour's column and hand it on: deinterlace_ops.hip)
inline Shape shape(const cvk_rect &w, bool pairs, int out_fx0, int cus, int made = kLanes) {
    Shape s;
    s.pix = pairs ? 2 : 1;
    s.xs = pairs ? w.x0 - (int)(((long long)w.x0 - out_fx0) & 1) : w.x0;
    const long long cols = (long long)w.x1 - s.xs + 1, rows = (long long)w.y1 - w.y0 + 1;
    const long long chunks = (cols + s.pix * made - 1) / (s.pix * made);
    const long long waves = (long long)(cus > 0 ? cus : 256) * kWavesPerCu;
    long long seg = (rows * chunks + waves - 1) / waves;
    seg = seg < kMinSeg ? kMinSeg : (seg > kMaxSeg ? kMaxSeg : seg);
    if ((rows + seg - 1) / seg > kMaxGridY) seg = (rows + kMaxGridY - 1) / kMaxGridY;     // (from 65 535 x 64 + 1 rows on)
    s.seg = (int)seg;
    s.grid = dim3((unsigned)chunks, (unsigned)((rows + seg - 1) / seg), 1);
    return s;
}

inline bool rect_empty(const cvk_rect &r) { return r.x1 < r.x0 || r.y1 < r.y0; }

}  // namespace rowstream
