// scope_ops.hip -- video scopes: histogram, waveform, RGB parade and vectorscope of an f16 frame, and the picture of a table.
//
// No reference code (the reference has no scope).  The contract is DESIGN.md "Scopes" and include/canvas_scope.h, restated here.
// A scope is the display edge's sibling (display_ops.hip): it reads the same 8 B/px and looks every half up in the same 64 KiB
// byte table `t`, r = t[hr], g = t[hg], b = t[hb], a = t[ha].  What it writes is counters.  Integer work throughout:
//     Y  = (13933*r + 46871*g + 4732*b + 32768) >> 16
//     Cb = min(255, 128 + ((-7509*r - 25259*g + 32768*b + 32768) >> 16))        (arithmetic shift: a true floor)
//     Cr = min(255, 128 + (( 32768*r - 29763*g -  3005*b + 32768) >> 16))
// and a pixel at column x counts in output column c = (x - region_x0) * columns / region_w (64-bit; 32-bit where it fits).
//
// k_scope_count, the first reduction of the code base.  Shape:
//   - the byte table sits in LDS as in k_display (64 KiB), beside the workgroup's private counters (Shape<KIND>, below):
//       histogram    5 x 256 counters,        5 KiB: 512 lanes, two workgroups per CU
//       waveform     16 output columns x 256, 16 KiB: 512 lanes, two workgroups per CU
//       parade       3 x 16 columns x 256,    48 KiB: 1024 lanes, one workgroup per CU
//       vectorscope  86 rows of Cr x 256,     86 KiB: 1024 lanes, one workgroup per CU
//   - a work item is (strip, row group).  A strip is what the counters hold: 16 output columns of a waveform or a parade -- the
//     item reads only the pixel columns that fall into them --, the whole picture for the histogram, and for the vectorscope a
//     band of 86 rows of Cr: its 256 KiB of counters do not fit, so each of three bands reads ALL the pixels and counts those
//     whose Cr falls into it (3 x 8 B/px read; every counter stays private, whatever the picture).  The rows of a strip are
//     dealt to several row groups, so that the chip is filled whatever the picture's shape.  A grid of at most one workgroup per
//     slot of the chip strides over the items; the items are never a few more than the slots;
//   - per item: zero the counters, count with LDS atomics that return nothing, then add the non-zero counters to the table in
//     global memory with atomics that return nothing (consecutive lanes, consecutive counters).  Integer adds: the result does
//     not depend on the order;
//   - every add goes through count(): the lanes of a wave that share the first live lane's counter go in as ONE add of their
//     number, and whoever is left adds 1 alone.  A flat picture, where all 64 lanes hit one counter, is one add per wave instead
//     of 64 serialised ones; noise pays two ballots and a compare;
//   - lanes are laid out lx (a power of two from 64 up) along x by LANES / lx rows, so a wave reads one run of a row.  Two pixels
//     per lane in one 16-byte load where base and pitch keep pairs aligned (a pair cut by the edge of the measured set is
//     loaded by its half that lies inside: nothing outside the set is read), else one pixel in 8 bytes.  Non-temporal loads.
//   - every loop has the same trip count in all lanes of a workgroup (lanes outside the set are masked, not absent): count()
//     needs the whole wave.
// Bound: see DESIGN.md "Scopes", Measured.  Algorithmic bytes: 8 B/px read (the vectorscope 24), a few KiB written.
//
// k_scope_render: a plain stream, one counter per pixel, v = fminf((float)n * gain, 1), truncated to half, non-temporal stores.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "pixel_math.hpp"

namespace {

constexpr int kTable = 65536;
typedef uint32_t v4 __attribute__((ext_vector_type(4)));
typedef uint32_t v2 __attribute__((ext_vector_type(2)));

// lanes per workgroup, workgroups per CU, counters per workgroup and what a strip is made of (output columns; rows of Cr)
template <int KIND> struct Shape { static constexpr int lanes = 512, per_cu = 2, planes = 5, strip = 1; };      // histogram
template <> struct Shape<CVK_SCOPE_WAVEFORM> { static constexpr int lanes = 512, per_cu = 2, planes = 1, strip = 16; };
template <> struct Shape<CVK_SCOPE_PARADE> { static constexpr int lanes = 1024, per_cu = 1, planes = 3, strip = 16; };
template <> struct Shape<CVK_SCOPE_VECTORSCOPE> { static constexpr int lanes = 1024, per_cu = 1, planes = 1, strip = 86; };

struct scope_job {
    cvk_view src;
    cvk_rect m;                 // the measured rectangle, inside src
    uint32_t *counts;
    const uint8_t *table;
    long long region_w;
    int region_x0, columns, skip;
    int strip0, nstrips;        // the first strip that m reaches, how many it reaches
    int groups, rows;           // row groups per strip, rows per group
    int lx_log2;
};

struct render_job {
    cvk_view out;
    cvk_rect win;
    const uint32_t *counts;
    int px0, py0, columns;
    float gain;
};

__device__ __forceinline__ void stage(uint8_t *lds, const uint8_t *table) {
    const uint4 *t = reinterpret_cast<const uint4 *>(table);
    uint4 *d = reinterpret_cast<uint4 *>(lds);
    for (int i = threadIdx.x; i < kTable / 16; i += blockDim.x) d[i] = t[i];
    __syncthreads();
}

// +1 at bins[idx] (LDS) for every lane with `on` set.  All 64 lanes of the wave call together.
__device__ __forceinline__ void count(uint32_t *bins, uint32_t idx, bool on) {
    const unsigned long long live = __ballot(on);
    if (live == 0) return;
    const int leader = __ffsll(live) - 1;
    const uint32_t first = (uint32_t)__builtin_amdgcn_readlane((int)idx, leader);
    const unsigned long long same = __ballot(on && idx == first);
    if ((int)__lane_id() == leader) (void)__hip_atomic_fetch_add(bins + first, (uint32_t)__popcll(same), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (on && idx != first) (void)__hip_atomic_fetch_add(bins + idx, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__device__ __forceinline__ uint32_t luma(uint32_t r, uint32_t g, uint32_t b) { return (13933u * r + 46871u * g + 4732u * b + 32768u) >> 16; }
__device__ __forceinline__ uint32_t chroma_b(int r, int g, int b) { const int v = 128 + ((-7509 * r - 25259 * g + 32768 * b + 32768) >> 16); return (uint32_t)(v < 255 ? v : 255); }
__device__ __forceinline__ uint32_t chroma_r(int r, int g, int b) { const int v = 128 + ((32768 * r - 29763 * g - 3005 * b + 32768) >> 16); return (uint32_t)(v < 255 ? v : 255); }

// one pixel (lo = g:r, hi = a:b) into the counters of a strip that starts at c0 and holds nc output columns (rows of Cr); c: the
// pixel's output column within the strip
template <int KIND>
__device__ __forceinline__ void tally(uint32_t *bins, const uint8_t *t, uint32_t lo, uint32_t hi, int c, int c0, int nc, bool on, int skip) {
    const uint32_t r = t[lo & 0xFFFFu], g = t[lo >> 16], b = t[hi & 0xFFFFu];
    if (KIND == CVK_SCOPE_HISTOGRAM || skip) {
        const uint32_t a = t[hi >> 16];
        if (skip) on = on && a != 0;
        if (KIND == CVK_SCOPE_HISTOGRAM) count(bins + 768, a, on);
    }
    if (KIND == CVK_SCOPE_HISTOGRAM) {
        count(bins, r, on);
        count(bins + 256, g, on);
        count(bins + 512, b, on);
        count(bins + 1024, luma(r, g, b), on);
    } else if (KIND == CVK_SCOPE_WAVEFORM) {
        count(bins, (uint32_t)c * 256u + luma(r, g, b), on);
    } else if (KIND == CVK_SCOPE_PARADE) {
        count(bins, (uint32_t)c * 256u + r, on);
        count(bins, (uint32_t)(nc + c) * 256u + g, on);
        count(bins, (uint32_t)(2 * nc + c) * 256u + b, on);
    } else {
        const uint32_t row = chroma_r((int)r, (int)g, (int)b) - (uint32_t)c0;       // (below the band: wraps to a large number)
        count(bins, row * 256u + chroma_b((int)r, (int)g, (int)b), on && row < (uint32_t)nc);
    }
}

template <int KIND, bool PAIR>
__global__ __launch_bounds__(Shape<KIND>::lanes) void k_scope_count(scope_job j) {
    constexpr int kLanes = Shape<KIND>::lanes, kPlanes = Shape<KIND>::planes, kStrip = Shape<KIND>::strip, kStep = PAIR ? 2 : 1;
    constexpr bool kColumns = KIND == CVK_SCOPE_WAVEFORM || KIND == CVK_SCOPE_PARADE;        // a strip is a run of pixel columns
    __shared__ __attribute__((aligned(16))) uint8_t t[kTable];
    __shared__ uint32_t bins[kPlanes * kStrip * 256];
    stage(t, j.table);
    const int lx = 1 << j.lx_log2, tx = (int)threadIdx.x & (lx - 1), ty = (int)threadIdx.x >> j.lx_log2, ly = kLanes >> j.lx_log2;
    const bool fits32 = (unsigned long long)j.region_w * (unsigned long long)j.columns < (1ull << 32);
    const uint2 *data = reinterpret_cast<const uint2 *>(j.src.data);
    const int items = j.nstrips * j.groups;
    for (int item = (int)blockIdx.x; item < items; item += (int)gridDim.x) {
        const int strip = j.strip0 + item / j.groups, group = item % j.groups;
        const int c0 = strip * kStrip, nc = min(kStrip, j.columns - c0), used = kPlanes * nc * 256;
        for (int i = (int)threadIdx.x; i < used; i += kLanes) bins[i] = 0u;
        __syncthreads();
        // the columns of the measured rectangle that fall into the strip: output column c starts at region_x0 + ceil(c * W / columns)
        int xs = j.m.x0, xe = j.m.x1;
        if (kColumns) {
            const long long first = (long long)j.region_x0 + ((long long)c0 * j.region_w + j.columns - 1) / j.columns;
            const long long last = (long long)j.region_x0 + ((long long)(c0 + nc) * j.region_w + j.columns - 1) / j.columns - 1;
            const long long lo = first > xs ? first : xs, hi = last < xe ? last : xe;
            xs = lo <= hi ? (int)lo : 0;                         // (no pixel of the strip: an empty run)
            xe = lo <= hi ? (int)hi : -1;
        }
        const int y0 = j.m.y0 + group * j.rows, y1 = min(j.m.y1, y0 + j.rows - 1);
        // (with pairs: from the even pixel of the buffer's row at or before xs)
        const int xa = PAIR ? xs - ((xs - j.src.fx0) & 1) : xs;
        for (int xb = xa; xs <= xe && xb <= xe; xb += lx * kStep) {
            const int x = xb + tx * kStep;
            const bool in0 = x >= xs && x <= xe, in1 = PAIR && x + 1 >= xs && x + 1 <= xe;
            int col0 = 0, col1 = 0;
            if (kColumns) {
                const unsigned long long d0 = (unsigned long long)((long long)x - j.region_x0), d1 = d0 + 1;
                if (fits32) {
                    if (in0) col0 = (int)((uint32_t)d0 * (uint32_t)j.columns / (uint32_t)j.region_w) - c0;
                    if (in1) col1 = (int)((uint32_t)d1 * (uint32_t)j.columns / (uint32_t)j.region_w) - c0;
                } else {
                    if (in0) col0 = (int)(d0 * (unsigned long long)j.columns / (unsigned long long)j.region_w) - c0;
                    if (in1) col1 = (int)(d1 * (unsigned long long)j.columns / (unsigned long long)j.region_w) - c0;
                }
            }
            for (int yb = y0; yb <= y1; yb += ly) {
                const int y = yb + ty;
                const bool on0 = in0 && y <= y1, on1 = in1 && y <= y1;
                v4 q = { 0u, 0u, 0u, 0u };
                if (on0 || on1) {
                    const uint2 *p = data + (size_t)(y - j.src.fy0) * (size_t)j.src.pitch + (size_t)(x - j.src.fx0);
                    if (PAIR && on0 && on1) q = __builtin_nontemporal_load(reinterpret_cast<const v4 *>(p));
                    else if (on0) { const v2 a = __builtin_nontemporal_load(reinterpret_cast<const v2 *>(p)); q.x = a.x; q.y = a.y; }
                    else { const v2 a = __builtin_nontemporal_load(reinterpret_cast<const v2 *>(p + 1)); q.z = a.x; q.w = a.y; }
                }
                tally<KIND>(bins, t, q.x, q.y, col0, c0, nc, on0, j.skip);
                if (PAIR) tally<KIND>(bins, t, q.z, q.w, col1, c0, nc, on1, j.skip);
            }
        }
        __syncthreads();
        // counter i of the strip is [plane][c][level] over nc columns (rows of Cr); in the table its plane has j.columns of them
        for (int i = (int)threadIdx.x; i < used; i += kLanes) {
            const uint32_t v = bins[i];
            const int plane = i / (nc * 256);
            if (v) (void)__hip_atomic_fetch_add(j.counts + (size_t)plane * (size_t)j.columns * 256u + (size_t)c0 * 256u + (size_t)(i - plane * nc * 256), v,
                                                __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
    }
}

template <int KIND>
__global__ __launch_bounds__(256) void k_scope_render(render_job j) {
    const uint32_t w = (uint32_t)(j.win.x1 - j.win.x0 + 1), h = (uint32_t)(j.win.y1 - j.win.y0 + 1), n = w * h;
    uint2 *data = reinterpret_cast<uint2 *>(j.out.data);
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const uint32_t row = i / w, col = i - row * w;
        const int x = j.win.x0 + (int)col, y = j.win.y0 + (int)row;
        const uint32_t pi = (uint32_t)(x - j.px0), pj = (uint32_t)(y - j.py0);
        // waveform [pi][255 - pj]; parade [panel][pi % columns][255 - pj], the panels side by side: the same index; vectorscope [255 - pj][pi]
        const uint32_t at = KIND == CVK_SCOPE_VECTORSCOPE ? (255u - pj) * 256u + pi : pi * 256u + (255u - pj);
        const float v = __builtin_fminf((float)j.counts[at] * j.gain, 1.0f);
        cvs::px32 o = { v, v, v, 1.0f };
        if (KIND == CVK_SCOPE_PARADE) {
            const uint32_t panel = pi / (uint32_t)j.columns;
            o.r = panel == 0u ? v : 0.0f; o.g = panel == 1u ? v : 0.0f; o.b = panel == 2u ? v : 0.0f;
        }
        const uint2 code = cvs::narrow(o);
        const v2 out = { code.x, code.y };
        __builtin_nontemporal_store(out, reinterpret_cast<v2 *>(data + (size_t)(y - j.out.fy0) * (size_t)j.out.pitch + (size_t)(x - j.out.fx0)));
    }
}

// the launch of one kind: j holds the frame, the rectangle, the region and the columns; the rest is worked out here
template <int KIND>
void launch_count(scope_job j, int cus, hipStream_t s) {
    constexpr int kLanes = Shape<KIND>::lanes, kStrip = Shape<KIND>::strip;
    constexpr bool kColumns = KIND == CVK_SCOPE_WAVEFORM || KIND == CVK_SCOPE_PARADE;
    const long long w = (long long)j.m.x1 - j.m.x0 + 1, h = (long long)j.m.y1 - j.m.y0 + 1;
    if (kColumns) {      // the strips whose output columns the rectangle reaches
        const long long c_first = ((long long)j.m.x0 - j.region_x0) * j.columns / j.region_w, c_last = ((long long)j.m.x1 - j.region_x0) * j.columns / j.region_w;
        j.strip0 = (int)(c_first / kStrip);
        j.nstrips = (int)(c_last / kStrip) - j.strip0 + 1;
    } else {
        j.strip0 = 0;
        j.nstrips = (j.columns + kStrip - 1) / kStrip;           // 1; the vectorscope's three bands of Cr
    }
    // Enough pixels per item to be worth a 64 KiB table load; no more items than the chip has slots unless the strips alone are
    // more (a few items beyond the slots would have a few workgroups do twice the work of the others).
    const long long per_wg = (long long)kLanes * 8, most = (long long)(cus > 0 ? cus : 256) * Shape<KIND>::per_cu;
    long long want = (w * h * (kColumns ? 1 : j.nstrips) + per_wg - 1) / per_wg;
    want = want < 1 ? 1 : want > most ? most : want;
    long long groups = want / j.nstrips;
    groups = groups < 1 ? 1 : groups > h ? h : groups;
    j.rows = (int)((h + groups - 1) / groups);
    j.groups = (int)((h + j.rows - 1) / j.rows);
    const long long items = (long long)j.nstrips * j.groups;
    // the widest strip, in pixels, decides how the lanes are laid out
    const bool pair = (((uintptr_t)j.src.data) & 15u) == 0 && (j.src.pitch & 1) == 0;
    long long span = kColumns ? ((long long)kStrip * j.region_w + j.columns - 1) / j.columns + 1 : w;
    if (span > w) span = w;
    const long long across = pair ? span / 2 + 1 : span;
    j.lx_log2 = 6;
    while ((1ll << j.lx_log2) < across && (1 << j.lx_log2) < kLanes) j.lx_log2++;
    dim3 grid((unsigned)(items < most ? items : most)), block(kLanes);
    if (pair) hipLaunchKernelGGL((k_scope_count<KIND, true>), grid, block, 0, s, j);
    else hipLaunchKernelGGL((k_scope_count<KIND, false>), grid, block, 0, s, j);
}

}  // namespace

extern "C" int cvk_scope_counts(uint32_t *counts, cvk_view src, cvk_rect m, const uint8_t *table, int kind, int region_x0, long long region_w,
                                int columns, int skip_transparent, int cus, void *stream) {
    if (m.x1 < m.x0 || m.y1 < m.y0) return 0;
    if (kind < CVK_SCOPE_HISTOGRAM || kind > CVK_SCOPE_VECTORSCOPE) return (int)hipErrorInvalidValue;
    if (kind == CVK_SCOPE_HISTOGRAM || kind == CVK_SCOPE_VECTORSCOPE) {
        columns = kind == CVK_SCOPE_VECTORSCOPE ? 256 : 1;       // (the vectorscope's rows of Cr stand where the output columns stand)
        region_x0 = m.x0;
        region_w = (long long)m.x1 - m.x0 + 1;
    }
    // the rectangle lies inside the region and inside the buffer
    if (columns < 1 || columns > 4096 || region_w < 1 || m.x0 < region_x0 || (long long)m.x1 - region_x0 >= region_w) return (int)hipErrorInvalidValue;
    if (m.x0 < src.fx0 || m.y0 < src.fy0 || m.x1 > src.fx1 || m.y1 > src.fy1) return (int)hipErrorInvalidValue;
    scope_job j;
    j.src = src; j.m = m; j.counts = counts; j.table = table;
    j.region_w = region_w; j.region_x0 = region_x0; j.columns = columns; j.skip = skip_transparent ? 1 : 0;
    j.strip0 = 0; j.nstrips = 1; j.groups = 1; j.rows = 1; j.lx_log2 = 6;
    hipStream_t s = (hipStream_t)stream;
    if (kind == CVK_SCOPE_HISTOGRAM) launch_count<CVK_SCOPE_HISTOGRAM>(j, cus, s);
    else if (kind == CVK_SCOPE_WAVEFORM) launch_count<CVK_SCOPE_WAVEFORM>(j, cus, s);
    else if (kind == CVK_SCOPE_PARADE) launch_count<CVK_SCOPE_PARADE>(j, cus, s);
    else launch_count<CVK_SCOPE_VECTORSCOPE>(j, cus, s);
    return (int)hipGetLastError();
}

extern "C" int cvk_scope_render(cvk_view out, cvk_rect win, int px0, int py0, const uint32_t *counts, int kind, int columns, float gain, void *stream) {
    if (win.x1 < win.x0 || win.y1 < win.y0) return 0;
    const int panels = kind == CVK_SCOPE_PARADE ? 3 : 1;
    if (kind != CVK_SCOPE_WAVEFORM && kind != CVK_SCOPE_PARADE && kind != CVK_SCOPE_VECTORSCOPE) return (int)hipErrorInvalidValue;
    if (kind == CVK_SCOPE_VECTORSCOPE) columns = 256;
    // the window lies inside the picture and inside the buffer
    if (columns < 1 || columns > 4096 || win.x0 < px0 || win.y0 < py0 || (long long)win.x1 - px0 >= (long long)panels * columns || (long long)win.y1 - py0 >= 256) return (int)hipErrorInvalidValue;
    if (win.x0 < out.fx0 || win.y0 < out.fy0 || win.x1 > out.fx1 || win.y1 > out.fy1) return (int)hipErrorInvalidValue;
    render_job j;
    j.out = out; j.win = win; j.counts = counts; j.px0 = px0; j.py0 = py0; j.columns = columns; j.gain = gain;
    const size_t n = (size_t)(win.x1 - win.x0 + 1) * (size_t)(win.y1 - win.y0 + 1);
    dim3 grid((unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096)), block(256);
    hipStream_t s = (hipStream_t)stream;
    if (kind == CVK_SCOPE_WAVEFORM) hipLaunchKernelGGL(k_scope_render<CVK_SCOPE_WAVEFORM>, grid, block, 0, s, j);
    else if (kind == CVK_SCOPE_PARADE) hipLaunchKernelGGL(k_scope_render<CVK_SCOPE_PARADE>, grid, block, 0, s, j);
    else hipLaunchKernelGGL(k_scope_render<CVK_SCOPE_VECTORSCOPE>, grid, block, 0, s, j);
    return (int)hipGetLastError();
}
