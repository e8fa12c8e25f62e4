// unsharp_ops.hip -- unsharp mask: the register-window blur of blur_kernel.hpp with the mask as its
// epilogue, and the elementwise mask for blurs that other kernels made.
//
//   B = the A11 blur of the source (blur_kernel.hpp: x pass, then y pass, ascending taps, in the arithmetic flavour in force)
//   per colour channel, f32, every operation rounded on its own in BOTH flavours (no line of the reference to follow):
//       d = s - B;  out = fabsf(d) < threshold ? s : s + amount * d          (a NaN d fails the comparison: sharpened)
//   out.a = s.a;  f16 targets truncated at the store, once.
//
// k_unsharp is k_blur's sweep (one target column per lane, strips of W - (NT - 1) columns, segments of rows, the vertical window
// of NT horizontal sums in registers) and nothing of it is changed: same loads, same LDS rows, same sums in the same order.
// What the mask needs besides B is the source pixel under the output pixel, and the sweep has held it already: it is tap NT/2
// of the horizontal pass of the step NT/2 rows earlier (the lane's own column, read from the LDS row for that sum).  It is kept
// in `centre`, slots at compile-time indices like the ring's; a slot lives from the step that reads it from LDS to the step
// NT/2 later that emits its row, so NT/2 + 1 of the NT names are alive at any time.  No second read of the source, no
// intermediate frame: algorithmic bytes are the blur's, source pixel + target pixel.
// A kernel of its own and not a mode of k_blur: k_blur's instances (blur, blur + over, halving) keep their code objects and their
// register counts byte for byte, and this one carries none of their batch, epilogue and decimation arguments.
// One column per lane: the form that takes every window geometry (blur_pair_ops.hip needs pair-aligned windows, so a two-column
// mask could only ever be a second form beside this one).
//
// k_unsharp_combine: out = mask(source, blurred) over a rectangle, one pixel per lane, for the tap lists the sweep has no
// instance for (even counts, more than 13 taps, non-finite taps, pinned table kernels): the blur goes to an f32 frame first.
// Same expression on the same f32 values: the same codes as the fused kernel wherever both can run.
#include "blur_kernel.hpp"

namespace {

// the mask of one channel pair; `alpha`: the second element is alpha, passed through
template <bool ALPHA>
__device__ __forceinline__ f32x2 mask2(f32x2 s, f32x2 b, float amount, float threshold) {
    const f32x2 d = s - b;
    const f32x2 m = d * amount;
    const f32x2 sharp = s + m;
    f32x2 o;
    o.x = __builtin_fabsf(d.x) < threshold ? s.x : sharp.x;
    if constexpr (ALPHA) o.y = s.y;
    else o.y = __builtin_fabsf(d.y) < threshold ? s.y : sharp.y;
    return o;
}

template <int NT, int W, bool HALF>
__global__ __launch_bounds__(W) void k_unsharp(cvk_unsharp_params up) {
    constexpr int C = NT / 2, OUTW = W - NT + 1, PITCH = W + 16;
    static_assert((NT & 1) && NT >= 3 && NT <= 13, "odd tap counts up to 13");
    __shared__ float4 rowbuf[2][PITCH];
    const int lane = threadIdx.x;
    const int xo = up.tx0 + (int)blockIdx.x * OUTW;          // first target column of the strip
    const int sfirst = xo - C;                               // first source column of the strip
    const int tcol = xo + lane;                              // the target column this lane produces
    const bool out_live = lane < OUTW && tcol <= up.tx1;
    const int ta = up.ty0 + (int)blockIdx.y * up.rows_per_wg;
    const int tb = min(ta + up.rows_per_wg - 1, up.ty1);
    const int ys0 = ta - C;                                  // first source row the segment needs
    const int steps = (tb - ta) + NT;

    float w[NT];
#pragma unroll
    for (int k = 0; k < NT; k++) w[k] = up.taps[k];
    const float amount = up.amount, threshold = up.threshold;

    constexpr size_t PX = HALF ? 8 : 16;
    const size_t srow = (size_t)up.source.pitch * PX, trow = (size_t)up.target.pitch * PX;
    const int scol = sfirst + lane;                          // the source column this lane loads
    const bool col_live = scol >= up.sx0 && scol <= up.sx1;
    const char *sbase = reinterpret_cast<const char *>(up.source.data) + (ptrdiff_t)(scol - up.source.fx0) * (ptrdiff_t)PX;
    char *tbase = reinterpret_cast<char *>(up.target.data) + (ptrdiff_t)(tcol - up.target.fx0) * (ptrdiff_t)PX;

    if (lane < PITCH - W) { rowbuf[0][W + lane] = make_float4(0.f, 0.f, 0.f, 0.f); rowbuf[1][W + lane] = make_float4(0.f, 0.f, 0.f, 0.f); }

    Px ring[NT], centre[NT];
#pragma unroll
    for (int k = 0; k < NT; k++) ring[k].rg = ring[k].ba = centre[k].rg = centre[k].ba = f32x2{ 0.0f, 0.0f };

    auto fetch_row = [&](int ys, bool wanted) {
        return fetch<HALF>(sbase, srow, ys, up.source.fy0, wanted && col_live && ys >= up.sy0 && ys <= up.sy1);
    };
    Raw<HALF> cur = fetch_row(ys0, true);
    Raw<HALF> nxt = fetch_row(ys0 + 1, steps > 1);

    for (int i0 = 0; i0 < steps; i0 += NT) {
        // NT steps with the ring and centre slots as compile-time constants (a runtime index would send them to scratch)
        auto step = [&](auto jc) -> bool {
            constexpr int j = decltype(jc)::value;
            const int i = i0 + j;
            if (i >= steps) return false;                     // uniform over the workgroup
            const bool emits = i >= NT - 1;                   // uniform
            const int t = ta + (i - (NT - 1));                // the target row this step completes
            // two rows ahead goes out now; this row's data was requested two steps ago
            const Raw<HALF> far = fetch_row(ys0 + i + 2, i + 2 < steps);
            float4 *buf = rowbuf[i & 1];
            buf[lane] = widen<HALF>(cur);
            cur = nxt;
            nxt = far;
            __syncthreads();
            float4 v[NT];
#pragma unroll
            for (int k = 0; k < NT; k++) v[k] = buf[lane + k];
            // v[C] is source pixel (tcol, ys0 + i): the centre of the row that step i + C emits
            centre[j].rg = f32x2{ v[C].x, v[C].y };
            centre[j].ba = f32x2{ v[C].z, v[C].w };
            f32x2 rg, ba;
            if constexpr (cvs::kContract) {
                // the clang build's t += s * c: one fused multiply-add per tap (the first: fma(s, c, 0) = the product)
                rg = f32x2{ v[0].x, v[0].y } * w[0]; ba = f32x2{ v[0].z, v[0].w } * w[0];
#pragma unroll
                for (int k = 1; k < NT; k++) { rg = cvs::madd(f32x2{ v[k].x, v[k].y }, w[k], rg); ba = cvs::madd(f32x2{ v[k].z, v[k].w }, w[k], ba); }
            } else {
                // all products first, then the two add chains interleaved (blur_kernel.hpp: a packed add right behind the
                // multiply it needs costs a hazard slot per tap); rounding and order of the additions as written
                f32x2 prg[NT], pba[NT];
#pragma unroll
                for (int k = 0; k < NT; k++) { prg[k] = f32x2{ v[k].x, v[k].y } * w[k]; pba[k] = f32x2{ v[k].z, v[k].w } * w[k]; }
                __builtin_amdgcn_sched_barrier(0);
                rg = prg[0]; ba = pba[0];
#pragma unroll
                for (int k = 1; k < NT; k++) { rg = rg + prg[k]; ba = ba + pba[k]; }
            }
            ring[j].rg = rg;
            ring[j].ba = ba;
            if (emits) {
                // ring[(j+1) % NT] is the oldest row = tap 0
                f32x2 org, oba;
                if constexpr (cvs::kContract) {
                    org = ring[(j + 1) % NT].rg * w[0]; oba = ring[(j + 1) % NT].ba * w[0];
#pragma unroll
                    for (int k = 1; k < NT; k++) { const Px &p = ring[(j + 1 + k) % NT]; org = cvs::madd(p.rg, w[k], org); oba = cvs::madd(p.ba, w[k], oba); }
                } else {
                    f32x2 qrg[NT], qba[NT];
#pragma unroll
                    for (int k = 0; k < NT; k++) { const Px &p = ring[(j + 1 + k) % NT]; qrg[k] = p.rg * w[k]; qba[k] = p.ba * w[k]; }
                    __builtin_amdgcn_sched_barrier(0);
                    org = qrg[0]; oba = qba[0];
#pragma unroll
                    for (int k = 1; k < NT; k++) { org = org + qrg[k]; oba = oba + qba[k]; }
                }
                const Px &s = centre[(j + NT - C) % NT];      // written C steps ago
                org = mask2<false>(s.rg, org, amount, threshold);
                oba = mask2<true>(s.ba, oba, amount, threshold);
                if (out_live) {
                    char *o = tbase + (size_t)(t - up.target.fy0) * trow;
                    if constexpr (HALF) *reinterpret_cast<uint2 *>(o) = make_uint2(cvs::f2h_rz2(org.x, org.y), cvs::f2h_rz2(oba.x, oba.y));
                    else *reinterpret_cast<float4 *>(o) = make_float4(org.x, org.y, oba.x, oba.y);
                }
            }
            return true;
        };
        each_slot(step, std::make_integer_sequence<int, NT>{});
    }
}

template <int NT, int W, bool HALF>
int launch_unsharp(cvk_unsharp_params up, int cus, hipStream_t s) {
    constexpr int OUTW = W - NT + 1;
    const int cols = up.tx1 - up.tx0 + 1, rows = up.ty1 - up.ty0 + 1;
    const int strips = (cols + OUTW - 1) / OUTW;
    static std::atomic<int> cached{ 0 };            // (several threads may launch at once)
    int mine = cached.load(std::memory_order_relaxed);
    if (!mine) { mine = resident_per_cu(k_unsharp<NT, W, HALF>, W); cached.store(mine, std::memory_order_relaxed); }
    if (up.rows_per_wg <= 0) {
        // as many workgroups as the chip holds at once, all in one wave of the grid (blur_kernel.hpp launch)
        int segs = (mine * cus) / strips;
        if (segs < 1) segs = 1;
        int r = (rows + segs - 1) / segs;
        if (r < NT - 1) r = NT - 1;                 // halo rows cost at most as much as the rows produced
        if (r > rows) r = rows;
        up.rows_per_wg = r;
    }
    dim3 grid((unsigned)strips, (unsigned)((rows + up.rows_per_wg - 1) / up.rows_per_wg), 1);
    hipLaunchKernelGGL((k_unsharp<NT, W, HALF>), grid, dim3(W), 0, s, up);
    return (int)hipGetLastError();
}

template <int W, bool HALF>
int pick_unsharp(const cvk_unsharp_params *up, int cus, hipStream_t s) {
    switch (up->ntaps) {
    case 3:  return launch_unsharp<3, W, HALF>(*up, cus, s);
    case 5:  return launch_unsharp<5, W, HALF>(*up, cus, s);
    case 7:  return launch_unsharp<7, W, HALF>(*up, cus, s);
    case 9:  return launch_unsharp<9, W, HALF>(*up, cus, s);
    case 11: return launch_unsharp<11, W, HALF>(*up, cus, s);
    case 13: return launch_unsharp<13, W, HALF>(*up, cus, s);
    }
    return (int)hipErrorInvalidValue;
}

// one pixel per lane over the rectangle r; rows beyond the grid's are walked by the same workgroups
template <bool HALF>
__global__ __launch_bounds__(256) void k_unsharp_combine(cvk_view out, cvk_view src, cvk_view blurred, cvk_rect r, float amount, float threshold) {
    const int x = r.x0 + (int)(blockIdx.x * 256 + threadIdx.x);
    if (x > r.x1) return;
    for (int y = r.y0 + (int)blockIdx.y; y <= r.y1; y += (int)gridDim.y) {
        const size_t si = (size_t)(y - src.fy0) * (size_t)src.pitch + (size_t)(x - src.fx0);
        const size_t bi = (size_t)(y - blurred.fy0) * (size_t)blurred.pitch + (size_t)(x - blurred.fx0);
        const size_t oi = (size_t)(y - out.fy0) * (size_t)out.pitch + (size_t)(x - out.fx0);
        Raw<HALF> raw;
        if constexpr (HALF) raw.v = static_cast<const uint2 *>(src.data)[si]; else raw.v = static_cast<const float4 *>(src.data)[si];
        const float4 s = widen<HALF>(raw), b = static_cast<const float4 *>(blurred.data)[bi];
        const f32x2 org = mask2<false>(f32x2{ s.x, s.y }, f32x2{ b.x, b.y }, amount, threshold);
        const f32x2 oba = mask2<true>(f32x2{ s.z, s.w }, f32x2{ b.z, b.w }, amount, threshold);
        if constexpr (HALF) static_cast<uint2 *>(out.data)[oi] = make_uint2(cvs::f2h_rz2(org.x, org.y), cvs::f2h_rz2(oba.x, oba.y));
        else static_cast<float4 *>(out.data)[oi] = make_float4(org.x, org.y, oba.x, oba.y);
    }
}

}  // namespace

extern "C" int cvk_unsharp_supported(int ntaps) { return (ntaps & 1) && ntaps >= 3 && ntaps <= 13; }

extern "C" int cvk_unsharp(const cvk_unsharp_params *up, int cus, void *stream) {
    if (up->tx1 < up->tx0 || up->ty1 < up->ty0) return 0;
    if (!cvk_unsharp_supported(up->ntaps)) return (int)hipErrorInvalidValue;
    // strip width as the blur's: 256 lanes unless the frame is so narrow that 128 wastes fewer
    const bool narrow = up->tx1 - up->tx0 + 1 <= 128;
    hipStream_t s = (hipStream_t)stream;
    if (up->half) return narrow ? pick_unsharp<128, true>(up, cus, s) : pick_unsharp<256, true>(up, cus, s);
    return narrow ? pick_unsharp<128, false>(up, cus, s) : pick_unsharp<256, false>(up, cus, s);
}

extern "C" int cvk_unsharp_combine(cvk_view out, cvk_view src, cvk_view blurred, cvk_rect r, int half, float amount, float threshold, void *stream) {
    if (r.x1 < r.x0 || r.y1 < r.y0) return 0;
    const long long cols = (long long)r.x1 - r.x0 + 1, rows = (long long)r.y1 - r.y0 + 1;
    // at most 32 768 workgroups along y, the rows beyond walked in the kernel: a fold kept as defence (the runtime was measured
    // to take grid.y = rows past 65 535, DESIGN.md "Extents"); tests/test_extents_gpu.py runs it at 65 535, 65 536 and 70 001 rows
    dim3 grid((unsigned)((cols + 255) / 256), (unsigned)(rows < 32768 ? rows : 32768), 1);
    if (half) hipLaunchKernelGGL(k_unsharp_combine<true>, grid, dim3(256), 0, (hipStream_t)stream, out, src, blurred, r, amount, threshold);
    else hipLaunchKernelGGL(k_unsharp_combine<false>, grid, dim3(256), 0, (hipStream_t)stream, out, src, blurred, r, amount, threshold);
    return (int)hipGetLastError();
}
