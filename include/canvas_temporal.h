/*
 * canvas_temporal.h -- the temporal noise reducer of libcanvas_hip.so: a frame averaged with the two or four frames around it in
 * time where nothing moved, left alone where something did.  With channels = CVS_MEDIAN_A it is the temporal matte smoother.  An
 * extension of include/canvas_hip.h (frames, boxes, streams and the coordinate contract are its; the channel bits are
 * include/canvas_median.h's); the function lives in the same library.  Contract: DESIGN.md "Temporal denoise".
 */
#ifndef CANVAS_TEMPORAL_H
#define CANVAS_TEMPORAL_H

#include "canvas_hip.h"
#include "canvas_median.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Motion-adaptive temporal denoise (DESIGN.md "Temporal denoise").  Removes what differs from frame to frame -- sensor noise,
 * grain, tape noise, the shimmer of a keyed matte -- and keeps full spatial detail where the picture is static: each pixel of
 * `cur` is averaged with the same pixel of the neighbouring frames, each neighbour weighted by how little moved between it and
 * `cur` in the 3 x 3 pixels around the pixel; a ramp of width `softness` lies between "averaged" and "untouched".
 * `prev2`, `prev1`, `next1` and `next2` (frames i - 2, i - 1, i + 1, i + 2 beside cur = frame i) may each be NULL or have an empty
 * current_window: that neighbour is absent (the start or end of a clip).
 * win = out.full_window ∩ cur.current_window; on success out.current_window = win, pixels outside win keep what they held.
 * All arithmetic in f32 on exactly widened halfs, every operation rounded on its own in BOTH arithmetic flavours, one truncation
 * at the store.  Neighbours are taken in the fixed order n = prev1, next1, prev2, next2.  For each present neighbour n and each
 * pixel (x, y) of win:
 *     m_n   the largest d = fabsf(cur(c, r).ch - n(c, r).ch) over rows r in y-1 .. y+1, columns c in x-1 .. x+1 and the SELECTED
 *           channels, of the samples (c, r) that lie inside cur.current_window ∩ n.current_window (out.full_window plays no part:
 *           tiles equal the whole); a NaN d is +inf.
 *     v_n   0 if (x, y) lies outside n.current_window or no sample counts; else softness > 0 ?
 *           1 - ramp((m_n - threshold) * inv_soft) : (m_n <= threshold ? 1 : 0), with inv_soft = 1.0f / softness and
 *           ramp(t) = (t < 1) ? ((t > 0) ? t : 0) : 1 (NaN -> 1), the chroma key's.
 *     w_n   w_prev1 = v_prev1, w_next1 = v_next1, w_prev2 = min(v_prev2, w_prev1), w_next2 = min(v_next2, w_next1): a farther
 *           frame never counts for more than the nearer one on its side, and where something passed through at i +- 1 averaging
 *           stops there.  An absent nearer frame has weight 0: prev2 without prev1 contributes nothing.
 * Per selected channel: acc = cur.ch; W = 1.0f; then in the order of n, for each neighbour with w_n > 0: t = w_n * n.ch;
 * acc = acc + t; W = W + w_n (a neighbour with w_n == 0 is left out, not multiplied: 0 x inf would be NaN); inv = 1.0f / W, one
 * correctly rounded IEEE divide per pixel; o = acc * inv, truncated to half.  If every weight is 0 the pixel is cur's codes,
 * whole; channels that `channels` does not select are cur's codes always.
 * With no neighbour present the call is the frame copy of cur over win.  The inputs may share buffers among themselves (all five
 * may be one frame); none that is present may be the output's buffer.  An empty cur.current_window or win: 0, an empty window,
 * nothing launched -- on a host with a device: the device is entered before the windows are looked at, as in deinterlace.c, so
 * without one the call fails with the library's "no CPU path" message like every other.
 * Refused with -1 and a message, before the device is touched, out.current_window set empty: out, cur or p NULL; channels 0 or
 * with a bit outside CVS_MEDIAN_ALL; flags != 0; a threshold that is not finite (a negative one is legal: "never static"); a
 * softness that is negative or not finite; out->data equal to a present input's data; an input's current_window outside its
 * buffer; a coordinate beyond +-CVS_MAX_COORD in any frame handed in, absent ones included. */
typedef struct cvs_temporal_denoise {
    float threshold;   /* largest difference to a neighbouring frame that still counts as "nothing moved" */
    float softness;    /* width of the ramp from averaged to untouched beyond threshold; 0 = hard switch */
    int   channels;    /* CVS_MEDIAN_R | _G | _B | _A mask of the channels denoised (and compared); at least one */
    int   flags;       /* none defined: 0 */
} cvs_temporal_denoise;

/* Operands that share a buffer: out as a present input is refused (the kernel reads a 3 x 3 neighbourhood of what another wave
 * may already have written: there is no in-place form); the five inputs may be one buffer, in any combination. */
CVS_EXPORT int cvs_temporal_denoise_f16_dev(rgba_frame_f16 *out,
        const rgba_frame_f16 *prev2, const rgba_frame_f16 *prev1, const rgba_frame_f16 *cur,
        const rgba_frame_f16 *next1, const rgba_frame_f16 *next2,
        const cvs_temporal_denoise *p, cvs_stream_t s);

#ifdef __cplusplus
}
#endif
#endif
