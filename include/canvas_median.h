/*
 * canvas_median.h -- the despeckle of libcanvas_hip.so: a 3 x 3 or 5 x 5 median per channel, the library's rank filter.  An
 * extension of include/canvas_hip.h (frames, boxes, streams and the coordinate contract are its); the functions live in the same
 * library.  Contract: DESIGN.md "Median".
 */
#ifndef CANVAS_MEDIAN_H
#define CANVAS_MEDIAN_H

#include "canvas_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Median (DESIGN.md "Median"): removes what is wrong with single pixels -- dust, dead and hot pixels, drop-outs, the specks a
 * keyer leaves in a matte -- without moving an edge.  A selection: every output code is one of the input codes, nothing is ever
 * rounded or truncated, so both arithmetic flavours give the same bytes.
 * Window: win = target.full_window ∩ source.current_window; on success target.current_window = win, pixels of target outside win
 * keep what they held.  An empty source.current_window or win: 0, an empty window, nothing launched.
 * Neighbourhood: with cur = source.current_window and n = 2 * radius + 1, the n * n samples
 *     source(clamp(x + dx, cur.min.x, cur.max.x), clamp(y + dy, cur.min.y, cur.max.y)),  |dx|, |dy| <= radius
 * of a pixel (x, y) of win: replicated edges, always exactly n * n samples; target.full_window plays no part, so a tile of a
 * picture computed from the source grown by `radius` equals the same tile of the whole.
 * Order: per channel, a total order on the samples' BIT PATTERNS, not float compares, so that NaNs, both zeros and subnormals
 * are deterministic: the key of a half code h is (h & 0x8000) ? (uint16)~h : h | 0x8000, compared unsigned, that of an f32
 * pattern the same with 32 bits.  -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN.  The key is a bijection: equal keys are equal
 * codes and the result is unique.  med[ch] is the sample whose key is the (n * n + 1) / 2-th smallest: the 5th of 9, the 13th of 25.
 * Output: channels that `channels` does not select are source(x, y)'s codes.
 *     threshold == 0: the selected channels are med[ch]'s codes.
 *     threshold > 0:  d = the largest fabsf(s[ch] - med[ch]) over the SELECTED channels; for f16 the subtraction is in f32 on
 *         exactly widened halfs, for f32 on the values themselves, one subtraction rounded on its own.  If !(d <= threshold)
 *         (a NaN d, such as inf - inf or a NaN sample, counts as beyond) all selected channels take med; otherwise the pixel
 *         keeps source(x, y) whole.  The decision is per pixel, not per channel: a repaired speck leaves no colour fringe.
 * Refused with -1 and a message, before the device is touched, target.current_window set empty, nothing written: target, source
 * or p NULL; radius not 1 or 2; channels 0 or with a bit outside CVS_MEDIAN_ALL; flags != 0; a threshold that is negative or not
 * finite; target->data == source->data (the kernel gathers: there is no in-place form); source.current_window outside its
 * buffer; a coordinate beyond +-CVS_MAX_COORD (everything here is integer: the wide bound). */
#define CVS_MEDIAN_R 1
#define CVS_MEDIAN_G 2
#define CVS_MEDIAN_B 4
#define CVS_MEDIAN_A 8
#define CVS_MEDIAN_COLOUR 7
#define CVS_MEDIAN_ALL 15
typedef struct cvs_median {
    int   radius;      /* 1: 3 x 3, 2: 5 x 5 */
    float threshold;   /* 0: every pixel takes the median; > 0: only pixels that differ from it by more than this */
    int   channels;    /* CVS_MEDIAN_* mask of the channels filtered; the others pass code for code */
    int   flags;       /* none defined: 0 */
} cvs_median;

/* the target as the source's buffer is refused, and there is one input: canvas_hip.h "Operands that share a buffer" */
CVS_EXPORT int cvs_median_f16_dev(rgba_frame_f16 *target, const rgba_frame_f16 *source, const cvs_median *p, cvs_stream_t s);
CVS_EXPORT int cvs_median_f32_dev(rgba_frame_f32 *target, const rgba_frame_f32 *source, const cvs_median *p, cvs_stream_t s);

#ifdef __cplusplus
}
#endif
#endif
