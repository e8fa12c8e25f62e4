/*
 * canvas_deinterlace.h -- the motion-adaptive deinterlacer of libcanvas_hip.so: a woven frame made into a whole picture with
 * the frames before and after it, the first entry that looks at neighbouring frames in time.  An extension of
 * include/canvas_hip.h (frames, boxes, streams, cvs_field_to_frame_f16_dev and the coordinate contract are its); the function
 * lives in the same library.  Contract: DESIGN.md "Adaptive deinterlace".
 */
#ifndef CANVAS_DEINTERLACE_H
#define CANVAS_DEINTERLACE_H

#include "canvas_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Motion-adaptive deinterlace (DESIGN.md "Adaptive deinterlace").  Where nothing moved between `cur` and its neighbours in time
 * the rows of the other field are kept (full vertical resolution); where something moved they are interpolated from the kept
 * field, as cvs_field_to_frame_f16_dev does everywhere; a ramp of width `softness` lies between.
 * `prev` and `next` may each be NULL or have an empty current_window: that neighbour is absent (the start or end of a clip).
 * win = out.full_window ∩ cur.current_window; on success out.current_window = win, pixels outside win keep what they held.
 * All arithmetic in f32 on exactly widened halfs, every operation rounded on its own in BOTH arithmetic flavours, one truncation
 * at the store.  Row parity is that of the absolute coordinate, y & 1.  For a row y of win:
 *     (y & 1) == field:  the codes of cur, copied.
 *     every other row, per pixel (x, y):
 *       sp  per channel what cvs_field_to_frame_f16_dev makes there: rows y-1 and y+1 of cur, each used if it lies inside
 *           cur.current_window (out.full_window plays no part); both: upper * 0.5f + lower * 0.5f; one: its values; none: zeros
 *       wv  cur(x, y)
 *       m   the largest d = fabsf(cur(c, r).ch - n(c, r).ch) over the present neighbours n, rows r in y-1 .. y+1, columns c in
 *           x-1 .. x+1 and the four channels (alpha is a channel like the others), of the samples (c, r) that lie inside
 *           cur.current_window ∩ n.current_window (again out.full_window plays no part: tiles equal the whole); a NaN d is +inf.
 *           Only rows of equal parity in different frames are compared, so no field order has to be known.
 *       k   1 if no sample counts; else softness > 0 ? ramp((m - threshold) * inv_soft) : (m <= threshold ? 0 : 1), with
 *           inv_soft = 1.0f / softness and ramp(t) = (t < 1) ? ((t > 0) ? t : 0) : 1 (NaN -> 1), the chroma key's
 *       k == 0: the codes of wv;  k == 1: exactly what cvs_field_to_frame_f16_dev writes there (the mean truncated, or the single
 *       row's codes, or zeros);  otherwise per channel e = sp - wv; f = k * e; r = wv + f, truncated to half.
 * With both neighbours absent the call is cvs_field_to_frame_f16_dev's, bit for bit.  The inputs may be one frame (prev == cur is
 * legal); none may be the output's buffer.  An empty cur.current_window or win: 0, an empty window, nothing launched.
 * Refused with -1 and a message, before the device is touched, out.current_window set empty: out, cur or p NULL; field not 0 or 1;
 * flags != 0; a threshold that is not finite (a negative one is legal: "never static"); a softness that is negative or not finite;
 * out->data equal to a present input's data; an input's current_window outside its buffer; a coordinate beyond +-CVS_MAX_COORD. */
typedef struct cvs_deinterlace_adaptive {
    int   field;        /* 0: keep the even rows, 1: keep the odd rows (parity of the absolute y, y & 1) */
    float threshold;    /* largest difference that still counts as "nothing moved" */
    float softness;     /* width of the ramp from kept (weave) to interpolated; 0 = hard switch */
    int   flags;        /* none defined: 0 */
} cvs_deinterlace_adaptive;

/* out as one of the inputs is refused, the inputs may be one buffer: canvas_hip.h "Operands that share a buffer" */
CVS_EXPORT int cvs_deinterlace_adaptive_f16_dev(rgba_frame_f16 *out, const rgba_frame_f16 *prev, const rgba_frame_f16 *cur,
                                                const rgba_frame_f16 *next, const cvs_deinterlace_adaptive *p, cvs_stream_t s);

#ifdef __cplusplus
}
#endif
#endif
