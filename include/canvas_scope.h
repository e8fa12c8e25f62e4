/*
 * canvas_scope.h -- video scopes of libcanvas_hip.so: a histogram, a waveform, an RGB parade or a vectorscope of an f16 frame as a
 * table of counters, and the picture of such a table.  An extension of include/canvas_hip.h (frames, boxes, streams, transfer
 * tables and the coordinate contract are its); the functions live in the same library.  Contract: DESIGN.md "Scopes".
 */
#ifndef CANVAS_SCOPE_H
#define CANVAS_SCOPE_H

#include "canvas_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Video scopes (DESIGN.md "Scopes"): counters over the display edge's bytes, so what is measured is what is exported or shown.
 * T is the byte table of (pre_lut, ramp) that the entries above use; a pixel of half codes (hr, hg, hb, ha) has the levels
 * r = T[hr], g = T[hg], b = T[hb], a = T[ha], and in integers (floor is a true floor):
 *     Y  = (13933*r + 46871*g + 4732*b + 32768) >> 16
 *     Cb = min(255, 128 + floor((-7509*r - 25259*g + 32768*b + 32768) / 65536))
 *     Cr = min(255, 128 + floor(( 32768*r - 29763*g -  3005*b + 32768) / 65536))
 * The measured set M is region ∩ frame.current_window, without the pixels whose byte a is 0 under CVS_SCOPE_SKIP_TRANSPARENT.
 * With W the width of `region`, a pixel at column x counts in output column c = floor((x - region.min.x) * columns / W).
 * Tables of uint32, written in full by every successful call (zeros first, on the same stream), +1 per pixel of M at:
 *     HISTOGRAM    [5][256]            [0][r] [1][g] [2][b] [3][a] [4][Y]
 *     WAVEFORM     [columns][256]      [c][Y]
 *     PARADE       [3][columns][256]   [0][c][r] [1][c][g] [2][c][b]
 *     VECTORSCOPE  [256][256]          [Cr][Cb]
 * An empty current window or an empty M is a success with a table of zeros.
 * cvs_scope_render_f16_dev turns a table into an opaque picture of cvs_scope_picture_size (columns x 256, 3*columns x 256 with
 * the panels R, G, B from the left, 256 x 256; the histogram has none) at `place`, which must be exactly that size:
 * win = place ∩ target.full_window becomes target.current_window, and picture pixel (i, j) from the top left, with n its
 * counter, holds v = fminf((float)n * gain, 1.0f), truncated to half:
 *     WAVEFORM     n = [i][255 - j]                          (v, v, v, 1)
 *     PARADE       n = [i / columns][i % columns][255 - j]   v in that panel's channel, 0 in the other two, alpha 1
 *     VECTORSCOPE  n = [255 - j][i]                          (v, v, v, 1)
 * It reads nothing of `region`.  Refused with -1 and a message, before anything is enqueued and with the table and the
 * target's pixels untouched (render also sets an empty target window): NULL pointers; a table off the 4-byte grid; an unknown
 * kind (HISTOGRAM for render); unknown flags; a pre_lut naming no table; a rendering_intent or a gain that is negative or
 * not finite; columns outside 1..CVS_SCOPE_MAX_COLUMNS (WAVEFORM, PARADE); an empty region; a current window outside its
 * buffer; a coordinate of a frame or of the region beyond +-CVS_MAX_COORD; a place of another size, or one no pixel of which lies
 * within +-CVS_MAX_COORD (a place is clipped: it may overhang the bound as it overhangs a target that lies on it); 2^32 or more
 * pixels to measure. */
enum { CVS_SCOPE_HISTOGRAM = 0, CVS_SCOPE_WAVEFORM = 1, CVS_SCOPE_PARADE = 2, CVS_SCOPE_VECTORSCOPE = 3 };
enum { CVS_SCOPE_SKIP_TRANSPARENT = 1 };
enum { CVS_SCOPE_MAX_COLUMNS = 4096 };
typedef struct cvs_scope {
    int   kind;
    int   pre_lut;            /* CVS_LUT_NONE or a transfer table, as for the display edge */
    float rendering_intent;   /* 0: the gamma-0.45 ramp (bytes of cvs_frame_to_bytes_dev, RGBA8); > 0: the widget's ramp (bytes of cvs_frame_to_rgba8_intent_dev) */
    int   columns;            /* WAVEFORM / PARADE: 1 .. CVS_SCOPE_MAX_COLUMNS; ignored by the other kinds */
    int   flags;
    box2i region;             /* the pixels measured, on the frame's plane */
} cvs_scope;
CVS_EXPORT size_t cvs_scope_count(const cvs_scope *p);                       /* counters in the table; 0 + message when p is refused */
CVS_EXPORT int cvs_scope_picture_size(const cvs_scope *p, v2i *size);        /* host only */
/* one frame per entry, against a table of counts: nothing here falls under canvas_hip.h "Operands that share a buffer" */
CVS_EXPORT int cvs_scope_counts_f16_dev(uint32_t *counts_dev, const rgba_frame_f16 *frame, const cvs_scope *p, cvs_stream_t s);
CVS_EXPORT int cvs_scope_render_f16_dev(rgba_frame_f16 *target, const box2i *place, const uint32_t *counts_dev, const cvs_scope *p, float gain, cvs_stream_t s);
/* host frame in, host table out, staged like video_frame_to_bytes */
CVS_EXPORT int video_scope_counts(uint32_t *counts_host, const rgba_frame_f16 *host_frame, const cvs_scope *p);

#ifdef __cplusplus
}
#endif
#endif
