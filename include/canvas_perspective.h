/*
 * canvas_perspective.h -- the corner pin of libcanvas_hip.so: a perspective (projective) warp of a layer of un-premultiplied
 * pixels, and the host arithmetic that goes with it.  An extension of include/canvas_hip.h (frames, boxes, streams, the filter
 * constants of cvs_transform and the coordinate contract are its); the functions live in the same library.
 * Contract: DESIGN.md "Corner pin".
 */
#ifndef CANVAS_PERSPECTIVE_H
#define CANVAS_PERSPECTIVE_H

#include "canvas_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Corner pin (DESIGN.md "Corner pin").  h holds the nine coefficients of the TARGET -> SOURCE map, row by row, both sides
 * measured from an origin carried here: a pinned layer far from (0, 0) gets the bits of the same layer at the origin.
 * S = source.current_window, S' = S - source_origin.  Per pixel (X, Y) of the window written, in f32 (a half widened exactly),
 * every operation rounded on its own in BOTH arithmetic flavours:
 *     x = (float)(X - target_origin.x) ;  y = (float)(Y - target_origin.y)          subtracted as ints; exact by the span rule
 *     nu = (h0*x + h1*y) + h2 ;  nv = (h3*x + h4*y) + h5 ;  w = (h6*x + h7*y) + h8
 *     if not (w > 0):  out = (0, 0, 0, 0)                  on or beyond the vanishing line (the plane folds back there), and NaN
 *     u = nu / w ;  v = nv / w                                                        IEEE divides
 *     then NEAREST / BILINEAR exactly as cvs_transform (canvas_hip.h) with in() tested against S' and source(i, j) the pixel
 *     at (source_origin.x + i, source_origin.y + j): the copy rule on a sample (a == 0 and b == 0), alpha-weighted taps in
 *     the order (0,0), (1,0), (0,1), (1,1), A != 0 ? (R/A, G/A, B/A, A) : 0, one truncation at an f16 store, and a tap outside
 *     S' is never read.  CATMULL_ROM likewise: the sixteen taps, the copy rule and the clamp rule of cvs_transform.
 * With h6 = h7 = 0 and h8 = 1, w is exactly 1 and u = nu; with both origins (0, 0) as well the entries give cvs_transform's bytes.
 * The entry writes win = cvs_perspective_target_window(p, S, target.full_window) and sets target.current_window = win; pixels
 * outside win keep what they held.  An empty S or win: 0, an empty window, nothing launched.
 * Refused with -1 and a message, before the device is touched, the target's window set empty: a NULL argument; a source window
 * outside its buffer; a filter other than the three; flags != 0; an h[k] that is not finite; a determinant of h (in double) that is
 * zero or not finite; a coordinate beyond +-CVS_MAX_COORD; any coordinate of target.full_window - target_origin or of
 * S - source_origin (formed in 64 bit) beyond +-CVS_PERSPECTIVE_MAX_SPAN; target->data == source->data. */
enum { CVS_PERSPECTIVE_MAX_SPAN = 1 << 23 };
typedef struct cvs_perspective {
    float h[9];              /* TARGET -> SOURCE, both relative to the origins below */
    int   target_origin[2];  /* x, y */
    int   source_origin[2];
    int   filter;            /* CVS_TRANSFORM_NEAREST / CVS_TRANSFORM_BILINEAR / CVS_TRANSFORM_CATMULL_ROM */
    int   flags;             /* none defined: 0 */
} cvs_perspective;
/* a target that is the source's buffer is refused: canvas_hip.h "Operands that share a buffer" */
CVS_EXPORT int cvs_perspective_f32_dev(rgba_frame_f32 *target, const rgba_frame_f32 *source, const cvs_perspective *p, cvs_stream_t s);
CVS_EXPORT int cvs_perspective_f16_dev(rgba_frame_f16 *target, const rgba_frame_f16 *source, const cvs_perspective *p, cvs_stream_t s);
/* Host arithmetic, in double, every operation rounded on its own; no device needed.
 * _from_quad: the map that puts the real rectangle source_rect = (x0, y0, x1, y1), x1 > x0 and y1 > y0, onto the quad whose
 *     corners are where the rectangle's top-left, top-right, bottom-right and bottom-left land.  Integer coordinates are sample
 *     positions: a box2i's outer edges are min - 1/2 .. max + 1/2.  The origins are the floor of the quad's mean and of the
 *     rectangle's centre.  0; 1 with *p untouched for a quad that is not strictly convex (nothing to draw); -1 + message for a
 *     NULL, a value that is not finite, a rectangle that is not ascending or an unknown filter.  A parallelogram gives an affine
 *     map (h6 = h7 = 0, h8 = 1) by cvs_transform_from_parts' formulas, otherwise w is +1 at the quad's centre.
 * _target_window: the target pixels a tap inside source_current can reach, within target_full -- all of target_full when part
 *     of the window lies on or beyond the vanishing line.
 * _source_window: the source pixels the taps of target_window can touch (the whole +-2^30 range when a corner has w <= 0);
 *     not clipped to anything. */
CVS_EXPORT int cvs_perspective_from_quad(const double source_rect[4], const double quad[4][2], int filter, cvs_perspective *p);
CVS_EXPORT int cvs_perspective_target_window(const cvs_perspective *p, const box2i *source_current, const box2i *target_full, box2i *win);
CVS_EXPORT int cvs_perspective_source_window(const cvs_perspective *p, const box2i *target_window, box2i *need);

#ifdef __cplusplus
}
#endif
#endif
