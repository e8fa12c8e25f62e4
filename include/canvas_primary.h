/*
 * canvas_primary.h -- the primary colour corrector of libcanvas_hip.so: per-channel 1D curves, a 3 x 4 matrix and per-channel 1D
 * curves again, fused into one pass over a frame.  An extension of include/canvas_hip.h (frames, boxes, streams and the coordinate
 * contract are its); the functions live in the same library.  Contract: DESIGN.md "Primary colour correction".
 */
#ifndef CANVAS_PRIMARY_H
#define CANVAS_PRIMARY_H

#include "canvas_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Primary colour correction (DESIGN.md "Primary colour correction").  A curve set: three 1D tables of K = size nodes, one per
 * colour channel, 2 <= K <= 4097; node 0 sits on domain_min[c] and node K-1 on domain_max[c], the nodes between are evenly spaced.
 * The device form is planar -- K floats of R, then K of G, then K of B -- on a 16-byte boundary, cvs_curves_bytes(K) = 12*K bytes;
 * cvs_curves_pack makes it on the host from K rows of (r g b), a 1D .cube's order, and refuses values that are not finite (the
 * device entries cannot look).  domain_min[c] < domain_max[c], both finite.  size 0: the stage is absent, its domains are not read.
 * The host forms scale[c] = (float)(K-1) / (domain_max[c] - domain_min[c]) once per call, in float.  Per pixel s of the window, in
 * f32 (a half widened exactly), every operation rounded on its own in BOTH arithmetic flavours:
 *     curve(T, c, s):  t = (s - domain_min[c]) * scale[c]
 *                      t = (t > 0) ? ((t < (float)(K-1)) ? t : (float)(K-1)) : 0       NaN -> 0, -Inf -> 0, +Inf -> K-1
 *                      i = min((int)t, K-2) ;  f = t - (float)i                        0 <= f <= 1
 *                      return T[c][i] * (1 - f) + T[c][i+1] * f                        (1-f, two products, one sum: four roundings)
 *     v = (s.r, s.g, s.b)
 *     if pre.size:            v.c = curve(pre,  c, v.c)                                for c in r, g, b
 *     if CVS_PRIMARY_MATRIX:  v.c = ((m[4c]*v.r + m[4c+1]*v.g) + m[4c+2]*v.b) + m[4c+3]   from the three values before the stage
 *     if post.size:           v.c = curve(post, c, v.c)
 *     out.rgb = v ;  out.a = s.a, code for code (NaN included)
 * f16 targets are truncated once, at the store.  Frames are un-premultiplied, so alpha plays no part.
 * Two properties of the form a*(1-f) + b*f:
 *   - an input on a node (t a whole number) returns that node's value exactly, the last node included (f = 1 gives a*0 + b);
 *   - an identity table on the domain [0, 1] returns every half code in [0, 1] bit for bit when K - 1 is a power of two (K = 2, 3,
 *     5, ..., 4097); it does not for K = 256, 1024 or 4096 (the f32 results differ at all three; at 1024 so do the halfs they are
 *     truncated to).  (a + f*(b-a) would lose the exact last node.)
 * target.current_window = source.current_window ∩ target.full_window; an empty source window is a success with an empty target
 * window.  target may be the source's buffer: the pass is pixelwise, so in place is bit for bit the out-of-place result.
 * Refused with -1 and a message, before the device is touched, with the target's window set empty and nothing written, in this
 * order: a NULL frame or p; no stage present; a flag bit other than CVS_PRIMARY_MATRIX; a present stage whose size is outside
 * 2..4097; a present stage whose domain is not finite or not ascending; a present stage whose table pointer is NULL or off the
 * 16-byte grid; a table pointer given for an absent stage; a matrix entry that is not finite, when the stage is present; a current
 * window outside its buffer; coordinates beyond +-CVS_MAX_COORD.  Any extent inside the bound is folded, never refused. */
enum { CVS_CURVES_MIN_SIZE = 2, CVS_CURVES_MAX_SIZE = 4097 };
typedef struct cvs_curves {              /* three 1D tables of `size` nodes, one per colour channel */
    int   size;                          /* K; 0: the stage is absent */
    float domain_min[3], domain_max[3];  /* the input values of node 0 and node K-1, per channel */
} cvs_curves;
#define CVS_PRIMARY_MATRIX 1
typedef struct cvs_primary {
    cvs_curves pre;                      /* stage 1 */
    float      matrix[12];               /* stage 2, row-major 3 x 4: out.c = m[4c]*r + m[4c+1]*g + m[4c+2]*b + m[4c+3] */
    cvs_curves post;                     /* stage 3 */
    int        flags;                    /* CVS_PRIMARY_MATRIX: stage 2 is present; no other bit */
} cvs_primary;
CVS_EXPORT size_t cvs_curves_bytes(int size);                                       /* 12*K; 0 + message when refused */
/* host only: K rows of (r g b) -> K floats of R, K of G, K of B; -1 + message for a size outside 2..4097 or a value that is not finite */
CVS_EXPORT int cvs_curves_pack(float *planar_host, const float *rgb_rows_host, int size);
/* target may be source's buffer, in place; pre_dev / post_dev: the device form of p->pre / p->post, NULL for an absent stage */
CVS_EXPORT int cvs_primary_f16_dev(rgba_frame_f16 *target, const rgba_frame_f16 *source, const cvs_primary *p,
                                   const float *pre_dev, const float *post_dev, cvs_stream_t s);
CVS_EXPORT int cvs_primary_f32_dev(rgba_frame_f32 *target, const rgba_frame_f32 *source, const cvs_primary *p,
                                   const float *pre_dev, const float *post_dev, cvs_stream_t s);

#ifdef __cplusplus
}
#endif
#endif
