/*
 * canvas_lut3d.h -- the 3D colour lookup table of libcanvas_hip.so: a lattice of N x N x N colours applied to a frame by
 * tetrahedral interpolation.  An extension of include/canvas_hip.h (frames, boxes, streams and the coordinate contract are its);
 * the functions live in the same library.  Contract: DESIGN.md "3D LUT".
 */
#ifndef CANVAS_LUT3D_H
#define CANVAS_LUT3D_H

#include "canvas_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 3D LUT (DESIGN.md "3D LUT").  Lattice: N = size, 2 <= N <= 65, N^3 nodes, red fastest -- the node of lattice index
 * (ir, ig, ib) is at ir + N*(ig + N*ib), the order of a .cube file.  The device form is 4 floats per node (R, G, B, unused) on a
 * 16-byte boundary, cvs_lut3d_bytes(N) = 16*N^3 bytes; cvs_lut3d_pack makes it on the host from N^3*3 floats and refuses values
 * that are not finite (the device entries cannot look).  domain_min[c] < domain_max[c], both finite.
 * The host forms scale[c] = (float)(N-1) / (domain_max[c] - domain_min[c]) once per call, in float.  Per pixel s of the window,
 * in f32 (a half widened exactly), every operation rounded on its own in BOTH arithmetic flavours:
 *     for c in r, g, b:
 *         t   = (s.c - domain_min[c]) * scale[c]
 *         t   = (t > 0) ? ((t < (float)(N-1)) ? t : (float)(N-1)) : 0          NaN -> 0, -Inf -> 0, +Inf -> N-1
 *         i_c = min((int)t, N-2) ;  f_c = t - (float)i_c                       0 <= f_c <= 1
 *     order the channels by descending f; a tie goes to r before g, and g before b (a stable sort on (-f, channel))
 *         -> axes e1, e2, e3 with f1 >= f2 >= f3
 *     V0 = L[i] ; V1 = L[i + e1] ; V2 = L[i + e1 + e2] ; V3 = L[i + (1,1,1)]
 *     w0 = 1 - f1 ; w1 = f1 - f2 ; w2 = f2 - f3 ; w3 = f3
 *     out.c = ((V0.c*w0 + V1.c*w1) + V2.c*w2) + V3.c*w3                        for c in r, g, b
 *     out.a = s.a, code for code (NaN included)
 * f16 targets are truncated once at the store.  Frames are un-premultiplied, so alpha plays no part.
 * target.current_window = source.current_window ∩ target.full_window; an empty source window is a success with an empty target
 * window; target may be the source frame itself.  A colour on a lattice point gives that node's value exactly; an identity
 * lattice on the domain [0, 1] is the identity on every half code in [0, 1] when N - 1 is a power of two (2, 3, 5, 9, 17, 33,
 * 65), and only then.
 * Refused with -1 and a message, nothing enqueued and the target's window set empty: NULL pointers; a lattice off the 16-byte
 * grid; a size outside 2..65; a domain that is not finite or not ascending; unknown flags; a current window outside its buffer;
 * coordinates beyond +-CVS_MAX_COORD. */
enum { CVS_LUT3D_MIN_SIZE = 2, CVS_LUT3D_MAX_SIZE = 65 };
typedef struct cvs_lut3d {
    int   size;                          /* N */
    float domain_min[3], domain_max[3];  /* the colours of lattice index 0 and N-1, per channel */
    int   flags;                         /* 0 */
} cvs_lut3d;
CVS_EXPORT size_t cvs_lut3d_bytes(int size);                                        /* 16*N^3; 0 + message when refused */
/* host only: N^3 * 3 floats, red fastest -> N^3 * 4 floats (the fourth 0); -1 + message for a size outside 2..65 or a value that is not finite */
CVS_EXPORT int cvs_lut3d_pack(float *nodes4_host, const float *rgb_host, int size);
/* target may be source's buffer, in place: canvas_hip.h "Operands that share a buffer" */
CVS_EXPORT int cvs_lut3d_f16_dev(rgba_frame_f16 *target, const rgba_frame_f16 *source, const float *lattice_dev, const cvs_lut3d *p, cvs_stream_t s);
CVS_EXPORT int cvs_lut3d_f32_dev(rgba_frame_f32 *target, const rgba_frame_f32 *source, const float *lattice_dev, const cvs_lut3d *p, cvs_stream_t s);

#ifdef __cplusplus
}
#endif
#endif
