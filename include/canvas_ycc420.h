/*
 * canvas_ycc420.h -- the 4:2:0 Y'CbCr edges of libcanvas_hip.so for today's codecs: planar 8- and 10-bit (yuv420p, yuv420p10le),
 * NV12 and P010 <-> half RGBA, progressive.  The way in for what H.264, HEVC and AV1 decode to and for the surfaces hardware
 * decoders hand out, and the way out to their encoders.  An extension of include/canvas_hip.h (frames, boxes, coded_image, streams,
 * CVS_YCC_REC709 and the coordinate contract are its); the functions live in the same library.  Interlaced 4:2:0 stays with
 * cvs_reconstruct_mpeg2_dev / cvs_subsample_mpeg2_dev.  Contract, rounding included: DESIGN.md "4:2:0 Y'CbCr edges".
 */
#ifndef CANVAS_YCC420_H
#define CANVAS_YCC420_H

#include "canvas_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Layouts.  Everything is little-endian, strides are bytes, the raster's origin is frame coordinate (0, 0); width and height are
 * even and at least 2.
 *   CVS_420_PLANAR8    three planes: Y' W x H, Cb and Cr W/2 x H/2, one byte per sample; least strides W, W/2, W/2
 *   CVS_420_PLANAR10   three planes of uint16, the value in bits 0-9 (bits 10-15 ignored on the way in, written as 0 on the way
 *                      out); least strides 2W, W, W; bases and strides multiples of 2
 *   CVS_420_NV12       two planes: Y' W x H, then H/2 lines of the bytes Cb(k), Cr(k) interleaved; least strides W, W
 *   CVS_420_P010       NV12's shape in uint16, the value in bits 6-15 (bits 0-5 ignored on the way in, written as 0 on the way
 *                      out); least strides 2W, 2W; bases and strides multiples of 2
 * A larger stride or line count than the least is accepted (decoder surfaces are pitch-aligned) and the excess is never read or
 * written. */
enum { CVS_420_PLANAR8 = 0, CVS_420_PLANAR10 = 1, CVS_420_NV12 = 2, CVS_420_P010 = 3 };

/* Flags, beside CVS_YCC_REC709 of canvas_hip.h (neither matrix bit: Rec.601).
 *   CVS_YCC_REC2020          the non-constant-luminance Rec.2020 matrix (Kr 0.2627, Kb 0.0593); refused together with CVS_YCC_REC709
 *                              decode  R' = Y + 1.4746 Cr; G' = Y - 0.164553 Cb - 0.571353 Cr; B' = Y + 1.8814 Cb
 *                              encode  Y = 0.2627 0.6780 0.0593; Cb = -0.139630 -0.360370 0.5; Cr = 0.5 -0.459786 -0.040214
 *   CVS_YCC_FULL_RANGE       s = 1 (8-bit) or 4 (10-bit), max = 255 or 1023: decode Y / max and (C - 128s) / max in place of
 *                            (Y - 16s) / (219s) and (C - 128s) / (224s); encode q = Y and q = C + 128s / max; no [4, 1019] clamp
 *   CVS_YCC_SITING_CENTER    chroma in the middle of its 2 x 2 block (JPEG, MPEG-1)
 *   CVS_YCC_SITING_TOPLEFT   chroma co-sited with luma (2k, 2c) (UHD HDR streams).  Neither siting bit: left siting, the MPEG-2 /
 *                            H.264 / HEVC default, co-sited with even columns, halfway between rows 2c and 2c+1.  Both: refused
 *   CVS_YCC_NO_TRANSFER      no half table on the way in, no linear -> Rec.709 table on the way out: the frame holds the
 *                            non-linear R'G'B' codes, for a node that applies PQ, HLG or a camera curve itself
 * Any other bit is refused, CVS_YCC_PROGRESSIVE included: these edges are progressive by definition. */
enum { CVS_YCC_REC2020 = 4, CVS_YCC_FULL_RANGE = 8, CVS_YCC_SITING_CENTER = 16, CVS_YCC_SITING_TOPLEFT = 32, CVS_YCC_NO_TRANSFER = 64 };

/* How many planes `layout` takes (the return value: 3 or 2), and the least stride in bytes and the line count of each for a
 * width x height raster (entries beyond the layout's planes are set to 0).  Width and height even and >= 2 (and small enough for
 * the strides to fit an int); otherwise, or for an unknown layout, -1 and cvs_set_error.  Host only: no device is touched. */
CVS_EXPORT int cvs_ycc420_layout(int layout, int width, int height, int strides[3], int line_counts[3]);

/* Import: the samples of `image` (device pointers) -> the pixels of `frame` inside full_window ∩ raster, nothing else written;
 * current_window is emptied first and set to that box on success (0 with an empty window where the box is empty).
 *   decode     as above, correctly rounded; codes outside the legal range decode like any other
 *   vertical   c = y >> 1, rows clamped to [0, H/2 - 1].  Left and centre siting: near*0.75f + far*0.25f, near = p[c], far =
 *              p[c-1] (even y) or p[c+1] (odd y).  Top-left: p[c] (even y), (p[c] + p[c+1]) * 0.5f (odd y)
 *   horizontal k = x >> 1, columns clamped to [0, W/2 - 1].  Left and top-left siting: v(k) (even x), (v(k) + v(k+1)) * 0.5f (odd
 *              x).  Centre: near*0.75f + far*0.25f, near = v(k), far = v(k-1) (even x) or v(k+1) (odd x)
 *   matrix     r = (yf*m0 + cb*m1) + cr*m2, likewise g and b, every product and sum rounded on its own in both arithmetic flavours
 *   store      r, g, b and 1.0 truncated to half; all four codes through the Rec.709 -> linear (scene) half table unless
 *              CVS_YCC_NO_TRANSFER
 * PLANAR8, left siting, studio range, the transfer on, Rec.601 or Rec.709: byte for byte cvs_reconstruct_mpeg2_dev with
 * CVS_YCC_PROGRESSIVE.
 * Export: half RGBA -> samples.  The frame is only read; pixels outside current_window ∩ raster count as (0, 0, 0, 0), alpha is
 * ignored.  Every sample of the raster is written and nothing else: the least stride's bytes of each plane's lines.
 *   encode     r, g, b through the linear -> Rec.709 half table (unless CVS_YCC_NO_TRANSFER), widened; the matrix, no FMA
 *   chroma     from the colour differences E(y, x), the vertical step first, each left to right; row -1 reads row 0, column -1
 *              column 0:
 *                left      V = (E(2c) + E(2c+1)) * 0.5f;                    C = 0.25f*V(2k-1) + 0.5f*V(2k) + 0.25f*V(2k+1)
 *                centre    the same V;                                     C = (V(2k) + V(2k+1)) * 0.5f
 *                top-left  V = 0.25f*E(2c-1) + 0.5f*E(2c) + 0.25f*E(2c+1);  C as for left siting
 *   quantise   q = Y*(219s/max) + 16s/max or C*(224s/max) + 128s/max (full range: above); code = rint(clamp(q, 0, 1) * max), half
 *              to even, NaN -> 0; the 10-bit layouts in studio range then clamp the code to [4, 1019]
 * Round trips (samples -> import -> export): DESIGN.md "4:2:0 Y'CbCr edges".
 * Refused with -1 and cvs_set_error (import: an empty current_window), before any launch: a NULL frame or image; a coordinate
 * beyond +-CVS_MAX_COORD; a bad flag combination; an unknown layout; an odd width or height or one < 2; a NULL plane pointer; a
 * stride or line count below the least; a base or stride off its alignment; (export) a current_window outside the buffer. */
CVS_EXPORT int cvs_reconstruct_420_dev(rgba_frame_f16 *frame, const coded_image *image, int width, int height, int layout, int flags, cvs_stream_t stream);
CVS_EXPORT int cvs_subsample_420_dev(coded_image *image, const rgba_frame_f16 *frame, int width, int height, int layout, int flags, cvs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
