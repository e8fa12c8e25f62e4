/*
 * canvas_ycc422.h -- the 4:2:2 Y'CbCr edges of libcanvas_hip.so: planar 8- and 10-bit (yuv422p, yuv422p10le), packed UYVY
 * (2vuy) and packed v210 <-> half RGBA.  The way in for what ProRes, DNxHD/HR, DVCPRO50/HD, XDCAM HD422 and x264 High 4:2:2
 * decode to and for what SDI cards and the uncompressed QuickTime/AVI codecs speak, and the way out for a 10-bit master.  An
 * extension of include/canvas_hip.h (frames, boxes, coded_image, streams, the CVS_YCC_* flags and the coordinate contract are
 * its); the functions live in the same library.  Contract, rounding included: DESIGN.md "4:2:2 Y'CbCr edges".
 */
#ifndef CANVAS_YCC422_H
#define CANVAS_YCC422_H

#include "canvas_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Layouts.  Everything is little-endian, strides are bytes, the raster's origin is frame coordinate (0, 0).  4:2:2 subsamples
 * chroma along x only, co-sited with the even columns: there is no siting to choose and no rule for the height.
 *   CVS_422_PLANAR8    three planes: Y' W x H, Cb and Cr W/2 x H, one byte per sample; least strides W, W/2, W/2
 *   CVS_422_PLANAR10   three planes of uint16, the value in bits 0-9; least strides 2W, W, W; bases and strides multiples of 2
 *   CVS_422_UYVY       one plane; per pixel pair k the bytes Cb(k), Y'(2k), Cr(k), Y'(2k+1); least stride 2W
 *   CVS_422_V210       one plane; per 6 pixels four 32-bit words of three 10-bit fields (bits 0-9, 10-19, 20-29):
 *                        word 0: Cb0 Y0 Cr0   word 1: Y1 Cb1 Y2   word 2: Cr1 Y3 Cb2   word 3: Y4 Cr2 Y5
 *                      least stride 16 * ceil(W / 6); base and stride multiples of 4
 * A larger stride or line count than the least is accepted and the excess is never read or written. */
enum { CVS_422_PLANAR8 = 0, CVS_422_PLANAR10 = 1, CVS_422_UYVY = 2, CVS_422_V210 = 3 };

/* How many planes `layout` takes (the return value: 3 or 1), and the least stride in bytes and the line count of each for a
 * width x height raster (entries beyond the layout's planes are set to 0).  Width even and >= 2, height >= 1 (and small enough
 * for the strides to fit an int); otherwise, or for an unknown layout, -1 and cvs_set_error.  Host only: no device is touched. */
CVS_EXPORT int cvs_ycc422_layout(int layout, int width, int height, int strides[3], int line_counts[3]);

/* Import: the samples of `image` (device pointers) -> the pixels of `frame` inside full_window ∩ raster, nothing else written;
 * current_window is emptied first and set to that box on success (0 with an empty window where the box is empty).
 *   decode   yf = ((float)Y - 16s) / (219s), c = ((float)C - 128s) / (224s), s = 1 (8-bit) or 4 (10-bit), correctly rounded;
 *            codes outside the legal range decode like any other.  PLANAR10 ignores bits 10-15, V210 bits 30-31 and the fields
 *            of a last group that lie beyond the width
 *   chroma   x = 2k: v(k); x = 2k+1: (v(k) + v(k+1)) * 0.5f, k+1 clamped to W/2 - 1
 *   matrix   r = (yf*m0 + cb*m1) + cr*m2, likewise g and b, every product and sum rounded on its own in both arithmetic
 *            flavours; flags 0: Rec.601, CVS_YCC_REC709: Rec.709 (the matrices of cvs_reconstruct_mpeg2_dev)
 *   store    r, g, b and 1.0 truncated to half, all four codes through the Rec.709 -> linear (scene) half table
 * Export: half RGBA -> samples.  The frame is only read; pixels outside current_window ∩ raster count as (0, 0, 0, 0), alpha is
 * ignored.  Every sample of the raster is written and nothing else: the least stride's bytes of each of `height` lines.
 *   encode   r, g, b through the linear -> Rec.709 half table, widened; the R'G'B' -> Y'CbCr matrix of Rec.601 (the MPEG-2
 *            subsample's) or Rec.709 (0.2126 0.7152 0.0722 / -0.114572 -0.385428 0.5 / 0.5 -0.454153 -0.045847), no FMA
 *   chroma   C(k) = 0.25f*E(2k-1) + 0.5f*E(2k) + 0.25f*E(2k+1), left to right, column -1 reading column 0
 *   quantise q = Y*(219s/max) + 16s/max or C*(224s/max) + 128s/max, max = 255 or 1023; code = rint(clamp(q, 0, 1) * max), half
 *            to even, NaN -> 0; the 10-bit layouts then clamp the code to [4, 1019] (0-3 and 1020-1023 are reserved on SDI).
 *            PLANAR10 writes bits 10-15 as 0; V210 writes bits 30-31 as 0 and every group whole, fields beyond the width 0
 * Samples -> import -> export gives every 8-bit code back; a 10-bit luma code comes back within one code (the truncation to a
 * half's 11-bit significand), chroma exactly: a 10-bit master through half frames is good to one code, not transparent.
 * Refused with -1 and cvs_set_error (import: an empty current_window): a NULL frame or image; a coordinate beyond
 * +-CVS_MAX_COORD; a flag bit other than CVS_YCC_REC709 (CVS_YCC_PROGRESSIVE included); an unknown layout; an odd width, a width
 * < 2 or a height < 1; a NULL plane pointer; a stride or line count below the least; a base or stride off its alignment;
 * (export) a current_window outside the buffer. */
CVS_EXPORT int cvs_reconstruct_422_dev(rgba_frame_f16 *frame, const coded_image *image, int width, int height, int layout, int flags, cvs_stream_t stream);
CVS_EXPORT int cvs_subsample_422_dev(coded_image *image, const rgba_frame_f16 *frame, int width, int height, int layout, int flags, cvs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
