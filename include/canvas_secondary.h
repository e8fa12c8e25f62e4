/*
 * canvas_secondary.h -- the secondaries of libcanvas_hip.so: a qualifier that makes a matte from a pixel's hue, saturation and
 * luma, and a mix of two frames through a matte held in a third.  An extension of include/canvas_hip.h (frames, boxes, streams
 * and the coordinate contract are its); the functions live in the same library.  Contract: DESIGN.md "Secondaries".
 */
#ifndef CANVAS_SECONDARY_H
#define CANVAS_SECONDARY_H

#include "canvas_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Secondaries (DESIGN.md "Secondaries").  Frames are un-premultiplied.  All arithmetic is in f32 (a half widened exactly), every
 * operation rounded on its own in BOTH arithmetic flavours, divides IEEE and correctly rounded; f16 targets are truncated once,
 * at the store.  sel(t) = (t > 0) ? ((t < 1) ? t : 1) : 0; NaN gives 0: a pixel that cannot be measured is not selected.
 *
 * The qualifier.  A hue range is (center, width, softness) in degrees: hues within width / 2 of center are selected, and the
 * selection falls to none over `softness` degrees beyond; it wraps through 0 = 360.  A value range is (low, high, soft_low,
 * soft_high): values in [low, high] are selected, falling to none over soft_low below low and soft_high above high; high = +inf
 * is no upper bound.  The host forms once per call, in f32: hc = fmodf(center, 360) / 60, plus 6 if negative; hw = width / 120;
 * hs = softness / 60; h_edge = hw + hs; inv_hs = 1 / hs where hs > 0; per value range lo_edge = low - soft_low, hi_edge = high +
 * soft_high and inv_soft_low = 1 / soft_low, inv_soft_high = 1 / soft_high, each where its softness is > 0.  Per pixel (r, g, b)
 * of the key frame (key == NULL: the source is qualified against itself) and pixel s of the source:
 *     any of r, g, b NaN -> m = 0
 *     mx = max(r, g, b) ;  mn = min(r, g, b) ;  c = mx - mn
 *     y  = (r*0.2126f + g*0.7152f) + b*0.0722f
 *     s  = mx > 0 ? c / mx : 0                                         HSV saturation; may exceed 1 with negative components
 *     hue in sextants [0, 6], only where c > 0:
 *         r == mx (tested first):  h = (g - b) / c ;  if h < 0: h = h + 6
 *         else g == mx:            h = (b - r) / c + 2
 *         else:                    h = (r - g) / c + 4
 *         d = |h - hc| ;  e = 6 - d ;  d = e < d ? e : d
 *     m_h = !(c > 0) ? 0 : hs > 0 ? sel((h_edge - d) * inv_hs) : (d <= hw ? 1 : 0)       achromatic pixels are never selected by hue
 *     range(v) = min(soft_low  > 0 ? sel((v - lo_edge) * inv_soft_low)  : (v >= low  ? 1 : 0),
 *                    soft_high > 0 ? sel((hi_edge - v) * inv_soft_high) : (v <= high ? 1 : 0))
 *     m = (m_h * range_sat(s)) * range_luma(y)          an axis whose flag is clear contributes exactly 1
 *     CVS_QUAL_INVERT: m = 1 - m
 *     a' = s.a * m
 *     out = CVS_QUAL_SHOW_MATTE ? (a', a', a', 1) : (s.r, s.g, s.b, a')                   colour code for code
 * Pure R, Y, G, C, B, M have the hues 0, 1, 2, 3, 4, 5 exactly.
 *
 * The mix through a matte, per pixel of a, b and the matte M:
 *     v = CVS_MMIX_LUMA ? (M.r*0.2126f + M.g*0.7152f) + M.b*0.0722f : M.a ;  k = sel(v) ;  CVS_MMIX_INVERT: k = 1 - k
 *     k == 0: out = a's four codes ;  k == 1: out = b's four codes      selected, not computed: Inf and NaN pass as they are
 *     else for c in r, g, b, a:  e = b.c - a.c ;  f = k * e ;  out.c = a.c + f
 *
 * Windows.  Each input's current_window must lie inside its full_window.  The window worked on is the intersection of all inputs'
 * current_windows with the target's full_window; it becomes the target's current_window.  Where it is empty the entry returns 0
 * and launches nothing.
 *
 * Refused with -1 and a message that names the entry, before the device is touched, with the target's window set empty and
 * nothing written: a NULL frame (key excepted) or a NULL parameter struct; unknown flag bits; for an axis whose flag is set: a
 * center, width, softness, low, soft_low or soft_high that is not finite, a negative width or softness, a NaN high, or
 * high < low (high = +inf is allowed); a current window outside its buffer; coordinates beyond +-CVS_MAX_COORD, on every frame.
 * Fields of an axis whose flag is clear are not looked at.  Any extent inside the bound is folded, never refused.
 *
 * Operands that share a buffer, in the terms of the block in canvas_hip.h:
 *   - IN PLACE: the entry computes, bit for bit, windows included, what the same call gives on a distinct copy of the input.
 *     Every lane reads the pixels it writes before it writes them.
 *   - REFUSED: none.
 *   - SHARED: both operands are only read, and may be one buffer.
 *   in place:
 *     cvs_qualify_f16_dev (target, source) (target, key); cvs_qualify_f32_dev (target, source) (target, key);
 *     cvs_matte_mix_f16_dev (target, a) (target, b) (target, matte); cvs_matte_mix_f32_dev (target, a) (target, b) (target, matte)
 *   refused:
 *   shared:
 *     cvs_qualify_f16_dev (source, key); cvs_qualify_f32_dev (source, key);
 *     cvs_matte_mix_f16_dev (a, b) (a, matte) (b, matte); cvs_matte_mix_f32_dev (a, b) (a, matte) (b, matte)
 */
typedef struct { float center, width, softness; } cvs_hue_range;          /* degrees */
typedef struct { float low, high, soft_low, soft_high; } cvs_value_range;
#define CVS_QUAL_HUE        1u      /* which axes qualify */
#define CVS_QUAL_SATURATION 2u
#define CVS_QUAL_LUMA       4u
#define CVS_QUAL_INVERT     8u
#define CVS_QUAL_SHOW_MATTE 16u
typedef struct cvs_qualifier {
    uint32_t        flags;
    cvs_hue_range   hue;
    cvs_value_range saturation, luma;
} cvs_qualifier;
/* target may be source's or key's buffer, in place; key may be NULL */
CVS_EXPORT int cvs_qualify_f16_dev(rgba_frame_f16 *target, const rgba_frame_f16 *source, const rgba_frame_f16 *key, const cvs_qualifier *q, cvs_stream_t s);
CVS_EXPORT int cvs_qualify_f32_dev(rgba_frame_f32 *target, const rgba_frame_f32 *source, const rgba_frame_f32 *key, const cvs_qualifier *q, cvs_stream_t s);

#define CVS_MMIX_LUMA   1u          /* k from the matte's Rec.709 luma instead of its alpha */
#define CVS_MMIX_INVERT 2u
typedef struct cvs_matte_mix { uint32_t flags; } cvs_matte_mix;
/* target may be the buffer of a, of b or of matte, in place */
CVS_EXPORT int cvs_matte_mix_f16_dev(rgba_frame_f16 *target, const rgba_frame_f16 *a, const rgba_frame_f16 *b, const rgba_frame_f16 *matte, const cvs_matte_mix *p, cvs_stream_t s);
CVS_EXPORT int cvs_matte_mix_f32_dev(rgba_frame_f32 *target, const rgba_frame_f32 *a, const rgba_frame_f32 *b, const rgba_frame_f32 *matte, const cvs_matte_mix *p, cvs_stream_t s);

#ifdef __cplusplus
}
#endif
#endif
