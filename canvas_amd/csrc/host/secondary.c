/*
 * secondary.c -- cvs_qualify_f32_dev / _f16_dev and cvs_matte_mix_f32_dev / _f16_dev: a matte from a pixel's hue, saturation and
 * luma, and a mix of two frames through a matte held in a third.
 *
 * No reference code.  The contract is DESIGN.md "Secondaries" and the comment of include/canvas_secondary.h; refusals, window
 * arithmetic and what is computed once per call stay here, pixels go to kernels/secondary_ops.hip.  This file is compiled with
 * -ffp-contract=off: the edges of the ranges round as the model's do.
 */
#include "internal.h"
#include "canvas_secondary.h"

#define QUAL_FLAGS (CVS_QUAL_HUE | CVS_QUAL_SATURATION | CVS_QUAL_LUMA | CVS_QUAL_INVERT | CVS_QUAL_SHOW_MATTE)
#define MMIX_FLAGS (CVS_MMIX_LUMA | CVS_MMIX_INVERT)

static bool width_ok(float v) { return isfinite(v) && v >= 0.0f; }

/* one frame operand taken apart (the two frame structs differ in nothing but the pixel type); cur is a copy: the target may be
 * the same frame struct, and its window is emptied first */
typedef struct { const char *name; void *data; const box2i *full; box2i cur; } operand;

/* what every entry here does with its frames after its own refusals: 0 and the window worked on in *win (empty: nothing to do),
 * or -1 with the error set */
static int windows(const char *what, const box2i *tfull, const operand *in, int n, box2i *win) {
    for (int k = 0; k < n; k++)
        if (!cvs_box_contains(in[k].full, &in[k].cur)) { cvs_set_error("%s: %s: the input's current_window lies outside its buffer", what, in[k].name); return -1; }
    for (int k = 0; k < n; k++)
        if (cvs_coords_refused(what, in[k].name, in[k].full, &in[k].cur, CVS_MAX_COORD)) return -1;
    if (cvs_coords_refused(what, "target", tfull, NULL, CVS_MAX_COORD)) return -1;
    if (cvs_enter() != 0) return -1;
    *win = *tfull;
    for (int k = 0; k < n; k++) {
        if (box2i_is_empty(&in[k].cur)) { box2i_set_empty(win); return 0; }
        box2i next;
        box2i_intersect(&next, win, &in[k].cur);
        *win = next;
        if (box2i_is_empty(win)) return 0;
    }
    return 0;
}

static bool range_refused(const char *what, const char *axis, const cvs_value_range *r) {
    if (!isfinite(r->low) || !width_ok(r->soft_low) || !width_ok(r->soft_high) || isnan(r->high) || r->high < r->low) {
        cvs_set_error("%s: the %s range (low %g, high %g, soft_low %g, soft_high %g) needs a finite low, high >= low (+inf: no upper bound) and widths that are finite and not negative",
                      what, axis, r->low, r->high, r->soft_low, r->soft_high);
        return true;
    }
    return false;
}

static void range_plan(cvk_value_range *out, const cvs_value_range *r) {
    out->low = r->low;
    out->high = r->high;
    out->lo_edge = r->low - r->soft_low;
    out->hi_edge = r->high + r->soft_high;
    out->soft_lo = r->soft_low > 0.0f;
    out->soft_hi = r->soft_high > 0.0f;
    if (out->soft_lo) out->inv_lo = 1.0f / r->soft_low;
    if (out->soft_hi) out->inv_hi = 1.0f / r->soft_high;
}

static int qualify(void *tdata, const box2i *tfull, box2i *tcur, operand *in, int n, const cvs_qualifier *q, int half, cvs_stream_t stream, const char *what) {
    box2i_set_empty(tcur);
    if ((q->flags & ~QUAL_FLAGS) != 0) { cvs_set_error("%s: unknown flags 0x%x", what, q->flags); return -1; }
    if (q->flags & CVS_QUAL_HUE)
        if (!isfinite(q->hue.center) || !width_ok(q->hue.width) || !width_ok(q->hue.softness)) {
            cvs_set_error("%s: the hue range (center %g, width %g, softness %g) needs a finite center and widths that are finite and not negative", what, q->hue.center, q->hue.width, q->hue.softness);
            return -1;
        }
    if ((q->flags & CVS_QUAL_SATURATION) && range_refused(what, "saturation", &q->saturation)) return -1;
    if ((q->flags & CVS_QUAL_LUMA) && range_refused(what, "luma", &q->luma)) return -1;
    box2i win;
    if (windows(what, tfull, in, n, &win) != 0) return -1;
    if (box2i_is_empty(&win)) return 0;

    cvk_qualify_params qp;
    memset(&qp, 0, sizeof qp);
    qp.hue = (q->flags & CVS_QUAL_HUE) != 0;
    qp.saturation = (q->flags & CVS_QUAL_SATURATION) != 0;
    qp.lum = (q->flags & CVS_QUAL_LUMA) != 0;
    qp.invert = (q->flags & CVS_QUAL_INVERT) != 0;
    qp.matte = (q->flags & CVS_QUAL_SHOW_MATTE) != 0;
    if (qp.hue) {
        float hc = fmodf(q->hue.center, 360.0f) / 60.0f;
        if (hc < 0.0f) hc = hc + 6.0f;
        const float hs = q->hue.softness / 60.0f;
        qp.hc = hc;
        qp.hw = q->hue.width / 120.0f;
        qp.h_edge = qp.hw + hs;
        qp.hue_soft = hs > 0.0f;
        if (qp.hue_soft) qp.inv_hs = 1.0f / hs;
    }
    if (qp.saturation) range_plan(&qp.sat, &q->saturation);
    if (qp.lum) range_plan(&qp.luma, &q->luma);
    cvk_view kview;
    if (n == 2) kview = cvs_view(in[1].data, in[1].full);
    const int rc = cvk_qualify(&qp, cvs_view(tdata, tfull), cvs_view(in[0].data, in[0].full), n == 2 ? &kview : NULL, cvs_rect(&win), half, cvs_cus(), cvs_pick_stream(stream));
    if (rc != 0) { cvs_set_error("%s: %s", what, hipGetErrorString((hipError_t)rc)); return -1; }
    *tcur = win;
    return 0;
}

static int matte_mix(void *tdata, const box2i *tfull, box2i *tcur, operand *in, const cvs_matte_mix *p, int half, cvs_stream_t stream, const char *what) {
    box2i_set_empty(tcur);
    if ((p->flags & ~MMIX_FLAGS) != 0) { cvs_set_error("%s: unknown flags 0x%x", what, p->flags); return -1; }
    box2i win;
    if (windows(what, tfull, in, 3, &win) != 0) return -1;
    if (box2i_is_empty(&win)) return 0;
    const int rc = cvk_matte_mix(cvs_view(tdata, tfull), cvs_view(in[0].data, in[0].full), cvs_view(in[1].data, in[1].full), cvs_view(in[2].data, in[2].full), cvs_rect(&win),
                                 (p->flags & CVS_MMIX_LUMA) != 0, (p->flags & CVS_MMIX_INVERT) != 0, half, cvs_cus(), cvs_pick_stream(stream));
    if (rc != 0) { cvs_set_error("%s: %s", what, hipGetErrorString((hipError_t)rc)); return -1; }
    *tcur = win;
    return 0;
}

#define OPERAND(label, f) { label, (void *)(f)->data, &(f)->full_window, (f)->current_window }

#define QUALIFY_ENTRY(NAME, FRAME, HALF)                                                                                       \
    CVS_EXPORT int NAME(FRAME *target, const FRAME *source, const FRAME *key, const cvs_qualifier *q, cvs_stream_t s) {        \
        if (!target || !source || !q) {                                                                                        \
            if (target) box2i_set_empty(&target->current_window);                                                              \
            cvs_set_error(#NAME ": need the frames and the qualifier");                                                        \
            return -1;                                                                                                         \
        }                                                                                                                      \
        operand in[2] = { OPERAND("source", source), OPERAND("key", key ? key : source) };                                     \
        return qualify(target->data, &target->full_window, &target->current_window, in, key ? 2 : 1, q, HALF, s, #NAME);       \
    }
QUALIFY_ENTRY(cvs_qualify_f32_dev, rgba_frame_f32, 0)
QUALIFY_ENTRY(cvs_qualify_f16_dev, rgba_frame_f16, 1)

#define MATTE_MIX_ENTRY(NAME, FRAME, HALF)                                                                                     \
    CVS_EXPORT int NAME(FRAME *target, const FRAME *a, const FRAME *b, const FRAME *matte, const cvs_matte_mix *p, cvs_stream_t s) { \
        if (!target || !a || !b || !matte || !p) {                                                                             \
            if (target) box2i_set_empty(&target->current_window);                                                              \
            cvs_set_error(#NAME ": need the frames and the parameters");                                                       \
            return -1;                                                                                                         \
        }                                                                                                                      \
        operand in[3] = { OPERAND("a", a), OPERAND("b", b), OPERAND("matte", matte) };                                         \
        return matte_mix(target->data, &target->full_window, &target->current_window, in, p, HALF, s, #NAME);                  \
    }
MATTE_MIX_ENTRY(cvs_matte_mix_f32_dev, rgba_frame_f32, 0)
MATTE_MIX_ENTRY(cvs_matte_mix_f16_dev, rgba_frame_f16, 1)
