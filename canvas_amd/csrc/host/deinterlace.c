/*
 * deinterlace.c -- cvs_deinterlace_adaptive_f16_dev: a woven frame made into a whole picture with the frames before and after
 * it; rows of the other field kept where nothing moved, interpolated where something did.
 *
 * No reference code: the design names "motion-adaptive ... deinterlacing" among the field conversions
 * (docs/sphinx/feature-proposal/canvas.rst:283-303) and built none.  The contract is DESIGN.md "Adaptive deinterlace" and the
 * comment of include/canvas_deinterlace.h; refusals, window arithmetic and which neighbours are present stay here, pixels go to
 * kernels/deinterlace_ops.hip -- or, with no neighbour present, to kernels/field_ops.hip, which by the contract gives the same
 * bits and reads a third of the rows.  One build of the kernels (every operation rounded on its own), so no CVK() here.
 */
#include "internal.h"
#include "canvas_deinterlace.h"

static const char what[] = "cvs_deinterlace_adaptive_f16_dev";

static bool present(const rgba_frame_f16 *f) { return f && !box2i_is_empty(&f->current_window); }

CVS_EXPORT int cvs_deinterlace_adaptive_f16_dev(rgba_frame_f16 *out, const rgba_frame_f16 *prev, const rgba_frame_f16 *cur,
                                                const rgba_frame_f16 *next, const cvs_deinterlace_adaptive *p, cvs_stream_t s) {
    /* Asked before the output's window is emptied: handed in as ONE struct, the output is that input, window and all, and a
     * neighbour would then pass for absent (canvas_hip.h "Operands that share a buffer"). */
    const rgba_frame_f16 *in[3] = { cur, prev, next };
    bool shares = false;
    for (int i = 0; out && i < 3; i++) shares = shares || (in[i] && (i == 0 || present(in[i])) && out->data == in[i]->data);
    if (out) box2i_set_empty(&out->current_window);
    if (!out || !cur || !p) { cvs_set_error("%s: need the frames and the parameters", what); return -1; }
    if (p->field != 0 && p->field != 1) { cvs_set_error("%s: field %d is neither 0 (even rows) nor 1 (odd rows)", what, p->field); return -1; }
    if (p->flags != 0) { cvs_set_error("%s: unknown flags 0x%x", what, (unsigned)p->flags); return -1; }
    if (!isfinite(p->threshold)) { cvs_set_error("%s: threshold %g must be finite", what, p->threshold); return -1; }
    if (!isfinite(p->softness) || p->softness < 0.0f) { cvs_set_error("%s: softness %g must be finite and not negative", what, p->softness); return -1; }
    if (shares) { cvs_set_error("%s: the output cannot be one of the inputs", what); return -1; }
    for (int i = 0; i < 3; i++) {
        if (!in[i]) continue;
        if (!cvs_box_contains(&in[i]->full_window, &in[i]->current_window)) { cvs_set_error("%s: an input's current_window lies outside its buffer", what); return -1; }
    }
    if (cvs_coords_refused(what, "out", &out->full_window, NULL, CVS_MAX_COORD)) return -1;
    for (int i = 0; i < 3; i++)
        if (in[i] && cvs_coords_refused(what, "an input", &in[i]->full_window, &in[i]->current_window, CVS_MAX_COORD)) return -1;
    if (cvs_enter() != 0) return -1;

    box2i w;
    box2i_intersect(&w, &out->full_window, &cur->current_window);
    if (box2i_is_empty(&cur->current_window) || box2i_is_empty(&w)) return 0;

    /* the neighbours that have a sample within one pixel of the window written: the others change nothing */
    cvk_deinterlace_params dp;
    memset(&dp, 0, sizeof dp);
    box2i reach = { { w.min.x - 1, w.min.y - 1 }, { w.max.x + 1, w.max.y + 1 } };           /* (inside int: CVS_MAX_COORD) */
    int count = 0;
    for (int i = 1; i < 3; i++) {
        if (!present(in[i])) continue;
        if (i == 2 && count == 1 && next->data == prev->data && memcmp(&next->full_window, &prev->full_window, sizeof(box2i)) == 0 &&
            memcmp(&next->current_window, &prev->current_window, sizeof(box2i)) == 0) continue;          /* one frame given twice */
        box2i v, near;
        box2i_intersect(&v, &cur->current_window, &in[i]->current_window);
        box2i_intersect(&near, &v, &reach);
        if (box2i_is_empty(&v) || box2i_is_empty(&near)) continue;
        dp.n[count] = cvs_view(in[i]->data, &in[i]->full_window);
        dp.v[count] = cvs_rect(&v);
        count++;
    }

    int rc;
    if (count == 0) {
        rc = cvk_field_to_frame(cvs_view(out->data, &out->full_window), cvs_view(cur->data, &cur->full_window), cvs_rect(&w),
                                cvs_rect(&cur->current_window), p->field, cvs_cus(), cvs_pick_stream(s));
    } else {
        dp.out = cvs_view(out->data, &out->full_window);
        dp.cur = cvs_view(cur->data, &cur->full_window);
        dp.w = cvs_rect(&w);
        dp.cw = cvs_rect(&cur->current_window);
        dp.field = p->field;
        dp.threshold = p->threshold;
        dp.soft = p->softness > 0.0f;
        if (dp.soft) dp.inv_soft = 1.0f / p->softness;
        rc = cvk_deinterlace_adaptive(&dp, count, cvs_cus(), cvs_pick_stream(s));
    }
    if (rc != 0) { cvs_set_error("%s: %s", what, hipGetErrorString((hipError_t)rc)); return rc; }
    out->current_window = w;
    return 0;
}
