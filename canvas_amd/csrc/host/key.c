/*
 * key.c -- cvs_chroma_key_f32_dev / _f16_dev: a chroma-distance keyer with spill suppression.
 *
 * No reference code: its design notes name "Chromakey effects" among the filters an editor carries
 * (docs/sphinx/feature-proposal/hints.rst:70) and it built none.  The contract is DESIGN.md "Chroma key" and the comment of
 * include/canvas_hip.h; refusals, window arithmetic and what is computed once per call stay here, pixels go to
 * kernels/key_ops.hip.  This file is compiled with -ffp-contract=off: the key colour's Pb and Pr round as the kernel's do.
 */
#include "internal.h"

/* rows 1 and 2 of the A14 Rec.709 R'G'B' -> Y'PbPr matrix (kernels/dv_ops.hip, kernels/key_ops.hip) */
static const float c1[3] = { -0.114572f, -0.385428f, 0.5f }, c2[3] = { 0.5f, -0.454153f, -0.045847f };

static bool width_ok(float v) { return isfinite(v) && v >= 0.0f; }

/* the two entries with their frames taken apart (the two frame structs differ in nothing but the pixel type) */
static int chroma_key(void *tdata, const box2i *tfull, box2i *tcur, const void *sdata, const box2i *sfull, const box2i *scur,
                      const cvs_chroma_key *key, int half, cvs_stream_t stream, const char *what) {
    box2i_set_empty(tcur);
    if (!cvs_box_contains(sfull, scur)) { cvs_set_error("%s: the input's current_window lies outside its buffer", what); return -1; }
    if (cvs_coords_refused(what, "source", sfull, scur, CVS_MAX_COORD) || cvs_coords_refused(what, "target", tfull, NULL, CVS_MAX_COORD)) return -1;
    if (!isfinite(key->key[0]) || !isfinite(key->key[1]) || !isfinite(key->key[2])) { cvs_set_error("%s: the key colour is not finite", what); return -1; }
    if (!width_ok(key->tolerance) || !width_ok(key->softness) || !width_ok(key->spill_range)) {
        cvs_set_error("%s: tolerance %g, softness %g and spill_range %g must be finite and not negative", what, key->tolerance, key->softness, key->spill_range);
        return -1;
    }
    if (cvs_enter() != 0) return -1;
    box2i win;
    box2i_intersect(&win, scur, tfull);
    if (box2i_is_empty(scur) || box2i_is_empty(&win)) return 0;

    cvk_key_params kp;
    memset(&kp, 0, sizeof kp);
    kp.kpb = (key->key[0] * c1[0] + key->key[1] * c1[1]) + key->key[2] * c1[2];
    kp.kpr = (key->key[0] * c2[0] + key->key[1] * c2[1]) + key->key[2] * c2[2];
    kp.tolerance = key->tolerance;
    kp.soft = key->softness > 0.0f;
    kp.fade = key->spill_range > 0.0f;
    if (kp.soft) kp.inv_soft = 1.0f / key->softness;
    if (kp.fade) kp.inv_spill = 1.0f / key->spill_range;
    kp.spill = key->spill > 0.0f ? (key->spill < 1.0f ? key->spill : 1.0f) : 0.0f;       /* a NaN strength is none */
    kp.matte = (key->flags & CVS_KEY_SHOW_MATTE) != 0;
    const int rc = cvk_chroma_key(&kp, cvs_view(tdata, tfull), cvs_view((void *)sdata, sfull), cvs_rect(&win), half, cvs_cus(), cvs_pick_stream(stream));
    if (rc != 0) { cvs_set_error("%s: %s", what, hipGetErrorString((hipError_t)rc)); return -1; }
    *tcur = win;
    return 0;
}

CVS_EXPORT int cvs_chroma_key_f32_dev(rgba_frame_f32 *target, const rgba_frame_f32 *source, const cvs_chroma_key *key, cvs_stream_t s) {
    if (!target || !source || !key) {
        if (target) box2i_set_empty(&target->current_window);
        cvs_set_error("cvs_chroma_key_f32_dev: need the frames and the key");
        return -1;
    }
    const box2i scur = source->current_window;          /* (a copy: the target may be the source frame itself) */
    return chroma_key(target->data, &target->full_window, &target->current_window, source->data, &source->full_window, &scur, key, 0, s, "cvs_chroma_key_f32_dev");
}

CVS_EXPORT int cvs_chroma_key_f16_dev(rgba_frame_f16 *target, const rgba_frame_f16 *source, const cvs_chroma_key *key, cvs_stream_t s) {
    if (!target || !source || !key) {
        if (target) box2i_set_empty(&target->current_window);
        cvs_set_error("cvs_chroma_key_f16_dev: need the frames and the key");
        return -1;
    }
    const box2i scur = source->current_window;
    return chroma_key(target->data, &target->full_window, &target->current_window, source->data, &source->full_window, &scur, key, 1, s, "cvs_chroma_key_f16_dev");
}
