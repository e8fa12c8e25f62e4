/*
 * matte.c -- cvs_matte_refine_f32_dev / _f16_dev: clip, choke and feather of a matte, the three controls that follow a keyer.
 *
 * No reference code.  The contract is DESIGN.md "Matte refine" and the comment of include/canvas_hip.h; refusals, window
 * arithmetic, the reciprocal of the levels and the tile plan stay here, pixels go to kernels/matte_ops.hip.  This file is
 * compiled with -ffp-contract=off like key.c.
 */
#include "internal.h"

/* The workgroup's output tile.  The kernel keeps two f32 images of the tile plus a halo of `halo` = |choke| + ntaps / 2 samples on
 * every side in LDS, so the halo decides what fits: 128 x 32 pixels cost 2 x 136 x 40 x 4 B = 43 KiB at halo 4 (three workgroups
 * to the CU's 160 KiB) and 127 KiB at the largest halo, 28 (one).  Narrow windows take 64 columns; a halo beyond 8 takes 64
 * columns as long as that buys a second workgroup per CU. */
static void tile_plan(int halo, long long cols, int *tw, int *th) {
    *th = 32;
    *tw = cols > 64 ? 128 : 64;
    if (*tw == 128 && halo > 8) {
        const size_t wide = cvk_matte_lds_bytes(128, *th, halo), narrow = cvk_matte_lds_bytes(64, *th, halo);
        if (CVK_MATTE_MAX_LDS / narrow > CVK_MATTE_MAX_LDS / wide && CVK_MATTE_MAX_LDS / wide < 2) *tw = 64;
    }
}

/* the two entries with their frames taken apart (the two frame structs differ in nothing but the pixel type) */
static int matte_refine(void *tdata, const box2i *tfull, box2i *tcur, const void *sdata, const box2i *sfull, const box2i *scur,
                        const cvs_matte *m, int half, cvs_stream_t stream, const char *what) {
    box2i_set_empty(tcur);
    if (!cvs_box_contains(sfull, scur)) { cvs_set_error("%s: the input's current_window lies outside its buffer", what); return -1; }
    if (cvs_coords_refused(what, "source", sfull, scur, CVS_MAX_COORD) || cvs_coords_refused(what, "target", tfull, NULL, CVS_MAX_COORD)) return -1;
    if (m->choke > CVS_MATTE_MAX_CHOKE || m->choke < -CVS_MATTE_MAX_CHOKE) { cvs_set_error("%s: choke %d is beyond +-%d", what, m->choke, CVS_MATTE_MAX_CHOKE); return -1; }
    if (m->ntaps < 0 || m->ntaps > CVS_MATTE_MAX_TAPS || (m->ntaps > 0 && !(m->ntaps & 1))) {
        cvs_set_error("%s: the feather takes 0 or an odd count of up to %d taps, not %d", what, CVS_MATTE_MAX_TAPS, m->ntaps);
        return -1;
    }
    if (m->ntaps > 0 && !m->taps) { cvs_set_error("%s: %d taps and no tap list", what, m->ntaps); return -1; }
    for (int k = 0; k < m->ntaps; k++)
        if (!isfinite(m->taps[k])) { cvs_set_error("%s: tap %d is not finite", what, k); return -1; }
    if (!isfinite(m->black) || !isfinite(m->white) || !(m->white > m->black)) {
        cvs_set_error("%s: black %g and white %g must be finite, white above black", what, m->black, m->white);
        return -1;
    }
    if (m->flags & ~CVS_MATTE_SHOW) { cvs_set_error("%s: unknown flags 0x%x", what, (unsigned)m->flags); return -1; }
    if (tdata == sdata) { cvs_set_error("%s: the target is the source's buffer: the operation is not in place", what); return -1; }
    if (cvs_enter() != 0) return -1;
    box2i win;
    box2i_intersect(&win, scur, tfull);
    if (box2i_is_empty(scur) || box2i_is_empty(&win)) return 0;

    cvk_matte_params mp;
    memset(&mp, 0, sizeof mp);
    mp.out = cvs_view(tdata, tfull);
    mp.in = cvs_view((void *)sdata, sfull);
    mp.w = cvs_rect(&win);
    mp.s = cvs_rect(scur);
    mp.r = m->choke < 0 ? -m->choke : m->choke;
    mp.grow = m->choke < 0;
    mp.ntaps = m->ntaps;
    for (int k = 0; k < m->ntaps; k++) mp.taps[k] = m->taps[k];
    mp.levels = !(m->black == 0.0f && m->white == 1.0f);
    mp.black = m->black;
    mp.inv = 1.0f / (m->white - m->black);
    mp.show = (m->flags & CVS_MATTE_SHOW) != 0;
    tile_plan(mp.r + m->ntaps / 2, (long long)win.max.x - win.min.x + 1, &mp.tw, &mp.th);
    const int rc = cvk_matte_refine(&mp, half, cvs_pick_stream(stream));
    if (rc != 0) { cvs_set_error("%s: %s", what, hipGetErrorString((hipError_t)rc)); return -1; }
    *tcur = win;
    return 0;
}

CVS_EXPORT int cvs_matte_refine_f32_dev(rgba_frame_f32 *target, const rgba_frame_f32 *source, const cvs_matte *m, cvs_stream_t s) {
    if (!target || !source || !m) {
        if (target) box2i_set_empty(&target->current_window);
        cvs_set_error("cvs_matte_refine_f32_dev: need the frames and the matte settings");
        return -1;
    }
    return matte_refine(target->data, &target->full_window, &target->current_window, source->data, &source->full_window, &source->current_window, m, 0, s, "cvs_matte_refine_f32_dev");
}

CVS_EXPORT int cvs_matte_refine_f16_dev(rgba_frame_f16 *target, const rgba_frame_f16 *source, const cvs_matte *m, cvs_stream_t s) {
    if (!target || !source || !m) {
        if (target) box2i_set_empty(&target->current_window);
        cvs_set_error("cvs_matte_refine_f16_dev: need the frames and the matte settings");
        return -1;
    }
    return matte_refine(target->data, &target->full_window, &target->current_window, source->data, &source->full_window, &source->current_window, m, 1, s, "cvs_matte_refine_f16_dev");
}
