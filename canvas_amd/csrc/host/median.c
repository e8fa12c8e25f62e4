/*
 * median.c -- cvs_median_f32_dev / _f16_dev: a 3 x 3 or 5 x 5 median per channel, the despeckle.
 *
 * No reference code: the reference has no rank filter and names none.  The contract is DESIGN.md "Median" and the comment of
 * include/canvas_median.h; refusals and window arithmetic stay here, pixels go to kernels/median_ops.hip.  One build of the
 * kernels (a selection rounds nothing), so no CVK() here.  No allocation and no synchronisation: the call records into a graph.
 */
#include "internal.h"
#include "canvas_median.h"

/* the two entries with their frames taken apart (the two frame structs differ in nothing but the pixel type) */
static int median(void *tdata, const box2i *tfull, box2i *tcur, const void *sdata, const box2i *sfull, const box2i *scur,
                  const cvs_median *p, int half, cvs_stream_t stream, const char *what) {
    box2i_set_empty(tcur);
    if (p->radius != 1 && p->radius != 2) { cvs_set_error("%s: radius %d is neither 1 (3 x 3) nor 2 (5 x 5)", what, p->radius); return -1; }
    if (p->channels == 0 || (p->channels & ~CVS_MEDIAN_ALL) != 0) { cvs_set_error("%s: channels 0x%x is not a mask of CVS_MEDIAN_R, _G, _B, _A with a channel in it", what, (unsigned)p->channels); return -1; }
    if (p->flags != 0) { cvs_set_error("%s: unknown flags 0x%x", what, (unsigned)p->flags); return -1; }
    if (!isfinite(p->threshold) || p->threshold < 0.0f) { cvs_set_error("%s: threshold %g must be finite and not negative", what, p->threshold); return -1; }
    if (tdata == sdata) { cvs_set_error("%s: the target cannot be the source (the median gathers: there is no in-place form)", what); return -1; }
    if (!cvs_box_contains(sfull, scur)) { cvs_set_error("%s: the input's current_window lies outside its buffer", what); return -1; }
    if (cvs_coords_refused(what, "source", sfull, scur, CVS_MAX_COORD) || cvs_coords_refused(what, "target", tfull, NULL, CVS_MAX_COORD)) return -1;
    if (cvs_enter() != 0) return -1;
    box2i win;
    box2i_intersect(&win, scur, tfull);
    if (box2i_is_empty(scur) || box2i_is_empty(&win)) return 0;

    cvk_median_params mp;
    memset(&mp, 0, sizeof mp);
    mp.out = cvs_view(tdata, tfull);
    mp.in = cvs_view((void *)sdata, sfull);
    mp.w = cvs_rect(&win);
    mp.cw = cvs_rect(scur);
    mp.radius = p->radius;
    mp.channels = p->channels;
    mp.gated = p->threshold > 0.0f;
    mp.threshold = p->threshold;
    const int rc = cvk_median(&mp, half, cvs_cus(), cvs_pick_stream(stream));
    if (rc != 0) { cvs_set_error("%s: %s", what, hipGetErrorString((hipError_t)rc)); return -1; }
    *tcur = win;
    return 0;
}

CVS_EXPORT int cvs_median_f32_dev(rgba_frame_f32 *target, const rgba_frame_f32 *source, const cvs_median *p, cvs_stream_t s) {
    if (!target || !source || !p) {
        if (target) box2i_set_empty(&target->current_window);
        cvs_set_error("cvs_median_f32_dev: need the frames and the parameters");
        return -1;
    }
    const box2i scur = source->current_window;          /* (a copy: handed in as one struct, the target is the source) */
    return median(target->data, &target->full_window, &target->current_window, source->data, &source->full_window, &scur, p, 0, s, "cvs_median_f32_dev");
}

CVS_EXPORT int cvs_median_f16_dev(rgba_frame_f16 *target, const rgba_frame_f16 *source, const cvs_median *p, cvs_stream_t s) {
    if (!target || !source || !p) {
        if (target) box2i_set_empty(&target->current_window);
        cvs_set_error("cvs_median_f16_dev: need the frames and the parameters");
        return -1;
    }
    const box2i scur = source->current_window;
    return median(target->data, &target->full_window, &target->current_window, source->data, &source->full_window, &scur, p, 1, s, "cvs_median_f16_dev");
}
