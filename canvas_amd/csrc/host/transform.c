/*
 * transform.c -- cvs_transform_f32_dev / _f16_dev: an affine warp with an alpha-weighted bilinear or Catmull-Rom filter, and the host arithmetic
 * that goes with it (the coefficients from anchor, scale, rotation and position; the target and source windows).
 *
 * No reference code.  The contract is DESIGN.md "Affine transform" and the comment of include/canvas_hip.h; refusals, the windows
 * and the tile plan stay here, pixels go to kernels/transform_ops.hip (Catmull-Rom: kernels/warp_cubic_ops.hip).  All window arithmetic is in double, every operation
 * rounded on its own (this file is compiled with -ffp-contract=off), written in the order DESIGN.md gives so that the numpy model
 * of the tests (tests/transform_model.py) repeats it exactly.
 */
#include "internal.h"

#define WINDOW_LIMIT 1073741824.0                       /* 2^30: what a window bound is clamped to before it becomes an int */

/* The workgroup's tile of target pixels, tw x th == 256 lanes.  A wave is 64 consecutive lanes, x first: at 32 x 8 it covers a
 * 32 x 2 patch of the target, whose source footprint under any rotation stays within a few rows and columns of each other,
 * and a store instruction still writes two runs of 32 pixels (256 B of half pixels each).  64 x 4 gives one 64-pixel run per
 * wave and a footprint twice as long: measured on an MI355X it is 4 % slower at 30 degrees and 10 % slower at 90, and faster only
 * for a reduction to half size (DESIGN.md "Affine transform", Measured). */
static void tile_plan(cvk_transform_params *tp) {
    tp->tw = 32;
    tp->th = 8;
    tp->pair_loads = 0;
#ifdef CVS_DIAG
    /* measuring aid of the diagnostic build: CVS_TRANSFORM_PLAN=<tw>x<th>[p], p for the 16-byte pair loads */
    const char *env = getenv("CVS_TRANSFORM_PLAN");
    int tw, th;
    char p = 0;
    if (env && sscanf(env, "%dx%d%c", &tw, &th, &p) >= 2) { tp->tw = tw; tp->th = th; tp->pair_loads = p == 'p'; }
#endif
}

/* (which filters there are, their reach and the source window's pad: internal.h, shared by the two warps) */

/* m widened, its determinant and the forward (source -> target) map F; false with the error set where the contract refuses */
typedef struct { double m[6], det, f00, f01, f02, f10, f11, f12; } affine;
static bool affine_from(const cvs_transform *t, affine *a, const char *what) {
    if (!cvs_warp_filter_known(t->filter)) { cvs_set_error(CVS_WARP_FILTER_REFUSAL, what, t->filter); return false; }
    if (t->flags != 0) { cvs_set_error("%s: unknown flags 0x%x", what, (unsigned)t->flags); return false; }
    for (int k = 0; k < 6; k++) {
        if (!isfinite(t->m[k])) { cvs_set_error("%s: coefficient m[%d] is not finite", what, k); return false; }
        a->m[k] = (double)t->m[k];
    }
    const double *m = a->m;
    a->det = m[0] * m[4] - m[1] * m[3];
    if (a->det == 0.0 || !isfinite(a->det)) { cvs_set_error("%s: the determinant of m is %g: the transform cannot be inverted", what, a->det); return false; }
    a->f00 = m[4] / a->det;
    a->f01 = -m[1] / a->det;
    a->f10 = -m[3] / a->det;
    a->f11 = m[0] / a->det;
    a->f02 = -(a->f00 * m[2] + a->f01 * m[5]);
    a->f12 = -(a->f10 * m[2] + a->f11 * m[5]);
    return true;
}

/* [floor(lo) - pad, ceil(hi) + pad] of the four values, each bound clamped to +-2^30; a NaN among them gives the whole range */
static void bounds(const double v[4], double pad, int *lo, int *hi) {
    double least = v[0], most = v[0];
    bool nan = false;
    for (int k = 0; k < 4; k++) {
        if (isnan(v[k])) nan = true;
        if (v[k] < least) least = v[k];
        if (v[k] > most) most = v[k];
    }
    least = floor(least) - pad;
    most = ceil(most) + pad;
    if (nan || least < -WINDOW_LIMIT) least = -WINDOW_LIMIT;
    if (least > WINDOW_LIMIT) least = WINDOW_LIMIT;
    if (nan || most > WINDOW_LIMIT) most = WINDOW_LIMIT;
    if (most < -WINDOW_LIMIT) most = -WINDOW_LIMIT;
    *lo = (int)least;
    *hi = (int)most;
}

static void target_window(const affine *a, int filter, const box2i *scur, const box2i *tfull, box2i *win) {
    const double g = cvs_warp_filter_reach(filter);
    const double sx[4] = { scur->min.x - g, scur->max.x + g, scur->min.x - g, scur->max.x + g };
    const double sy[4] = { scur->min.y - g, scur->min.y - g, scur->max.y + g, scur->max.y + g };
    double tx[4], ty[4];
    for (int k = 0; k < 4; k++) {
        tx[k] = a->f00 * sx[k] + a->f01 * sy[k] + a->f02;
        ty[k] = a->f10 * sx[k] + a->f11 * sy[k] + a->f12;
    }
    box2i reach;
    bounds(tx, 1.0, &reach.min.x, &reach.max.x);
    bounds(ty, 1.0, &reach.min.y, &reach.max.y);
    box2i_intersect(win, &reach, tfull);
    if (box2i_is_empty(win)) box2i_set_empty(win);
}

CVS_EXPORT int cvs_transform_target_window(const cvs_transform *t, const box2i *source_current, const box2i *target_full, box2i *win) {
    if (win) box2i_set_empty(win);
    if (!t || !source_current || !target_full || !win) { cvs_set_error("cvs_transform_target_window: need the transform and the three boxes"); return -1; }
    affine a;
    if (!affine_from(t, &a, "cvs_transform_target_window")) return -1;
    if (box2i_is_empty(source_current) || box2i_is_empty(target_full)) return 0;
    target_window(&a, t->filter, source_current, target_full, win);
    return 0;
}

CVS_EXPORT int cvs_transform_source_window(const cvs_transform *t, const box2i *target_window_, box2i *need) {
    if (need) box2i_set_empty(need);
    if (!t || !target_window_ || !need) { cvs_set_error("cvs_transform_source_window: need the transform and the two boxes"); return -1; }
    affine a;
    if (!affine_from(t, &a, "cvs_transform_source_window")) return -1;
    if (box2i_is_empty(target_window_)) return 0;
    const double tx[4] = { target_window_->min.x, target_window_->max.x, target_window_->min.x, target_window_->max.x };
    const double ty[4] = { target_window_->min.y, target_window_->min.y, target_window_->max.y, target_window_->max.y };
    double u[4], v[4];
    for (int k = 0; k < 4; k++) {
        u[k] = a.m[0] * tx[k] + a.m[1] * ty[k] + a.m[2];
        v[k] = a.m[3] * tx[k] + a.m[4] * ty[k] + a.m[5];
    }
    bounds(u, cvs_warp_filter_pad(t->filter), &need->min.x, &need->max.x);
    bounds(v, cvs_warp_filter_pad(t->filter), &need->min.y, &need->max.y);
    return 0;
}

CVS_EXPORT int cvs_transform_from_parts(const double anchor[2], const double scale[2], double rotation_degrees, const double position[2], float m[6]) {
    if (!anchor || !scale || !position || !m) { cvs_set_error("cvs_transform_from_parts: need anchor, scale, position and the six coefficients' place"); return -1; }
    if (!isfinite(anchor[0]) || !isfinite(anchor[1]) || !isfinite(scale[0]) || !isfinite(scale[1]) || !isfinite(rotation_degrees) ||
        !isfinite(position[0]) || !isfinite(position[1])) {
        cvs_set_error("cvs_transform_from_parts: anchor, scale, rotation and position must be finite");
        return -1;
    }
    if (scale[0] == 0.0 || scale[1] == 0.0) return 1;
    double q = fmod(rotation_degrees, 360.0);
    if (q < 0.0) q = q + 360.0;
    double c, s;
    if (q == 0.0) { c = 1.0; s = 0.0; }
    else if (q == 90.0) { c = 0.0; s = 1.0; }
    else if (q == 180.0) { c = -1.0; s = 0.0; }
    else if (q == 270.0) { c = 0.0; s = -1.0; }
    else { const double r = rotation_degrees * M_PI / 180.0; c = cos(r); s = sin(r); }
    const double f00 = scale[0] * c, f01 = -scale[1] * s, f10 = scale[0] * s, f11 = scale[1] * c;
    const double f02 = position[0] - (f00 * anchor[0] + f01 * anchor[1]), f12 = position[1] - (f10 * anchor[0] + f11 * anchor[1]);
    const double det = f00 * f11 - f01 * f10;
    double d[6];
    d[0] = f11 / det;
    d[1] = -f01 / det;
    d[3] = -f10 / det;
    d[4] = f00 / det;
    d[2] = -(d[0] * f02 + d[1] * f12);
    d[5] = -(d[3] * f02 + d[4] * f12);
    float r[6];
    for (int k = 0; k < 6; k++) {
        r[k] = (float)d[k];
        if (!isfinite(r[k])) { cvs_set_error("cvs_transform_from_parts: coefficient m[%d] of the inverse is not finite", k); return -1; }
    }
    memcpy(m, r, sizeof r);
    return 0;
}

static bool coords_exact(const box2i *b) {
    const int lim = CVS_TRANSFORM_MAX_COORD;
    return box2i_is_empty(b) || (b->min.x >= -lim && b->min.y >= -lim && b->max.x <= lim && b->max.y <= lim);
}

/* the two entries with their frames taken apart (the two frame structs differ in nothing but the pixel type) */
static int transform(void *tdata, const box2i *tfull, box2i *tcur, const void *sdata, const box2i *sfull, const box2i *scur,
                     const cvs_transform *t, int half, cvs_stream_t stream, const char *what) {
    box2i_set_empty(tcur);
    if (!cvs_box_contains(sfull, scur)) { cvs_set_error("%s: the input's current_window lies outside its buffer", what); return -1; }
    affine a;
    if (!affine_from(t, &a, what)) return -1;
    if (!coords_exact(scur) || !coords_exact(tfull)) {
        cvs_set_error("%s: a window coordinate lies beyond +-%d, where a float no longer holds every integer", what, CVS_TRANSFORM_MAX_COORD);
        return -1;
    }
    if (cvs_coords_refused(what, "source", sfull, scur, CVS_MAX_COORD) || cvs_coords_refused(what, "target", tfull, NULL, CVS_MAX_COORD)) return -1;
    if (tdata == sdata) { cvs_set_error("%s: the target is the source's buffer: the operation is not in place", what); return -1; }
    if (cvs_enter() != 0) return -1;
    if (box2i_is_empty(scur) || box2i_is_empty(tfull)) return 0;
    box2i win;
    target_window(&a, t->filter, scur, tfull, &win);
    if (box2i_is_empty(&win)) return 0;

    cvk_transform_params tp;
    memset(&tp, 0, sizeof tp);
    tp.out = cvs_view(tdata, tfull);
    tp.in = cvs_view((void *)sdata, sfull);
    tp.w = cvs_rect(&win);
    tp.s = cvs_rect(scur);
    memcpy(tp.m, t->m, sizeof tp.m);
    tp.bilinear = t->filter == CVS_TRANSFORM_BILINEAR;
    tile_plan(&tp);
    const int rc = t->filter == CVS_TRANSFORM_CATMULL_ROM ? cvk_transform_cubic(&tp, half, cvs_pick_stream(stream)) : cvk_transform(&tp, half, cvs_pick_stream(stream));
    if (rc != 0) { cvs_set_error("%s: %s", what, hipGetErrorString((hipError_t)rc)); return -1; }
    *tcur = win;
    return 0;
}

CVS_EXPORT int cvs_transform_f32_dev(rgba_frame_f32 *target, const rgba_frame_f32 *source, const cvs_transform *t, cvs_stream_t s) {
    if (!target || !source || !t) {
        if (target) box2i_set_empty(&target->current_window);
        cvs_set_error("cvs_transform_f32_dev: need the frames and the transform");
        return -1;
    }
    return transform(target->data, &target->full_window, &target->current_window, source->data, &source->full_window, &source->current_window, t, 0, s, "cvs_transform_f32_dev");
}

CVS_EXPORT int cvs_transform_f16_dev(rgba_frame_f16 *target, const rgba_frame_f16 *source, const cvs_transform *t, cvs_stream_t s) {
    if (!target || !source || !t) {
        if (target) box2i_set_empty(&target->current_window);
        cvs_set_error("cvs_transform_f16_dev: need the frames and the transform");
        return -1;
    }
    return transform(target->data, &target->full_window, &target->current_window, source->data, &source->full_window, &source->current_window, t, 1, s, "cvs_transform_f16_dev");
}
