/*
 * perspective.c -- cvs_perspective_f32_dev / _f16_dev: the corner pin, a projective warp with the transform's alpha-weighted
 * bilinear or Catmull-Rom filter, and the host arithmetic that goes with it (the nine coefficients from a quad; the target and source windows).
 *
 * No reference code.  The contract is DESIGN.md "Corner pin" and the comment of include/canvas_perspective.h; refusals, the
 * windows and the origins stay here, pixels go to kernels/perspective_ops.hip (Catmull-Rom: kernels/warp_cubic_ops.hip).  All host arithmetic is in double, every
 * operation rounded on its own (this file is compiled with -ffp-contract=off), written in the order DESIGN.md gives so that the
 * numpy model of the tests (tests/perspective_model.py) repeats it exactly.
 */
#include "internal.h"
#include "canvas_perspective.h"

#define WINDOW_LIMIT 1073741824.0                       /* 2^30: what a window bound or an origin is clamped to before it becomes an int */

/* (which filters there are, their reach and the source window's pad: internal.h, shared by the two warps) */

/* h widened, with its adjugate over its determinant (the SOURCE -> TARGET map); false with the error set where the contract refuses */
typedef struct { double h[9], det, f[9]; } projective;
static bool projective_from(const cvs_perspective *p, projective *a, const char *what) {
    if (!cvs_warp_filter_known(p->filter)) { cvs_set_error(CVS_WARP_FILTER_REFUSAL, what, p->filter); return false; }
    if (p->flags != 0) { cvs_set_error("%s: unknown flags 0x%x", what, (unsigned)p->flags); return false; }
    for (int k = 0; k < 9; k++) {
        if (!isfinite(p->h[k])) { cvs_set_error("%s: coefficient h[%d] is not finite", what, k); return false; }
        a->h[k] = (double)p->h[k];
    }
    const double *h = a->h;
    double adj[9];
    adj[0] = h[4] * h[8] - h[5] * h[7];
    adj[1] = h[2] * h[7] - h[1] * h[8];
    adj[2] = h[1] * h[5] - h[2] * h[4];
    adj[3] = h[5] * h[6] - h[3] * h[8];
    adj[4] = h[0] * h[8] - h[2] * h[6];
    adj[5] = h[2] * h[3] - h[0] * h[5];
    adj[6] = h[3] * h[7] - h[4] * h[6];
    adj[7] = h[1] * h[6] - h[0] * h[7];
    adj[8] = h[0] * h[4] - h[1] * h[3];
    a->det = (h[0] * adj[0] + h[1] * adj[3]) + h[2] * adj[6];
    if (a->det == 0.0 || !isfinite(a->det)) { cvs_set_error("%s: the determinant of h is %g: the map cannot be inverted", what, a->det); return false; }
    for (int k = 0; k < 9; k++) a->f[k] = adj[k] / a->det;
    return true;
}

static double clamp_limit(double v) { return v < -WINDOW_LIMIT ? -WINDOW_LIMIT : (v > WINDOW_LIMIT ? WINDOW_LIMIT : v); }

/* [floor(lo) - pad, ceil(hi) + pad] of the four values, plus the origin, each bound clamped to +-2^30; a NaN gives the whole range */
static void bounds(const double v[4], double pad, int origin, int *lo, int *hi) {
    double least = v[0], most = v[0];
    bool nan = false;
    for (int k = 0; k < 4; k++) {
        if (isnan(v[k])) nan = true;
        if (v[k] < least) least = v[k];
        if (v[k] > most) most = v[k];
    }
    least = (floor(least) - pad) + (double)origin;
    most = (ceil(most) + pad) + (double)origin;
    if (nan || isnan(least)) least = -WINDOW_LIMIT;
    if (nan || isnan(most)) most = WINDOW_LIMIT;
    *lo = (int)clamp_limit(least);
    *hi = (int)clamp_limit(most);
}

static void target_window(const cvs_perspective *p, const projective *a, const box2i *scur, const box2i *tfull, box2i *win) {
    const double g = cvs_warp_filter_reach(p->filter);
    const double x0 = (double)((long long)scur->min.x - p->source_origin[0]) - g, x1 = (double)((long long)scur->max.x - p->source_origin[0]) + g;
    const double y0 = (double)((long long)scur->min.y - p->source_origin[1]) - g, y1 = (double)((long long)scur->max.y - p->source_origin[1]) + g;
    const double sx[4] = { x0, x1, x0, x1 }, sy[4] = { y0, y0, y1, y1 };
    const double *f = a->f;
    double tx[4], ty[4];
    bool folded = false;
    for (int k = 0; k < 4; k++) {
        const double nx = (f[0] * sx[k] + f[1] * sy[k]) + f[2], ny = (f[3] * sx[k] + f[4] * sy[k]) + f[5], w = (f[6] * sx[k] + f[7] * sy[k]) + f[8];
        if (!(w > 0.0)) folded = true;
        tx[k] = nx / w;
        ty[k] = ny / w;
    }
    if (folded) { *win = *tfull; return; }             /* part of S on the vanishing line: its picture has no bound */
    box2i reach;
    bounds(tx, 1.0, p->target_origin[0], &reach.min.x, &reach.max.x);
    bounds(ty, 1.0, p->target_origin[1], &reach.min.y, &reach.max.y);
    box2i_intersect(win, &reach, tfull);
    if (box2i_is_empty(win)) box2i_set_empty(win);
}

CVS_EXPORT int cvs_perspective_target_window(const cvs_perspective *p, const box2i *source_current, const box2i *target_full, box2i *win) {
    if (win) box2i_set_empty(win);
    if (!p || !source_current || !target_full || !win) { cvs_set_error("cvs_perspective_target_window: need the map and the three boxes"); return -1; }
    projective a;
    if (!projective_from(p, &a, "cvs_perspective_target_window")) return -1;
    if (box2i_is_empty(source_current) || box2i_is_empty(target_full)) return 0;
    target_window(p, &a, source_current, target_full, win);
    return 0;
}

CVS_EXPORT int cvs_perspective_source_window(const cvs_perspective *p, const box2i *target_window_, box2i *need) {
    if (need) box2i_set_empty(need);
    if (!p || !target_window_ || !need) { cvs_set_error("cvs_perspective_source_window: need the map and the two boxes"); return -1; }
    projective a;
    if (!projective_from(p, &a, "cvs_perspective_source_window")) return -1;
    if (box2i_is_empty(target_window_)) return 0;
    const double x0 = (double)((long long)target_window_->min.x - p->target_origin[0]), x1 = (double)((long long)target_window_->max.x - p->target_origin[0]);
    const double y0 = (double)((long long)target_window_->min.y - p->target_origin[1]), y1 = (double)((long long)target_window_->max.y - p->target_origin[1]);
    const double tx[4] = { x0, x1, x0, x1 }, ty[4] = { y0, y0, y1, y1 };
    const double *h = a.h;
    double u[4], v[4];
    bool folded = false;
    for (int k = 0; k < 4; k++) {
        const double nu = (h[0] * tx[k] + h[1] * ty[k]) + h[2], nv = (h[3] * tx[k] + h[4] * ty[k]) + h[5], w = (h[6] * tx[k] + h[7] * ty[k]) + h[8];
        if (!(w > 0.0)) folded = true;
        u[k] = nu / w;
        v[k] = nv / w;
    }
    if (folded) {                                        /* the window reaches the vanishing line: any source pixel may be asked for */
        need->min.x = need->min.y = (int)-WINDOW_LIMIT;
        need->max.x = need->max.y = (int)WINDOW_LIMIT;
        return 0;
    }
    bounds(u, cvs_warp_filter_pad(p->filter), p->source_origin[0], &need->min.x, &need->max.x);
    bounds(v, cvs_warp_filter_pad(p->filter), p->source_origin[1], &need->min.y, &need->max.y);
    return 0;
}

CVS_EXPORT int cvs_perspective_from_quad(const double source_rect[4], const double quad[4][2], int filter, cvs_perspective *p) {
    if (!source_rect || !quad || !p) { cvs_set_error("cvs_perspective_from_quad: need the rectangle, the four corners and the map's place"); return -1; }
    for (int k = 0; k < 4; k++)
        if (!isfinite(source_rect[k]) || !isfinite(quad[k][0]) || !isfinite(quad[k][1])) {
            cvs_set_error("cvs_perspective_from_quad: the rectangle and the corners must be finite");
            return -1;
        }
    if (!(source_rect[2] > source_rect[0]) || !(source_rect[3] > source_rect[1])) {
        cvs_set_error("cvs_perspective_from_quad: the rectangle (%g, %g)-(%g, %g) is not ascending", source_rect[0], source_rect[1], source_rect[2], source_rect[3]);
        return -1;
    }
    if (!cvs_warp_filter_known(filter)) { cvs_set_error(CVS_WARP_FILTER_REFUSAL, "cvs_perspective_from_quad", filter); return -1; }

    const double tox = clamp_limit(floor(((quad[0][0] + quad[1][0]) + (quad[2][0] + quad[3][0])) / 4.0));
    const double toy = clamp_limit(floor(((quad[0][1] + quad[1][1]) + (quad[2][1] + quad[3][1])) / 4.0));
    const double sox = clamp_limit(floor((source_rect[0] + source_rect[2]) / 2.0)), soy = clamp_limit(floor((source_rect[1] + source_rect[3]) / 2.0));
    double x[4], y[4];
    for (int k = 0; k < 4; k++) { x[k] = quad[k][0] - tox; y[k] = quad[k][1] - toy; }
    const double rx0 = source_rect[0] - sox, ry0 = source_rect[1] - soy, rx1 = source_rect[2] - sox, ry1 = source_rect[3] - soy;
    const double W = rx1 - rx0, H = ry1 - ry0;

    int positive = 0, negative = 0;
    for (int k = 0; k < 4; k++) {
        const int k1 = (k + 1) & 3, k2 = (k + 2) & 3;
        const double c = (x[k1] - x[k]) * (y[k2] - y[k1]) - (y[k1] - y[k]) * (x[k2] - x[k1]);
        if (c > 0.0) positive++;
        if (c < 0.0) negative++;
    }
    if (positive != 4 && negative != 4) return 1;      /* concave, crossed or flat: nothing to draw */

    double r[9];
    const double sx = (x[0] - x[1]) + (x[2] - x[3]), sy = (y[0] - y[1]) + (y[2] - y[3]);
    if (sx == 0.0 && sy == 0.0) {
        const double f00 = (x[1] - x[0]) / W, f01 = (x[3] - x[0]) / H, f10 = (y[1] - y[0]) / W, f11 = (y[3] - y[0]) / H;
        const double f02 = x[0] - (f00 * rx0 + f01 * ry0), f12 = y[0] - (f10 * rx0 + f11 * ry0);
        const double det = f00 * f11 - f01 * f10;
        r[0] = f11 / det;
        r[1] = -f01 / det;
        r[3] = -f10 / det;
        r[4] = f00 / det;
        r[2] = -(r[0] * f02 + r[1] * f12);
        r[5] = -(r[3] * f02 + r[4] * f12);
        r[6] = 0.0; r[7] = 0.0; r[8] = 1.0;
    } else {
        const double dx1 = x[1] - x[2], dx2 = x[3] - x[2], dy1 = y[1] - y[2], dy2 = y[3] - y[2], den = dx1 * dy2 - dx2 * dy1;
        const double g = (sx * dy2 - dx2 * sy) / den, hh = (dx1 * sy - sx * dy1) / den;
        const double a = (x[1] - x[0]) + g * x[1], b = (x[3] - x[0]) + hh * x[3], c = x[0];
        const double d = (y[1] - y[0]) + g * y[1], e = (y[3] - y[0]) + hh * y[3], f = y[0];
        const double a0[3] = { e - f * hh, c * hh - b, b * f - c * e };
        const double a1[3] = { f * g - d, a - c * g, c * d - a * f };
        const double a2[3] = { d * hh - e * g, b * g - a * hh, a * e - b * d };
        for (int k = 0; k < 3; k++) {
            r[k] = rx0 * a2[k] + W * a0[k];
            r[3 + k] = ry0 * a2[k] + H * a1[k];
            r[6 + k] = a2[k];
        }
        const double cx = ((x[0] + x[1]) + (x[2] + x[3])) / 4.0, cy = ((y[0] + y[1]) + (y[2] + y[3])) / 4.0;
        const double wc = (r[6] * cx + r[7] * cy) + r[8];
        for (int k = 0; k < 9; k++) r[k] = r[k] / wc;
    }
    cvs_perspective out;
    memset(&out, 0, sizeof out);
    for (int k = 0; k < 9; k++) {
        out.h[k] = (float)r[k];
        if (!isfinite(out.h[k])) { cvs_set_error("cvs_perspective_from_quad: coefficient h[%d] of the map is not finite", k); return -1; }
    }
    out.target_origin[0] = (int)tox; out.target_origin[1] = (int)toy;
    out.source_origin[0] = (int)sox; out.source_origin[1] = (int)soy;
    out.filter = filter;
    *p = out;
    return 0;
}

/* every coordinate of b - origin, formed in 64 bit, within +-CVS_PERSPECTIVE_MAX_SPAN (an exact float, then) */
static bool span_refused(const char *what, const char *operand, const box2i *b, const int origin[2]) {
    if (box2i_is_empty(b)) return false;
    const long long lim = CVS_PERSPECTIVE_MAX_SPAN;
    const long long v[4] = { (long long)b->min.x - origin[0], (long long)b->min.y - origin[1], (long long)b->max.x - origin[0], (long long)b->max.y - origin[1] };
    for (int k = 0; k < 4; k++)
        if (v[k] < -lim || v[k] > lim) {
            cvs_set_error("%s: %s (%d, %d)-(%d, %d) has a coordinate beyond +-%d of its origin (%d, %d), where a float no longer holds every integer",
                          what, operand, b->min.x, b->min.y, b->max.x, b->max.y, CVS_PERSPECTIVE_MAX_SPAN, origin[0], origin[1]);
            return true;
        }
    return false;
}

/* the two entries with their frames taken apart (the two frame structs differ in nothing but the pixel type) */
static int perspective(void *tdata, const box2i *tfull, box2i *tcur, const void *sdata, const box2i *sfull, const box2i *scur,
                       const cvs_perspective *p, int half, cvs_stream_t stream, const char *what) {
    box2i_set_empty(tcur);
    if (!cvs_box_contains(sfull, scur)) { cvs_set_error("%s: the input's current_window lies outside its buffer", what); return -1; }
    projective a;
    if (!projective_from(p, &a, what)) return -1;
    if (cvs_coords_refused(what, "source", sfull, scur, CVS_MAX_COORD) || cvs_coords_refused(what, "target", tfull, NULL, CVS_MAX_COORD)) return -1;
    if (span_refused(what, "the target's full_window", tfull, p->target_origin) || span_refused(what, "the source's current_window", scur, p->source_origin)) return -1;
    if (tdata == sdata) { cvs_set_error("%s: the target is the source's buffer: the operation is not in place", what); return -1; }
    if (cvs_enter() != 0) return -1;
    if (box2i_is_empty(scur) || box2i_is_empty(tfull)) return 0;
    box2i win;
    target_window(p, &a, scur, tfull, &win);
    if (box2i_is_empty(&win)) return 0;

    cvk_perspective_params pp;
    memset(&pp, 0, sizeof pp);
    pp.out = cvs_view(tdata, tfull);
    pp.in = cvs_view((void *)sdata, sfull);
    pp.w.x0 = win.min.x - p->target_origin[0]; pp.w.x1 = win.max.x - p->target_origin[0];       /* (within the span: no overflow) */
    pp.w.y0 = win.min.y - p->target_origin[1]; pp.w.y1 = win.max.y - p->target_origin[1];
    pp.s.x0 = scur->min.x - p->source_origin[0]; pp.s.x1 = scur->max.x - p->source_origin[0];
    pp.s.y0 = scur->min.y - p->source_origin[1]; pp.s.y1 = scur->max.y - p->source_origin[1];
    pp.tdx = (long long)p->target_origin[0] - tfull->min.x; pp.tdy = (long long)p->target_origin[1] - tfull->min.y;
    pp.sdx = (long long)p->source_origin[0] - sfull->min.x; pp.sdy = (long long)p->source_origin[1] - sfull->min.y;
    memcpy(pp.h, p->h, sizeof pp.h);
    pp.bilinear = p->filter == CVS_TRANSFORM_BILINEAR;
    const int rc = p->filter == CVS_TRANSFORM_CATMULL_ROM ? cvk_perspective_cubic(&pp, half, cvs_pick_stream(stream)) : cvk_perspective(&pp, half, cvs_pick_stream(stream));
    if (rc != 0) { cvs_set_error("%s: %s", what, hipGetErrorString((hipError_t)rc)); return -1; }
    *tcur = win;
    return 0;
}

CVS_EXPORT int cvs_perspective_f32_dev(rgba_frame_f32 *target, const rgba_frame_f32 *source, const cvs_perspective *p, cvs_stream_t s) {
    if (!target || !source || !p) {
        if (target) box2i_set_empty(&target->current_window);
        cvs_set_error("cvs_perspective_f32_dev: need the frames and the map");
        return -1;
    }
    return perspective(target->data, &target->full_window, &target->current_window, source->data, &source->full_window, &source->current_window, p, 0, s, "cvs_perspective_f32_dev");
}

CVS_EXPORT int cvs_perspective_f16_dev(rgba_frame_f16 *target, const rgba_frame_f16 *source, const cvs_perspective *p, cvs_stream_t s) {
    if (!target || !source || !p) {
        if (target) box2i_set_empty(&target->current_window);
        cvs_set_error("cvs_perspective_f16_dev: need the frames and the map");
        return -1;
    }
    return perspective(target->data, &target->full_window, &target->current_window, source->data, &source->full_window, &source->current_window, p, 1, s, "cvs_perspective_f16_dev");
}
