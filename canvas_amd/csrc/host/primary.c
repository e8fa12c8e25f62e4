/*
 * primary.c -- cvs_primary_f32_dev / _f16_dev: per-channel 1D curves, a 3 x 4 matrix and per-channel 1D curves again in one pass,
 * with the host-side packer of a curve set.
 *
 * No reference code: the reference has no colour tool beyond gain/offset and the 3x3 matrix.  The contract is DESIGN.md "Primary
 * colour correction" and the comment of include/canvas_primary.h; refusals (in the header's order), window arithmetic and scale[]
 * (formed once per call) stay here, pixels go to kernels/primary_ops.hip.  The tables are the caller's device buffers: the entries
 * keep no state and record into a graph.  This file is compiled with -ffp-contract=off.
 */
#include "internal.h"
#include "canvas_primary.h"

static bool size_ok(int size) { return size >= CVS_CURVES_MIN_SIZE && size <= CVS_CURVES_MAX_SIZE; }

CVS_EXPORT size_t cvs_curves_bytes(int size) {
    if (!size_ok(size)) { cvs_set_error("cvs_curves_bytes: size %d, outside %d..%d", size, CVS_CURVES_MIN_SIZE, CVS_CURVES_MAX_SIZE); return 0; }
    return (size_t)12 * (size_t)size;
}

CVS_EXPORT int cvs_curves_pack(float *planar_host, const float *rgb_rows_host, int size) {
    if (!planar_host || !rgb_rows_host) { cvs_set_error("cvs_curves_pack: need both tables"); return -1; }
    if (!size_ok(size)) { cvs_set_error("cvs_curves_pack: size %d, outside %d..%d", size, CVS_CURVES_MIN_SIZE, CVS_CURVES_MAX_SIZE); return -1; }
    for (int k = 0; k < size * 3; k++)
        if (!isfinite(rgb_rows_host[k])) {
            cvs_set_error("cvs_curves_pack: value %d (node %d, channel %d) is not finite", k, k / 3, k % 3);
            return -1;
        }
    for (int k = 0; k < size; k++)
        for (int c = 0; c < 3; c++) planar_host[c * size + k] = rgb_rows_host[3 * k + c];
    return 0;
}

/* refusals 4 .. 7 of the header for one stage; 0: fine */
static int stage_refused(const char *what, const char *stage, const cvs_curves *cv, const float *table, int step) {
    if (cv->size == 0) {
        if (step == 7 && table) { cvs_set_error("%s: a table for the %s curves, which are absent (size 0)", what, stage); return -1; }
        return 0;
    }
    if (step == 4 && !size_ok(cv->size)) { cvs_set_error("%s: %s curves of size %d, outside %d..%d", what, stage, cv->size, CVS_CURVES_MIN_SIZE, CVS_CURVES_MAX_SIZE); return -1; }
    if (step == 5)
        for (int c = 0; c < 3; c++)
            if (!isfinite(cv->domain_min[c]) || !isfinite(cv->domain_max[c]) || !(cv->domain_min[c] < cv->domain_max[c])) {
                cvs_set_error("%s: domain %g..%g of channel %d of the %s curves must be finite and ascending", what, cv->domain_min[c], cv->domain_max[c], c, stage);
                return -1;
            }
    if (step == 6 && !table) { cvs_set_error("%s: the %s curves need their table", what, stage); return -1; }
    if (step == 6 && ((uintptr_t)table & 15u) != 0) { cvs_set_error("%s: the table of the %s curves is not on a 16-byte boundary", what, stage); return -1; }
    return 0;
}

static void stage_plan(const cvs_curves *cv, float *dmin, float *scale) {
    for (int c = 0; c < 3; c++) {
        const float width = cv->domain_max[c] - cv->domain_min[c];
        dmin[c] = cv->domain_min[c];
        scale[c] = (float)(cv->size - 1) / width;
    }
}

/* the two entries with their frames taken apart (the two frame structs differ in nothing but the pixel type) */
static int primary(void *tdata, const box2i *tfull, box2i *tcur, const void *sdata, const box2i *sfull, const box2i *scur,
                   const cvs_primary *p, const float *pre, const float *post, int half, cvs_stream_t stream, const char *what) {
    box2i_set_empty(tcur);
    const bool matrix = (p->flags & CVS_PRIMARY_MATRIX) != 0;
    if (p->pre.size == 0 && p->post.size == 0 && !matrix) { cvs_set_error("%s: no stage is present (no curves and no matrix)", what); return -1; }
    if ((p->flags & ~CVS_PRIMARY_MATRIX) != 0) { cvs_set_error("%s: unknown flags 0x%x", what, p->flags); return -1; }
    for (int step = 4; step <= 7; step++)
        if (stage_refused(what, "pre", &p->pre, pre, step) != 0 || stage_refused(what, "post", &p->post, post, step) != 0) return -1;
    if (matrix)
        for (int k = 0; k < 12; k++)
            if (!isfinite(p->matrix[k])) { cvs_set_error("%s: matrix entry %d (row %d) is not finite", what, k, k / 4); return -1; }
    if (!cvs_box_contains(sfull, scur)) { cvs_set_error("%s: the input's current_window lies outside its buffer", what); return -1; }
    if (cvs_coords_refused(what, "source", sfull, scur, CVS_MAX_COORD) || cvs_coords_refused(what, "target", tfull, NULL, CVS_MAX_COORD)) return -1;
    if (cvs_enter() != 0) return -1;
    box2i win;
    box2i_intersect(&win, scur, tfull);
    if (box2i_is_empty(scur) || box2i_is_empty(&win)) return 0;

    cvk_primary_params pp;
    memset(&pp, 0, sizeof pp);
    pp.pre = pre;
    pp.post = post;
    pp.kpre = p->pre.size;
    pp.kpost = p->post.size;
    if (pp.kpre) stage_plan(&p->pre, pp.pre_min, pp.pre_scale);
    if (pp.kpost) stage_plan(&p->post, pp.post_min, pp.post_scale);
    pp.matrix = matrix;
    if (matrix) memcpy(pp.m, p->matrix, sizeof pp.m);
    const int rc = cvk_primary(&pp, cvs_view(tdata, tfull), cvs_view((void *)sdata, sfull), cvs_rect(&win), half, cvs_cus(), cvs_pick_stream(stream));
    if (rc != 0) { cvs_set_error("%s: %s", what, hipGetErrorString((hipError_t)rc)); return -1; }
    *tcur = win;
    return 0;
}

CVS_EXPORT int cvs_primary_f32_dev(rgba_frame_f32 *target, const rgba_frame_f32 *source, const cvs_primary *p, const float *pre_dev, const float *post_dev, cvs_stream_t s) {
    if (!target || !source || !p) {
        if (target) box2i_set_empty(&target->current_window);
        cvs_set_error("cvs_primary_f32_dev: need the frames and the stage's description");
        return -1;
    }
    const box2i scur = source->current_window;          /* (a copy: the target may be the source frame itself) */
    return primary(target->data, &target->full_window, &target->current_window, source->data, &source->full_window, &scur, p, pre_dev, post_dev, 0, s, "cvs_primary_f32_dev");
}

CVS_EXPORT int cvs_primary_f16_dev(rgba_frame_f16 *target, const rgba_frame_f16 *source, const cvs_primary *p, const float *pre_dev, const float *post_dev, cvs_stream_t s) {
    if (!target || !source || !p) {
        if (target) box2i_set_empty(&target->current_window);
        cvs_set_error("cvs_primary_f16_dev: need the frames and the stage's description");
        return -1;
    }
    const box2i scur = source->current_window;
    return primary(target->data, &target->full_window, &target->current_window, source->data, &source->full_window, &scur, p, pre_dev, post_dev, 1, s, "cvs_primary_f16_dev");
}
