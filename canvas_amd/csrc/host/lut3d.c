/*
 * lut3d.c -- cvs_lut3d_f32_dev / _f16_dev: a 3D colour lookup table applied by tetrahedral interpolation, with the host-side
 * packer of its lattice.
 *
 * No reference code: the reference has no colour tool beyond gain/offset and the 3x3 matrix.  The contract is DESIGN.md "3D LUT"
 * and the comment of include/canvas_lut3d.h; refusals, window arithmetic and scale[] (formed once per call) stay here, pixels go
 * to kernels/lut3d_ops.hip.  The lattice is the caller's device buffer: the entries keep no state and record into a graph.
 * This file is compiled with -ffp-contract=off.
 */
#include "internal.h"
#include "canvas_lut3d.h"

static bool size_ok(int size) { return size >= CVS_LUT3D_MIN_SIZE && size <= CVS_LUT3D_MAX_SIZE; }

CVS_EXPORT size_t cvs_lut3d_bytes(int size) {
    if (!size_ok(size)) { cvs_set_error("cvs_lut3d_bytes: size %d, outside %d..%d", size, CVS_LUT3D_MIN_SIZE, CVS_LUT3D_MAX_SIZE); return 0; }
    return (size_t)16 * (size_t)size * (size_t)size * (size_t)size;
}

CVS_EXPORT int cvs_lut3d_pack(float *nodes4_host, const float *rgb_host, int size) {
    if (!nodes4_host || !rgb_host) { cvs_set_error("cvs_lut3d_pack: need both tables"); return -1; }
    if (!size_ok(size)) { cvs_set_error("cvs_lut3d_pack: size %d, outside %d..%d", size, CVS_LUT3D_MIN_SIZE, CVS_LUT3D_MAX_SIZE); return -1; }
    const size_t nodes = (size_t)size * (size_t)size * (size_t)size;
    for (size_t k = 0; k < nodes * 3; k++)
        if (!isfinite(rgb_host[k])) {
            cvs_set_error("cvs_lut3d_pack: value %zu (node %zu, channel %d) is not finite", k, k / 3, (int)(k % 3));
            return -1;
        }
    for (size_t k = 0; k < nodes; k++) {
        nodes4_host[4 * k + 0] = rgb_host[3 * k + 0];
        nodes4_host[4 * k + 1] = rgb_host[3 * k + 1];
        nodes4_host[4 * k + 2] = rgb_host[3 * k + 2];
        nodes4_host[4 * k + 3] = 0.0f;
    }
    return 0;
}

/* the two entries with their frames taken apart (the two frame structs differ in nothing but the pixel type) */
static int lut3d(void *tdata, const box2i *tfull, box2i *tcur, const void *sdata, const box2i *sfull, const box2i *scur,
                 const float *lattice, const cvs_lut3d *p, int half, cvs_stream_t stream, const char *what) {
    box2i_set_empty(tcur);
    if (((uintptr_t)lattice & 15u) != 0) { cvs_set_error("%s: the lattice is not on a 16-byte boundary", what); return -1; }
    if (!size_ok(p->size)) { cvs_set_error("%s: size %d, outside %d..%d", what, p->size, CVS_LUT3D_MIN_SIZE, CVS_LUT3D_MAX_SIZE); return -1; }
    for (int c = 0; c < 3; c++)
        if (!isfinite(p->domain_min[c]) || !isfinite(p->domain_max[c]) || !(p->domain_min[c] < p->domain_max[c])) {
            cvs_set_error("%s: domain %g..%g of channel %d must be finite and ascending", what, p->domain_min[c], p->domain_max[c], c);
            return -1;
        }
    if (p->flags != 0) { cvs_set_error("%s: unknown flags 0x%x", what, p->flags); return -1; }
    if (!cvs_box_contains(sfull, scur)) { cvs_set_error("%s: the input's current_window lies outside its buffer", what); return -1; }
    if (cvs_coords_refused(what, "source", sfull, scur, CVS_MAX_COORD) || cvs_coords_refused(what, "target", tfull, NULL, CVS_MAX_COORD)) return -1;
    if (cvs_enter() != 0) return -1;
    box2i win;
    box2i_intersect(&win, scur, tfull);
    if (box2i_is_empty(scur) || box2i_is_empty(&win)) return 0;

    cvk_lut3d_params lp;
    memset(&lp, 0, sizeof lp);
    lp.lattice = lattice;
    lp.n = p->size;
    for (int c = 0; c < 3; c++) {
        const float width = p->domain_max[c] - p->domain_min[c];
        lp.dmin[c] = p->domain_min[c];
        lp.scale[c] = (float)(p->size - 1) / width;
    }
    const int rc = cvk_lut3d(&lp, cvs_view(tdata, tfull), cvs_view((void *)sdata, sfull), cvs_rect(&win), half, cvs_cus(), cvs_pick_stream(stream));
    if (rc != 0) { cvs_set_error("%s: %s", what, hipGetErrorString((hipError_t)rc)); return -1; }
    *tcur = win;
    return 0;
}

CVS_EXPORT int cvs_lut3d_f32_dev(rgba_frame_f32 *target, const rgba_frame_f32 *source, const float *lattice_dev, const cvs_lut3d *p, cvs_stream_t s) {
    if (!target || !source || !lattice_dev || !p) {
        if (target) box2i_set_empty(&target->current_window);
        cvs_set_error("cvs_lut3d_f32_dev: need the frames, the lattice and the table's description");
        return -1;
    }
    const box2i scur = source->current_window;          /* (a copy: the target may be the source frame itself) */
    return lut3d(target->data, &target->full_window, &target->current_window, source->data, &source->full_window, &scur, lattice_dev, p, 0, s, "cvs_lut3d_f32_dev");
}

CVS_EXPORT int cvs_lut3d_f16_dev(rgba_frame_f16 *target, const rgba_frame_f16 *source, const float *lattice_dev, const cvs_lut3d *p, cvs_stream_t s) {
    if (!target || !source || !lattice_dev || !p) {
        if (target) box2i_set_empty(&target->current_window);
        cvs_set_error("cvs_lut3d_f16_dev: need the frames, the lattice and the table's description");
        return -1;
    }
    const box2i scur = source->current_window;
    return lut3d(target->data, &target->full_window, &target->current_window, source->data, &source->full_window, &scur, lattice_dev, p, 1, s, "cvs_lut3d_f16_dev");
}
