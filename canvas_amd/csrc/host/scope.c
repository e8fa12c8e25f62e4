/*
 * scope.c -- video scopes: cvs_scope_counts_f16_dev (histogram, waveform, RGB parade, vectorscope of an f16 frame as a table of
 * uint32 counters), cvs_scope_render_f16_dev (the picture of a table) and the host-frame twin video_scope_counts.
 *
 * No reference code: the reference has no scope.  The contract is DESIGN.md "Scopes" and the comment of include/canvas_scope.h.
 * Levels are the display edge's bytes, so the byte table is display.c's, from its cache (internal.h cvs_display_table_lock).
 * Refusals, window arithmetic and the zeroing of the table stay here; pixels go to kernels/scope_ops.hip.  No scratch, no host
 * synchronisation and no host read of frame contents: both device entries record into a graph.
 */
#include "internal.h"
#include "canvas_scope.h"

static bool known_kind(int kind) { return kind >= CVS_SCOPE_HISTOGRAM && kind <= CVS_SCOPE_VECTORSCOPE; }
static bool has_columns(int kind) { return kind == CVS_SCOPE_WAVEFORM || kind == CVS_SCOPE_PARADE; }

/* what both device entries refuse about the struct alone, in the contract's order: true with the error set */
static bool params_refused(const char *what, const cvs_scope *p) {
    if (!known_kind(p->kind)) { cvs_set_error("%s: unknown kind %d", what, p->kind); return true; }
    if (p->flags & ~CVS_SCOPE_SKIP_TRANSPARENT) { cvs_set_error("%s: unknown flags 0x%x", what, p->flags); return true; }
    if (p->pre_lut != CVS_LUT_NONE && (p->pre_lut < 0 || p->pre_lut >= CVS_LUT_COUNT)) { cvs_set_error("%s: no such transfer table: %d", what, p->pre_lut); return true; }
    if (!isfinite(p->rendering_intent) || p->rendering_intent < 0.0f) { cvs_set_error("%s: rendering_intent %g must be finite and not negative", what, p->rendering_intent); return true; }
    if (has_columns(p->kind) && (p->columns < 1 || p->columns > CVS_SCOPE_MAX_COLUMNS)) {
        cvs_set_error("%s: %d columns, outside 1..%d", what, p->columns, CVS_SCOPE_MAX_COLUMNS);
        return true;
    }
    return false;
}

CVS_EXPORT size_t cvs_scope_count(const cvs_scope *p) {
    if (!p) { cvs_set_error("cvs_scope_count: need the scope"); return 0; }
    if (!known_kind(p->kind)) { cvs_set_error("cvs_scope_count: unknown kind %d", p->kind); return 0; }
    if (has_columns(p->kind) && (p->columns < 1 || p->columns > CVS_SCOPE_MAX_COLUMNS)) {
        cvs_set_error("cvs_scope_count: %d columns, outside 1..%d", p->columns, CVS_SCOPE_MAX_COLUMNS);
        return 0;
    }
    switch (p->kind) {
    case CVS_SCOPE_HISTOGRAM: return 5 * 256;
    case CVS_SCOPE_WAVEFORM: return (size_t)p->columns * 256;
    case CVS_SCOPE_PARADE: return (size_t)3 * (size_t)p->columns * 256;
    default: return 256 * 256;
    }
}

CVS_EXPORT int cvs_scope_picture_size(const cvs_scope *p, v2i *size) {
    if (!p || !size) { cvs_set_error("cvs_scope_picture_size: need the scope and the size"); return -1; }
    if (p->kind == CVS_SCOPE_HISTOGRAM) { cvs_set_error("cvs_scope_picture_size: a histogram has no picture"); return -1; }
    if (cvs_scope_count(p) == 0) return -1;
    size->x = p->kind == CVS_SCOPE_WAVEFORM ? p->columns : p->kind == CVS_SCOPE_PARADE ? 3 * p->columns : 256;
    size->y = 256;
    return 0;
}

/* everything cvs_scope_counts_f16_dev refuses, in the contract's order, without touching the device */
static bool counts_refused(const char *what, const void *counts, const rgba_frame_f16 *frame, const cvs_scope *p) {
    if (!counts || !frame || !p) { cvs_set_error("%s: need the table, the frame and the scope", what); return true; }
    if (((uintptr_t)counts & 3u) != 0) { cvs_set_error("%s: the table is not on a 4-byte boundary", what); return true; }
    if (params_refused(what, p)) return true;
    if (box2i_is_empty(&p->region)) { cvs_set_error("%s: the region is empty", what); return true; }
    if (!cvs_box_contains(&frame->full_window, &frame->current_window)) { cvs_set_error("%s: the frame's current_window lies outside its buffer", what); return true; }
    if (cvs_coords_refused(what, "frame", &frame->full_window, &frame->current_window, CVS_MAX_COORD)) return true;
    if (!cvs_box_within(&p->region, CVS_MAX_COORD)) {
        cvs_set_error("%s: region (%d, %d)-(%d, %d) has a coordinate beyond +-%d (CVS_MAX_COORD)", what, p->region.min.x, p->region.min.y, p->region.max.x, p->region.max.y, CVS_MAX_COORD);
        return true;
    }
    box2i m;
    box2i_intersect(&m, &p->region, &frame->current_window);
    if (!box2i_is_empty(&frame->current_window) && !box2i_is_empty(&m) && (unsigned long long)cvs_box_width(&m) * (unsigned long long)cvs_box_height(&m) >= (1ull << 32)) {
        cvs_set_error("%s: %lld x %lld pixels to measure, more than a 32-bit counter holds", what, cvs_box_width(&m), cvs_box_height(&m));
        return true;
    }
    return false;
}

CVS_EXPORT int cvs_scope_counts_f16_dev(uint32_t *counts_dev, const rgba_frame_f16 *frame, const cvs_scope *p, cvs_stream_t stream) {
    static const char *what = "cvs_scope_counts_f16_dev";
    if (counts_refused(what, counts_dev, frame, p)) return -1;
    if (cvs_enter() != 0) return -1;
    hipStream_t s = cvs_pick_stream(stream);
    const size_t bytes = cvs_scope_count(p) * sizeof(uint32_t);
    box2i m;
    box2i_intersect(&m, &p->region, &frame->current_window);
    if (box2i_is_empty(&frame->current_window) || box2i_is_empty(&m)) {
        CVS_HIP(hipMemsetAsync(counts_dev, 0, bytes, s));
        return 0;
    }
    /* the table first: a call that finds none has enqueued nothing */
    int slot = -1;
    const uint8_t *table = cvs_display_table_lock(p->pre_lut, p->rendering_intent, &slot);
    if (!table) return -1;
    int rc = (int)hipMemsetAsync(counts_dev, 0, bytes, s);
    if (rc == 0) rc = cvk_scope_counts(counts_dev, cvs_view(frame->data, &frame->full_window), cvs_rect(&m), table, p->kind, p->region.min.x, cvs_box_width(&p->region),
                                       has_columns(p->kind) ? p->columns : 1, (p->flags & CVS_SCOPE_SKIP_TRANSPARENT) != 0, cvs_cus(), s);
    cvs_display_table_unlock(slot, rc == 0, s);
    if (rc != 0) { cvs_set_error("%s: %s", what, hipGetErrorString((hipError_t)rc)); return -1; }
    return 0;
}

CVS_EXPORT int cvs_scope_render_f16_dev(rgba_frame_f16 *target, const box2i *place, const uint32_t *counts_dev, const cvs_scope *p, float gain, cvs_stream_t stream) {
    static const char *what = "cvs_scope_render_f16_dev";
    if (target) box2i_set_empty(&target->current_window);
    if (!target || !place || !counts_dev || !p) { cvs_set_error("%s: need the target, the place, the table and the scope", what); return -1; }
    if (((uintptr_t)counts_dev & 3u) != 0) { cvs_set_error("%s: the table is not on a 4-byte boundary", what); return -1; }
    if (p->kind == CVS_SCOPE_HISTOGRAM) { cvs_set_error("%s: a histogram has no picture", what); return -1; }
    if (params_refused(what, p)) return -1;
    v2i size;
    if (cvs_scope_picture_size(p, &size) != 0) return -1;
    if (box2i_is_empty(place) || cvs_box_width(place) != size.x || cvs_box_height(place) != size.y) {
        cvs_set_error("%s: place (%d, %d)-(%d, %d) is not the picture's %d x %d", what, place->min.x, place->min.y, place->max.x, place->max.y, size.x, size.y);
        return -1;
    }
    /* A picture larger than its target overhangs it, and so overhangs the coordinate bound where the target lies on it: `place` is
     * clipped, and what is formed from it (x - place.min.x inside the clipped window) stays below the picture's size.  A place
     * no pixel of which lies within the bound reaches no target the contract allows: refused, as a coordinate beyond it. */
    if (place->min.x > CVS_MAX_COORD || place->min.y > CVS_MAX_COORD || place->max.x < -CVS_MAX_COORD || place->max.y < -CVS_MAX_COORD) {
        cvs_set_error("%s: place (%d, %d)-(%d, %d) lies beyond +-%d (CVS_MAX_COORD)", what, place->min.x, place->min.y, place->max.x, place->max.y, CVS_MAX_COORD);
        return -1;
    }
    if (cvs_coords_refused(what, "target", &target->full_window, NULL, CVS_MAX_COORD)) return -1;
    if (!isfinite(gain) || gain < 0.0f) { cvs_set_error("%s: gain %g must be finite and not negative", what, gain); return -1; }
    if (cvs_enter() != 0) return -1;
    box2i win;
    box2i_intersect(&win, place, &target->full_window);
    if (box2i_is_empty(&win)) return 0;
    const int rc = cvk_scope_render(cvs_view(target->data, &target->full_window), cvs_rect(&win), place->min.x, place->min.y, counts_dev, p->kind, p->columns, gain, cvs_pick_stream(stream));
    if (rc != 0) { cvs_set_error("%s: %s", what, hipGetErrorString((hipError_t)rc)); return -1; }
    target->current_window = win;
    return 0;
}

/* the counts of a HOST frame into a HOST table: the rows of the current window go up, the counters come back */
CVS_EXPORT int video_scope_counts(uint32_t *counts_host, const rgba_frame_f16 *frame, const cvs_scope *p) {
    static const char *what = "video_scope_counts";
    if (counts_refused(what, counts_host, frame, p)) return -1;            /* before a byte is staged */
    if (cvs_enter() != 0) return -1;
    const size_t out_bytes = cvs_scope_count(p) * sizeof(uint32_t);
    const box2i *w = &frame->current_window;
    hipStream_t s = cvs_pick_stream(NULL);
    /* only the rows of the current window travel: a device frame whose full window is that band of rows */
    rgba_frame_f16 band = *frame;
    cvs_staged din = { 0 }, dout = { 0 };
    int rc = 0;
    if (!box2i_is_empty(w)) {
        band.full_window.min.y = w->min.y; band.full_window.max.y = w->max.y;
        const size_t pitch = (size_t)cvs_box_width(&frame->full_window);
        rc = cvs_stage_in(&din, frame->data + (size_t)(w->min.y - frame->full_window.min.y) * pitch, cvs_box_pixels(&band.full_window) * sizeof(rgba_f16), 1, s);
        band.data = din.dev;
    }
    if (rc == 0) rc = cvs_stage_in(&dout, NULL, out_bytes, 0, s);
    if (rc == 0) rc = cvs_scope_counts_f16_dev(dout.dev, &band, p, s);
    if (rc == 0) rc = cvs_stage_out(&dout, counts_host, s);
    cvs_stage_free(&din); cvs_stage_free(&dout);
    return rc;
}
