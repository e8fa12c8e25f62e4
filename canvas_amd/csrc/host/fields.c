/*
 * fields.c -- conversions between woven (interlaced) frames and whole pictures: one field to a frame, vertical softening
 * before a weave, two pictures woven into one frame, and the frame arithmetic of 2:3 pulldown addition.
 *
 * No reference code: the design lists these conversions (docs/sphinx/feature-proposal/canvas.rst:283-303) and the editor names
 * them (fluggo/editor/model/sources.py:536-542), only the pulldown removal was built (src/process/Pulldown23RemovalFilter.c;
 * frames.c here).  The contract is DESIGN.md "Field conversions" and the comments of include/canvas_hip.h; window arithmetic
 * stays on the host, pixels go to kernels/field_ops.hip.  The kernels hold no a * b + c that a contraction could change
 * (every product is by a power of two, exact), so there is one build of them and no CVK() here.
 */
#include "internal.h"

/* what the three device entries check before any device call: frames present, distinct buffers, every input's current window
 * inside its buffer.  The output's window is empty from here on until the call has succeeded. */
static int fields_enter(const char *what, rgba_frame_f16 *out, const rgba_frame_f16 *a, const rgba_frame_f16 *b) {
    if (out) box2i_set_empty(&out->current_window);
    if (!out || !a || !b) { cvs_set_error("%s: need the frames", what); return -1; }
    if (out->data == a->data || out->data == b->data) { cvs_set_error("%s: the output cannot be one of the inputs", what); return -1; }
    if (!cvs_box_contains(&a->full_window, &a->current_window) || !cvs_box_contains(&b->full_window, &b->current_window)) {
        cvs_set_error("%s: an input's current_window lies outside its buffer", what);
        return -1;
    }
    if (cvs_coords_refused(what, "out", &out->full_window, NULL, CVS_MAX_COORD) || cvs_coords_refused(what, "an input", &a->full_window, &a->current_window, CVS_MAX_COORD) ||
        cvs_coords_refused(what, "an input", &b->full_window, &b->current_window, CVS_MAX_COORD)) return -1;
    return cvs_enter();
}

CVS_EXPORT int cvs_field_to_frame_f16_dev(rgba_frame_f16 *out, const rgba_frame_f16 *in, int field, cvs_stream_t s) {
    if (out) box2i_set_empty(&out->current_window);
    if (field != 0 && field != 1) { cvs_set_error("cvs_field_to_frame_f16_dev: field %d is neither 0 (even rows) nor 1 (odd rows)", field); return -1; }
    if (fields_enter("cvs_field_to_frame_f16_dev", out, in, in) != 0) return -1;
    box2i w;
    box2i_intersect(&w, &out->full_window, &in->current_window);
    if (box2i_is_empty(&in->current_window) || box2i_is_empty(&w)) return 0;
    const int rc = cvk_field_to_frame(cvs_view(out->data, &out->full_window), cvs_view(in->data, &in->full_window), cvs_rect(&w),
                                      cvs_rect(&in->current_window), field, cvs_cus(), cvs_pick_stream(s));
    if (rc != 0) { cvs_set_error("cvs_field_to_frame_f16_dev: %s", hipGetErrorString((hipError_t)rc)); return rc; }
    out->current_window = w;
    return 0;
}

CVS_EXPORT int cvs_soften_fields_f16_dev(rgba_frame_f16 *out, const rgba_frame_f16 *in, cvs_stream_t s) {
    if (fields_enter("cvs_soften_fields_f16_dev", out, in, in) != 0) return -1;
    box2i w;
    box2i_intersect(&w, &out->full_window, &in->current_window);
    if (box2i_is_empty(&in->current_window) || box2i_is_empty(&w)) return 0;
    const int rc = cvk_soften_fields(cvs_view(out->data, &out->full_window), cvs_view(in->data, &in->full_window), cvs_rect(&w),
                                     cvs_rect(&in->current_window), cvs_cus(), cvs_pick_stream(s));
    if (rc != 0) { cvs_set_error("cvs_soften_fields_f16_dev: %s", hipGetErrorString((hipError_t)rc)); return rc; }
    out->current_window = w;
    return 0;
}

CVS_EXPORT int cvs_interlace_fields_f16_dev(rgba_frame_f16 *out, const rgba_frame_f16 *even, const rgba_frame_f16 *odd, cvs_stream_t s) {
    if (fields_enter("cvs_interlace_fields_f16_dev", out, even, odd) != 0) return -1;
    /* the bounding box of the inputs that have pixels (gl.c:604-606), clipped to the buffer */
    const bool have_even = !box2i_is_empty(&even->current_window), have_odd = !box2i_is_empty(&odd->current_window);
    if (!have_even && !have_odd) return 0;
    box2i w = have_even ? even->current_window : odd->current_window;
    if (have_even && have_odd) box2i_union(&w, &even->current_window, &odd->current_window);
    box2i_intersect(&w, &w, &out->full_window);
    if (box2i_is_empty(&w)) return 0;
    const int rc = cvk_interlace_fields(cvs_view(out->data, &out->full_window), cvs_view(even->data, &even->full_window),
                                        cvs_view(odd->data, &odd->full_window), cvs_rect(&w), cvs_rect(&even->current_window),
                                        cvs_rect(&odd->current_window), cvs_cus(), cvs_pick_stream(s));
    if (rc != 0) { cvs_set_error("cvs_interlace_fields_f16_dev: %s", hipGetErrorString((hipError_t)rc)); return rc; }
    out->current_window = w;
    return 0;
}

/* The inverse of cvs_pulldown23_frames (frames.c).  With the cadence of Pulldown23RemovalFilter.c:56-60 -- AA BB BC CD DD, first
 * letter the even rows, second the odd rows -- and offset 0, output frame 5k + r takes its even rows from source frame 4k + e[r]
 * and its odd rows from 4k + o[r]; `offset` starts the cadence that many output frames in, counted from the source frame that
 * output frame then shows (shift[offset]).  Floor division: negative frame indices continue the cadence backwards. */
CVS_EXPORT int cvs_pulldown23_add_frames(int offset, int frame_index, int *even_source, int *odd_source) {
    static const int e[5] = { 0, 1, 1, 2, 3 }, o[5] = { 0, 1, 2, 3, 3 }, shift[5] = { 0, 1, 2, 3, 3 };
    if (offset < 0 || offset > 4) { cvs_set_error("cvs_pulldown23_add_frames: offset %d outside 0..4", offset); return -1; }
    const long long i = (long long)frame_index + offset;
    long long k = i / 5, r = i % 5;
    if (r < 0) { r += 5; k -= 1; }
    *even_source = (int)(4 * k + e[r] - shift[offset]);
    *odd_source = (int)(4 * k + o[r] - shift[offset]);
    return *even_source != *odd_source;
}
