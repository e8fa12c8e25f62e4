/*
 * temporal.c -- cvs_temporal_denoise_f16_dev: a frame averaged with the two or four frames around it in time where nothing moved,
 * left alone where something did.
 *
 * No reference code: the reference has no temporal filter and names none.  The contract is DESIGN.md "Temporal denoise" and the
 * comment of include/canvas_temporal.h; refusals, window arithmetic and which neighbours reach the kernel stay here, pixels go to
 * kernels/temporal_ops.hip -- or, with no neighbour left, to the frame copy, which by the contract gives the same bits.  One build
 * of the kernels (every operation rounded on its own), so no CVK() here.  No allocation and no synchronisation: the call records
 * into a graph.
 */
#include "internal.h"
#include "canvas_temporal.h"

static const char what[] = "cvs_temporal_denoise_f16_dev";

static bool present(const rgba_frame_f16 *f) { return f && !box2i_is_empty(&f->current_window); }

CVS_EXPORT int cvs_temporal_denoise_f16_dev(rgba_frame_f16 *out,
        const rgba_frame_f16 *prev2, const rgba_frame_f16 *prev1, const rgba_frame_f16 *cur,
        const rgba_frame_f16 *next1, const rgba_frame_f16 *next2,
        const cvs_temporal_denoise *p, cvs_stream_t s) {
    /* cur, then the neighbours in the contract's order of summation */
    const rgba_frame_f16 *in[5] = { cur, prev1, next1, prev2, next2 };
    /* Asked before the output's window is emptied: handed in as ONE struct, the output is that input, window and all, and a
     * neighbour would then pass for absent (canvas_hip.h "Operands that share a buffer"). */
    bool shares = false;
    for (int i = 0; out && i < 5; i++) shares = shares || (in[i] && (i == 0 || present(in[i])) && out->data == in[i]->data);
    if (out) box2i_set_empty(&out->current_window);
    if (!out || !cur || !p) { cvs_set_error("%s: need the frames and the parameters", what); return -1; }
    if (p->channels == 0 || (p->channels & ~CVS_MEDIAN_ALL) != 0) { cvs_set_error("%s: channels 0x%x is not a mask of CVS_MEDIAN_R, _G, _B, _A with a channel in it", what, (unsigned)p->channels); return -1; }
    if (p->flags != 0) { cvs_set_error("%s: unknown flags 0x%x", what, (unsigned)p->flags); return -1; }
    if (!isfinite(p->threshold)) { cvs_set_error("%s: threshold %g must be finite", what, p->threshold); return -1; }
    if (!isfinite(p->softness) || p->softness < 0.0f) { cvs_set_error("%s: softness %g must be finite and not negative", what, p->softness); return -1; }
    if (shares) { cvs_set_error("%s: the output cannot be one of the inputs", what); return -1; }
    for (int i = 0; i < 5; i++) {
        if (!in[i]) continue;
        if (!cvs_box_contains(&in[i]->full_window, &in[i]->current_window)) { cvs_set_error("%s: an input's current_window lies outside its buffer", what); return -1; }
    }
    if (cvs_coords_refused(what, "out", &out->full_window, NULL, CVS_MAX_COORD)) return -1;
    for (int i = 0; i < 5; i++)
        if (in[i] && cvs_coords_refused(what, "an input", &in[i]->full_window, &in[i]->current_window, CVS_MAX_COORD)) return -1;
    if (cvs_enter() != 0) return -1;

    box2i w;
    box2i_intersect(&w, &out->full_window, &cur->current_window);
    if (box2i_is_empty(&cur->current_window) || box2i_is_empty(&w)) return 0;

    /* the neighbours that have a sample within one pixel of the window written: the others change nothing, and neither does a
     * far frame whose near frame is left out (its weight is capped by 0) */
    cvk_temporal_params tp;
    memset(&tp, 0, sizeof tp);
    box2i reach = { { w.min.x - 1, w.min.y - 1 }, { w.max.x + 1, w.max.y + 1 } };           /* (inside int: CVS_MAX_COORD) */
    int count = 0, slot[5] = { -1, -1, -1, -1, -1 };          /* slot[i]: where in[i] went in tp.n */
    for (int i = 1; i < 5; i++) {
        if (!present(in[i])) continue;
        if (i >= 3 && slot[i - 2] < 0) continue;
        box2i v, near;
        box2i_intersect(&v, &cur->current_window, &in[i]->current_window);
        box2i_intersect(&near, &v, &reach);
        if (box2i_is_empty(&v) || box2i_is_empty(&near)) continue;
        tp.n[count] = cvs_view(in[i]->data, &in[i]->full_window);
        tp.v[count] = cvs_rect(&v);
        tp.near[count] = i >= 3 ? slot[i - 2] : -1;
        slot[i] = count++;
    }

    int rc;
    if (count == 0) {
        rc = cvk_copy_f16(cvs_view(out->data, &out->full_window), cvs_view(cur->data, &cur->full_window), cvs_rect(&w), cvs_pick_stream(s));
    } else {
        tp.out = cvs_view(out->data, &out->full_window);
        tp.cur = cvs_view(cur->data, &cur->full_window);
        tp.w = cvs_rect(&w);
        tp.cw = cvs_rect(&cur->current_window);
        tp.channels = p->channels;
        tp.threshold = p->threshold;
        tp.soft = p->softness > 0.0f;
        if (tp.soft) tp.inv_soft = 1.0f / p->softness;
        rc = cvk_temporal_denoise(&tp, count, cvs_cus(), cvs_pick_stream(s));
    }
    if (rc != 0) { cvs_set_error("%s: %s", what, hipGetErrorString((hipError_t)rc)); return rc; }
    out->current_window = w;
    return 0;
}
