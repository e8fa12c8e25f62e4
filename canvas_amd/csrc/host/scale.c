/*
 * scale.c -- separable resampling and blur: which kernel takes a call, on the host; pixels in kernels/fir_ops.hip and the sweeps.
 *
 * video_scale_bilinear_f32 / _pull follow src/cprocess/video_scale.c:231-319 decision for
 * decision: the identity shortcuts, smaller factor first (:252), the intermediate frame's window
 * (:256-262, :271-277 -- derived with `* factor`, so a two-axis downscale only covers part of the
 * target; kept, it is what the reference outputs), the zero fill, the window of lines actually
 * touched (:124, :191, :225), the pull rectangle (:303-309).
 *
 * Per pass the reference regenerates a triangle filter per line with the fractional offset of
 * that line's centre (:67-71, :97-101).  fir_tables.c runs the same generator on the host and
 * records, per target line, which source lines feed it and with what weight, in ascending source
 * order; that table (a few KiB) is kept on the device and the gather kernel does the rest.
 *
 * The FIR blur and the Lanczos resampler have no counterpart to follow (the reference has no blur,
 * and filter_createLanczos has no caller): they are defined in DESIGN.md and reuse the same kernel.
 */
#define _GNU_SOURCE
#include "internal.h"
#include <limits.h>
#include <math.h>
#include <stdatomic.h>

static _Atomic int g_fir_path = CVS_FIR_PATH_AUTO;

static _Thread_local int t_scale_fused;         /* the calling thread's last scaler call ran both passes in one launch */
CVS_EXPORT int cvs_scale_last_was_fused(void) { return t_scale_fused; }
static _Thread_local int t_fir_kernel;          /* CVS_FIR_KERNEL_*: the kernel the calling thread's last FIR launch went to */
CVS_EXPORT int cvs_fir_last_kernel(void) { return t_fir_kernel; }
/* A fused kernel that was chosen for a table pair and then did not launch: the next kernel in line still computes the
 * same pixels, 3-7x slower -- that must not go unnoticed. */
/* (Goes to the log handler only: the call then succeeds on the next kernel, and a successful call leaves no message in
 * cvs_last_error(); cvs_fir_last_kernel() and cvs_fir_fell_through_count() are the programmatic signals.) */
static _Thread_local int t_fell_through;        /* launches of the calling thread that went to the next kernel in line */
CVS_EXPORT int cvs_fir_fell_through_count(void) { return t_fell_through; }
static void fir_launch_fell_through(const char *kernel, int rc) {
    (void)hipGetLastError();
    t_fell_through++;
    cvs_log_warning("%s did not launch (%s): falling back to the next FIR kernel", kernel, hipGetErrorString((hipError_t)rc));
}
CVS_EXPORT void cvs_fir_path_override(int mode) { atomic_store(&g_fir_path, mode & (CVS_FIR_PATH_PASSES | CVS_FIR_PATH_TILED | CVS_FIR_PATH_TABLES | CVS_FIR_PATH_HV | CVS_FIR_PATH_ONE_COLUMN | CVS_FIR_PATH_TWO_COLUMNS | CVS_FIR_PATH_STRIPS | CVS_FIR_PATH_TILES)); }

/* ---------------------------------------------------------------- frames
 * a frame of either pixel format, as the passes and the FIR launches see it (a source's `cur`: the window they read) */
typedef struct { void *data; box2i full, cur; int half; } any_frame;

static size_t any_bytes(const any_frame *f) { return cvs_box_pixels(&f->full) * (f->half ? sizeof(rgba_f16) : sizeof(rgba_f32)); }

/* An entry point's frame of either format: `f` is an rgba_frame_f16 * when `half`, else an rgba_frame_f32 * (the two
 * structs differ in nothing but the pixel type).  All NULL for a null frame. */
typedef struct { void *frame, *data; box2i *full, *cur; } frame_ref;

static frame_ref frame_of(const void *f, int half) {
    frame_ref r = { (void *)f, NULL, NULL, NULL };
    if (f && half) { rgba_frame_f16 *h = r.frame; r.data = h->data; r.full = &h->full_window; r.cur = &h->current_window; }
    else if (f)    { rgba_frame_f32 *g = r.frame; r.data = g->data; r.full = &g->full_window; r.cur = &g->current_window; }
    return r;
}

/* frame i of a batch entry's array of them (rgba_frame_f16 *const * when `half`, else rgba_frame_f32 *const *) */
static frame_ref frame_at(const void *frames, int i, int half) {
    return frame_of(half ? (const void *)((const rgba_frame_f16 *const *)frames)[i] : (const void *)((const rgba_frame_f32 *const *)frames)[i], half);
}

/* the frame with its windows as they stand now */
static any_frame any_of(const frame_ref *f, int half) {
    const any_frame a = { f->data, *f->full, *f->cur, half };
    return a;
}

/* What a single-frame entry checks first, with its frames as frame_of() reads them into *t, *src: a device for the call,
 * and a source window inside its own buffer (else a kernel would read past it).  On refusal the target's window is
 * emptied; `what` names the entry point.  `lim`: the coordinate bound of the entry's family (CVS_MAX_COORD; the resamplers,
 * which form positions in float: CVS_RESAMPLE_MAX_COORD).
 * First of all, before any device call: a target that is the source's buffer.  Every kernel behind these entries gathers
 * source pixels that another lane, or another workgroup, writes as target pixels (canvas_hip.h "Operands that share a
 * buffer"): none of them runs in place, whichever takes the call. */
static bool shares_buffer(const frame_ref *t, const frame_ref *src, const char *what) {
    if (!t->data || t->data != src->data) return false;
    cvs_set_error("%s: the target is the source's buffer: the operation is not in place", what);
    return true;
}

static bool entry_refused(void *target, const void *source, int half, const char *what, frame_ref *t, frame_ref *src, int lim) {
    *t = frame_of(target, half);
    *src = frame_of(source, half);
    if (shares_buffer(t, src, what)) { box2i_set_empty(t->cur); return true; }
    if (cvs_enter() != 0) { box2i_set_empty(t->cur); return true; }
    if (!cvs_box_contains(src->full, src->cur)) {
        cvs_set_error("%s: the input's current_window lies outside its buffer", what);
        box2i_set_empty(t->cur);
        return true;
    }
    if (cvs_coords_refused(what, "source", src->full, src->cur, lim) || cvs_coords_refused(what, "target", t->full, NULL, lim)) {
        box2i_set_empty(t->cur);
        return true;
    }
    return false;
}

static void batch_empty_from(const void *targets, int from, int count, int half) {
    for (int i = from; i < count; i++) box2i_set_empty(frame_at(targets, i, half).cur);
}

/* What `count` single calls would refuse, a batch entry refuses before anything is launched: null arrays or frames; a
 * source window outside its buffer (it would send a kernel's rows out of bounds) or no device, with every target's window
 * emptied; a frame whose target is its own source's buffer, likewise, and first. */
static bool batch_refused(const void *targets, const void *sources, int count, int half, const char *what, int lim) {
    if (!targets || !sources) { cvs_set_error("%s: bad arguments", what); return true; }
    for (int i = 0; i < count; i++)
        if (!frame_at(targets, i, half).frame || !frame_at(sources, i, half).frame) {
            cvs_set_error("%s: frame %d of %d is a null pointer", what, i, count);
            return true;
        }
    for (int i = 0; i < count; i++) {
        const frame_ref t = frame_at(targets, i, half), src = frame_at(sources, i, half);
        if (shares_buffer(&t, &src, what)) { batch_empty_from(targets, 0, count, half); return true; }
    }
    for (int i = 0; i < count; i++) {
        const frame_ref src = frame_at(sources, i, half);
        if (!cvs_box_contains(src.full, src.cur)) {
            cvs_set_error("%s: the input's current_window lies outside its buffer (frame %d)", what, i);
            batch_empty_from(targets, 0, count, half);
            return true;
        }
        if (cvs_coords_refused(what, "a source", src.full, src.cur, lim) || cvs_coords_refused(what, "a target", frame_at(targets, i, half).full, NULL, lim)) {
            batch_empty_from(targets, 0, count, half);
            return true;
        }
    }
    if (cvs_enter() != 0) { batch_empty_from(targets, 0, count, half); return true; }
    return false;
}

/* ---- batches of frames of one geometry (kernels.h cvk_frame_batch) ---- */
static bool same_box(const box2i *a, const box2i *b) { return memcmp(a, b, sizeof *a) == 0; }

/* Frames first .. first + n - 1 (n <= CVK_FRAME_BATCH) of a batch entry's arrays as the batch *b of one launch, with
 * noverlays (<= CVK_BLUR_MAX_OVER) layers each, frame-major.  False when that cannot be one launch: fewer than two frames,
 * or an output that overlaps an input of the run (another frame's, or its own at a shifted address) or another output. */
static bool batch_group(cvk_frame_batch *b, const void *targets, const void *sources, int half, int first, int n, size_t tbytes, size_t sbytes,
                        const rgba_frame_f16 *const *overlays, int noverlays) {
    const void *in[CVK_FRAME_BATCH * (1 + CVK_BLUR_MAX_OVER)];
    int nin = 0;
    memset(b, 0, sizeof *b);
    b->n = n;
    for (int i = 0; i < n; i++) {
        b->target[i] = frame_at(targets, first + i, half).data;
        in[nin++] = b->source[i] = frame_at(sources, first + i, half).data;
        for (int l = 0; l < noverlays; l++) in[nin++] = b->over[i][l] = overlays[(size_t)(first + i) * noverlays + l]->data;
    }
    if (n < 2) return false;
    for (int i = 0; i < n; i++) {
        const char *o = b->target[i];
        for (int j = 0; j < nin; j++) { const char *q = in[j]; if (q && o < q + sbytes && q < o + tbytes) return false; }
        for (int j = 0; j < i; j++) { const char *q = b->target[j]; if (o < q + tbytes && q < o + tbytes) return false; }
    }
    return true;
}

/* one launch of k_fir (kernels/fir_ops.hip: one lane per target pixel, taps gathered through L1/L2): target lines t0 .. t1
 * along `axis` from the table `tab`, whose first line is t0, and lines lo .. hi of the other axis */
static int gather_pass(const any_frame *t, const any_frame *src, const cvk_fir_axis *tab, int axis, int t0, int t1, int lo, int hi, hipStream_t s) {
    if (t1 < t0 || hi < lo) return 0;
    cvk_fir_params fp;
    memset(&fp, 0, sizeof fp);
    fp.target = cvs_view(t->data, &t->full);
    fp.source = cvs_view(src->data, &src->full);
    fp.axis = axis;
    fp.t0 = t0; fp.t1 = t1; fp.lo = lo; fp.hi = hi;
    fp.ntaps = tab->ntaps; fp.tap_src = tab->src; fp.taps = tab->taps; fp.stride = tab->stride;
    fp.in_half = src->half; fp.out_half = t->half;
    return CVK(cvk_fir_gather)(&fp, s);
}

/* the fused kernels' parameters for the target rectangle tx0 .. tx1 x ty0 .. ty1 from the table pair h, v (max_sh: the
 * tiles' own) */
static cvk_fir2d_params fir2d_params(const any_frame *t, const any_frame *src, int tx0, int ty0, int tx1, int ty1,
                                     const cvs_fir_table *h, const cvs_fir_table *v) {
    cvk_fir2d_params fp;
    memset(&fp, 0, sizeof fp);
    fp.target = cvs_view(t->data, &t->full);
    fp.source = cvs_view(src->data, &src->full);
    fp.in_half = src->half; fp.out_half = t->half;
    fp.tx0 = tx0; fp.ty0 = ty0; fp.tx1 = tx1; fp.ty1 = ty1;
    fp.h = h->axis; fp.v = v->axis;
    fp.max_sw = h->max_foot > 0 ? h->max_foot : 1;
    return fp;
}

/* ---------------------------------------------------------------- the triangle scaler */

/* one pass of video_scale.c:34-127 (axis 0) or :129-229 (axis 1) on device frames */
static int triangle_pass(any_frame *target, float tmin, const any_frame *source, float smin, float factor, int axis, hipStream_t s) {
    const box2i srect = source->cur, trect = target->full;
    const int lo = axis ? (srect.min.y > trect.min.y ? srect.min.y : trect.min.y) : (srect.min.x > trect.min.x ? srect.min.x : trect.min.x);
    const int hi = axis ? (srect.max.y < trect.max.y ? srect.max.y : trect.max.y) : (srect.max.x < trect.max.x ? srect.max.x : trect.max.x);
    const int s0 = axis ? srect.min.x : srect.min.y, s1 = axis ? srect.max.x : srect.max.y;
    const int t0 = axis ? trect.min.x : trect.min.y, t1 = axis ? trect.max.x : trect.max.y;

    /* the per-line taps depend only on the geometry, which repeats from frame to frame: planned once, kept on the
     * device; steady state is one gather launch (and the zero fill, when the pass leaves part of the target alone),
     * nothing synchronous */
    cvs_fir_table table;
    int rc = cvs_fir_table_triangle(tmin, smin, factor, s0, s1, t0, t1, axis == 0 || lo <= hi, &table);
    if (rc != 0) return rc;
    const int used_lo = table.used_lo, used_hi = table.used_hi;
    /* video_scale.c:25-32,44: the target starts as zeros (all-zero bytes are 0.0 in either format).  The gather writes every
     * pixel of lines used_lo..used_hi x lo..hi (a line without taps gets its zeros there): when that is the whole buffer --
     * the usual case -- the fill would only be overwritten (an enlarging 4K pass: 500 MB of the 1.3 GB it moved). */
    {
        const int o0 = axis ? trect.min.y : trect.min.x, o1 = axis ? trect.max.y : trect.max.x;
        const bool covers = used_hi >= used_lo && hi >= lo && used_lo == t0 && used_hi == t1 && lo == o0 && hi == o1;
        if (!covers && any_bytes(target)) {
            hipError_t e_ = hipMemsetAsync(target->data, 0, any_bytes(target), s);
            if (e_ != hipSuccess) { cvs_fir_table_release(&table, s); cvs_set_error("zero fill: %s", hipGetErrorString(e_)); return -1; }
        }
    }
    if (used_hi >= used_lo && hi >= lo) {
        /* the gather reads source lines named in the table; they lie inside the source window by construction */
        const size_t first = (size_t)(used_lo - t0);
        cvk_fir_axis from = table.axis;
        from.ntaps += first; from.src += first * (size_t)from.stride; from.taps += first * (size_t)from.stride;
        rc = gather_pass(target, source, &from, axis, used_lo, used_hi, lo, hi, s);
        if (rc == 0) t_fir_kernel = CVS_FIR_KERNEL_PASS;
    }
    cvs_fir_table_release(&table, s);
    if (rc != 0) { cvs_set_error("FIR gather launch failed: %s", hipGetErrorString((hipError_t)rc)); return rc; }
    if (axis) box2i_set(&target->cur, used_lo, lo, used_hi, hi);
    else      box2i_set(&target->cur, lo, used_lo, hi, used_hi);
    return 0;
}

/* Both passes of video_scale_bilinear_f32 in one launch when the vertical pass comes first (equal factors, or the vertical
 * one smaller: video_scale.c:252) -- sweep_vh_ops.hip.  Same tables, same windows as the two triangle_pass calls below
 * would use: the frame between the passes (`mid_full`, video_scale.c:254-272) never exists, only its geometry does.
 * `batch` (cvs_scale_bilinear_*_batch_dev): the frames that go into the launch along with `target` and `source`; only the
 * tile kernel takes one.  0 = done, 1 = not for this kernel (the caller runs the two passes), 2 = not for this kernel as a
 * batch, < 0 = error. */
static int triangle_fused_vh(any_frame *target, v2f tp, const any_frame *source, v2f sp, v2f fac, const box2i *mid_full,
                             const cvk_frame_batch *batch, hipStream_t s) {
    const box2i *tf = &target->full, *sc = &source->cur;
    /* pass 1 (vertical) into the frame between the passes */
    const int lo1 = sc->min.x > mid_full->min.x ? sc->min.x : mid_full->min.x, hi1 = sc->max.x < mid_full->max.x ? sc->max.x : mid_full->max.x;
    cvs_fir_table tv, th = { .pin = -1 };
    if (hi1 < lo1) return 1;
    if (cvs_fir_table_triangle(tp.y, sp.y, fac.y, sc->min.y, sc->max.y, mid_full->min.y, mid_full->max.y, true, &tv) != 0) return -1;
    const int vlo = tv.used_lo, vhi = tv.used_hi;
    int rc = 1;
    if (vhi >= vlo) {
        /* pass 2 (horizontal) from that frame's window (lo1..hi1 x vlo..vhi) into the target */
        const int lo2 = vlo > tf->min.y ? vlo : tf->min.y, hi2 = vhi < tf->max.y ? vhi : tf->max.y;
        if (hi2 >= lo2 && cvs_fir_table_triangle(tp.x, sp.x, fac.x, lo1, hi1, tf->min.x, tf->max.x, true, &th) == 0) {
            const int hlo = th.used_lo, hhi = th.used_hi;
            /* every column (those without taps are zeros, as the fill leaves them); the vertical table's lines, lo2 .. hi2 of
             * them produced */
            cvk_fir2d_params fp = fir2d_params(target, source, tf->min.x, mid_full->min.y, tf->max.x, hi2, &th, &tv);
            /* short lists over few source pixels (enlarging): a workgroup per tile where that is the faster form (pinned:
             * wherever it takes the call); else a wave per strip */
            const int pinned = atomic_load(&g_fir_path);
            /* (a batch is one large target to the kernels: halfs go to the strips, as 4K -> 8K does -- profiles/r04/scaler_batch.txt) */
            const bool tiles = hhi >= hlo && !(pinned & CVS_FIR_PATH_STRIPS) &&
                               ((pinned & CVS_FIR_PATH_TILES) ? CVK(cvk_fir_tvh_supported)(&fp)
                                : batch && target->half ? false : CVK(cvk_fir_tvh_preferred)(&fp));
            /* the kernels' predicates (and the instance k_fir_vh picks) look at the target's base address -- a pair of halfs is
             * ONE 16-byte store -- and fp.target is frame 0: every frame of the launch must answer as frame 0 does, which with
             * one geometry means the same address modulo 16.  Else the frames run one by one. */
            bool alike = true;
            for (int i = 0; batch && i < batch->n; i++) alike = alike && !((((uintptr_t)batch->target[i]) ^ (uintptr_t)target->data) & 15u);
            if (batch && !(alike && hhi >= hlo && (tiles || CVK(cvk_fir_vh_supported)(&fp)))) rc = 2;
            else if (hhi >= hlo && (tiles || CVK(cvk_fir_vh_supported)(&fp))) {
                /* video_scale.c:25-32,44: rows the pass leaves alone are zeros */
                const bool covers = lo2 == tf->min.y && hi2 == tf->max.y;
                hipError_t e = hipSuccess;
                if (batch) {
                    fp.nframes = batch->n;
                    for (int i = 0; i < batch->n; i++) {
                        fp.frame_source[i] = batch->source[i]; fp.frame_target[i] = batch->target[i];
                        if (!covers && any_bytes(target) && e == hipSuccess) e = hipMemsetAsync(batch->target[i], 0, any_bytes(target), s);
                    }
                } else if (!covers && any_bytes(target)) e = hipMemsetAsync(target->data, 0, any_bytes(target), s);
                int krc = e != hipSuccess ? (int)e : tiles ? CVK(cvk_fir_tvh)(&fp, lo2 - fp.ty0, s) : CVK(cvk_fir_vh)(&fp, lo2 - fp.ty0, cvs_cus(), s);
                if (krc == 0) { box2i_set(&target->cur, hlo, lo2, hhi, hi2); t_fir_kernel = tiles ? CVS_FIR_KERNEL_TILE_VH : CVS_FIR_KERNEL_VH; rc = 0; }
                else { fir_launch_fell_through(tiles ? "k_fir_tile_vh" : "k_fir_vh", krc); rc = 1; }   /* did not launch: the two passes decide */
            }
        }
    }
    cvs_fir_table_release(&tv, s); cvs_fir_table_release(&th, s);
    return rc;
}

/* The other order (horizontal factor strictly smaller: the horizontal pass first) is the order of sweep_hv_ops.hip's kernel.
 * 0 = done, 1 = not for this kernel, < 0 = error. */
static int triangle_fused_hv(any_frame *target, v2f tp, const any_frame *source, v2f sp, v2f fac, const box2i *mid_full, hipStream_t s) {
    const box2i *tf = &target->full, *sc = &source->cur;
    /* pass 1 (horizontal) into the frame between the passes: rows lo1..hi1 */
    const int lo1 = sc->min.y > mid_full->min.y ? sc->min.y : mid_full->min.y, hi1 = sc->max.y < mid_full->max.y ? sc->max.y : mid_full->max.y;
    cvs_fir_table th, tv = { .pin = -1 };
    if (hi1 < lo1) return 1;
    if (cvs_arith() != CVS_ARITH_SEPARATE) return 1;           /* the horizontal-first sweep exists in the plain flavour only: the two passes */
    if (cvs_fir_table_triangle(tp.x, sp.x, fac.x, sc->min.x, sc->max.x, mid_full->min.x, mid_full->max.x, true, &th) != 0) return -1;
    const int hlo = th.used_lo, hhi = th.used_hi;
    int rc = 1;
    if (hhi >= hlo) {
        /* pass 2 (vertical) from that frame's window (hlo..hhi x lo1..hi1) into the target: columns lo2..hi2 */
        const int lo2 = hlo > tf->min.x ? hlo : tf->min.x, hi2 = hhi < tf->max.x ? hhi : tf->max.x;
        if (hi2 >= lo2 && cvs_fir_table_triangle(tp.y, sp.y, fac.y, lo1, hi1, tf->min.y, tf->max.y, true, &tv) == 0) {
            const int vlo = tv.used_lo, vhi = tv.used_hi;
            /* from the horizontal table's first column (those without taps are zeros); every line (those without taps are
             * written as zeros) */
            cvk_fir2d_params fp = fir2d_params(target, source, mid_full->min.x, tf->min.y, hi2, tf->max.y, &th, &tv);
            if (vhi >= vlo && cvk_fir_hv_supported(&fp)) {
                const bool covers = fp.tx0 == tf->min.x && hi2 == tf->max.x;
                hipError_t e = covers || !any_bytes(target) ? hipSuccess : hipMemsetAsync(target->data, 0, any_bytes(target), s);
                int krc = e != hipSuccess ? (int)e : cvk_fir_hv(&fp, cvs_cus(), s);
                if (krc == 0) { box2i_set(&target->cur, lo2, vlo, hi2, vhi); t_fir_kernel = CVS_FIR_KERNEL_HV; rc = 0; }
                else { fir_launch_fell_through("k_fir_hv", krc); rc = 1; }
            }
        }
    }
    cvs_fir_table_release(&tv, s); cvs_fir_table_release(&th, s);
    return rc;
}

/* video_scale_bilinear_f32 (video_scale.c:231-286) between frames of either format: f16 sources are widened as they
 * are read, f16 targets truncated as they are written (what the pulls around an f32 scaler node do, main.c:43-71,
 * 105-144); the frame between the two passes is always f32.  The caller has dealt with the all-identity case.
 * `batch`: NULL for a single call; a batch goes through the vertical-first fused launch or not at all (2: the caller does
 * its frames one by one). */
static int scale_core(any_frame *target, v2f tp, const any_frame *source, v2f sp, v2f fac, const cvk_frame_batch *batch, hipStream_t s) {
    t_scale_fused = 0;
    t_fir_kernel = CVS_FIR_KERNEL_NONE;
    if (batch && ((fac.x == 1.0f && tp.x == sp.x) || (fac.y == 1.0f && tp.y == sp.y) || fac.x < fac.y ||
                  (atomic_load(&g_fir_path) & (CVS_FIR_PATH_PASSES | CVS_FIR_PATH_TILED)))) return 2;
    if (fac.x == 1.0f && tp.x == sp.x) return triangle_pass(target, tp.y, source, sp.y, fac.y, 0, s);
    if (fac.y == 1.0f && tp.y == sp.y) return triangle_pass(target, tp.x, source, sp.x, fac.x, 1, s);

    any_frame mid;
    memset(&mid, 0, sizeof mid);
    const box2i *tf = &target->full, *sc = &source->cur;
    const bool x_first = fac.x < fac.y;
    const int fl = cvs_arith() == CVS_ARITH_CONTRACTED;       /* video_scale.c:257-277: sp - d * fac and sp + d * fac, one expression each */
    if (x_first)
        box2i_set(&mid.full, (int)madd_as(fl, -(tp.x - tf->min.x), fac.x, sp.x), sc->min.y,
                  (int)madd_as(fl, tf->max.x - tp.x, fac.x, sp.x), sc->max.y);
    else
        box2i_set(&mid.full, sc->min.x, (int)madd_as(fl, -(tp.y - tf->min.y), fac.y, sp.y),
                  sc->max.x, (int)madd_as(fl, tf->max.y - tp.y, fac.y, sp.y));
    box2i_intersect(&mid.full, &mid.full, tf);
    mid.cur = mid.full;
    if (!(atomic_load(&g_fir_path) & (CVS_FIR_PATH_PASSES | CVS_FIR_PATH_TILED))) {
        int rc = x_first ? triangle_fused_hv(target, tp, source, sp, fac, &mid.full, s) : triangle_fused_vh(target, tp, source, sp, fac, &mid.full, batch, s);
        if (rc == 0) t_scale_fused = 1;
        if (rc <= 0) return rc;                              /* done, or failed; 1: not for the fused kernel */
        if (batch) return 2;
    }
    size_t n = cvs_box_pixels(&mid.full);
    mid.data = cvs_pool_malloc(sizeof(rgba_f32) * (n ? n : 1), s);
    if (!mid.data) return -1;
    int rc;
    if (x_first) { rc = triangle_pass(&mid, tp.x, source, sp.x, fac.x, 1, s); if (rc == 0) rc = triangle_pass(target, tp.y, &mid, sp.y, fac.y, 0, s); }
    else         { rc = triangle_pass(&mid, tp.y, source, sp.y, fac.y, 0, s); if (rc == 0) rc = triangle_pass(target, tp.x, &mid, sp.x, fac.x, 1, s); }
    cvs_pool_free(mid.data, s);
    return rc;
}

/* cvs_scale_bilinear_f32_dev / _f16_dev.  Between two f16 frames: the f16 pull of a scaler node whose input is a
 * half-native source, without the widened copy of the input and the f32 copy of the output ever existing. */
static int scale_frame(void *target, v2f tp, const void *source, v2f sp, v2f fac, int half, cvs_stream_t stream, const char *what) {
    frame_ref t, src;
    if (entry_refused(target, source, half, what, &t, &src, CVS_RESAMPLE_MAX_COORD)) return -1;
    if (cvs_point_refused(what, "the target point", tp, CVS_RESAMPLE_MAX_COORD) || cvs_point_refused(what, "the source point", sp, CVS_RESAMPLE_MAX_COORD)) {
        box2i_set_empty(t.cur);
        return -1;
    }
    hipStream_t s = cvs_pick_stream(stream);
    if (fac.x == 1.0f && tp.x == sp.x && fac.y == 1.0f && tp.y == sp.y)
        return half ? cvs_copy_frame_f16_dev(target, source, s) : cvs_copy_frame_alpha_f32_dev(target, source, 1.0f, s);
    any_frame tf = any_of(&t, half);
    const any_frame sf = any_of(&src, half);
    int rc = scale_core(&tf, tp, &sf, sp, fac, NULL, s);
    *t.cur = tf.cur;
    if (rc != 0) box2i_set_empty(t.cur);
    return rc;
}

CVS_EXPORT int cvs_scale_bilinear_f32_dev(rgba_frame_f32 *target, v2f tp, const rgba_frame_f32 *source, v2f sp, v2f fac, cvs_stream_t stream) {
    return scale_frame(target, tp, source, sp, fac, 0, stream, "cvs_scale_bilinear_f32_dev");
}

CVS_EXPORT int cvs_scale_bilinear_f16_dev(rgba_frame_f16 *target, v2f tp, const rgba_frame_f16 *source, v2f sp, v2f fac, cvs_stream_t stream) {
    return scale_frame(target, tp, source, sp, fac, 1, stream, "cvs_scale_bilinear_f16_dev");
}

/* cvs_scale_bilinear_f16_dev / _f32_dev for `count` INDEPENDENT frames (a pull queue's frames in flight): frames of one geometry
 * that do not overlap go up to eight at a time into ONE launch of the tile kernel (grid.z = frame), where that kernel takes
 * the call (vertical pass first, short tap lists: enlarging); every other combination is carried out frame by frame, exactly
 * as `count` single calls.  Results are those of the single calls, bit for bit.  Geometry is compared within runs of 64
 * frames; the first group that cannot go into one launch sends it and every later frame down the single calls. */
static int scale_batch_frames(const void *targets, v2f tp, const void *sources, v2f sp, v2f fac, int count, int half,
                              cvs_stream_t stream, const char *what) {
    if (count <= 0) return 0;
    if (batch_refused(targets, sources, count, half, what, CVS_RESAMPLE_MAX_COORD)) return -1;
    if (cvs_point_refused(what, "the target point", tp, CVS_RESAMPLE_MAX_COORD) || cvs_point_refused(what, "the source point", sp, CVS_RESAMPLE_MAX_COORD)) {
        batch_empty_from(targets, 0, count, half);
        return -1;
    }
    hipStream_t s = cvs_pick_stream(stream);
    const size_t px = half ? sizeof(rgba_f16) : sizeof(rgba_f32);
    int rc = 0, done = 0;
    for (int base = 0; count > 1 && rc == 0 && done == base && base < count; base += 64) {
        const int end = count - base < 64 ? count : base + 64;
        const frame_ref t0 = frame_at(targets, base, half), s0 = frame_at(sources, base, half);
        bool uniform = end - base > 1 && !box2i_is_empty(s0.cur) && !box2i_is_empty(t0.full) &&
                       !(fac.x == 1.0f && tp.x == sp.x && fac.y == 1.0f && tp.y == sp.y);
        for (int i = base + 1; uniform && i < end; i++) {
            const frame_ref ti = frame_at(targets, i, half), si = frame_at(sources, i, half);
            uniform = same_box(ti.full, t0.full) && same_box(si.full, s0.full) && same_box(si.cur, s0.cur);
        }
        const size_t tbytes = cvs_box_pixels(t0.full) * px, sbytes = cvs_box_pixels(s0.full) * px;
        while (uniform && rc == 0 && done < end) {
            const int n = end - done < CVK_FRAME_BATCH ? end - done : CVK_FRAME_BATCH;
            cvk_frame_batch b;
            if (!batch_group(&b, targets, sources, half, done, n, tbytes, sbytes, NULL, 0)) break;      /* the rest frame by frame */
            const frame_ref td = frame_at(targets, done, half), sd = frame_at(sources, done, half);
            any_frame t = any_of(&td, half);
            const any_frame src = any_of(&sd, half);
            rc = scale_core(&t, tp, &src, sp, fac, &b, s);
            if (rc == 2) { rc = 0; break; }
            if (rc != 0) break;
            for (int i = 0; i < n; i++) *frame_at(targets, done + i, half).cur = t.cur;
            done += n;
        }
    }
    for (; rc == 0 && done < count; done++) {
        void *t = frame_at(targets, done, half).frame;
        const void *src = frame_at(sources, done, half).frame;
        rc = half ? cvs_scale_bilinear_f16_dev(t, tp, src, sp, fac, stream) : cvs_scale_bilinear_f32_dev(t, tp, src, sp, fac, stream);
    }
    if (rc != 0) batch_empty_from(targets, done, count, half);
    return rc;
}

CVS_EXPORT int cvs_scale_bilinear_f16_batch_dev(rgba_frame_f16 *const *targets, v2f tp, const rgba_frame_f16 *const *sources, v2f sp, v2f fac, int count, cvs_stream_t stream) {
    return scale_batch_frames(targets, tp, sources, sp, fac, count, 1, stream, "cvs_scale_bilinear_f16_batch_dev");
}

CVS_EXPORT int cvs_scale_bilinear_f32_batch_dev(rgba_frame_f32 *const *targets, v2f tp, const rgba_frame_f32 *const *sources, v2f sp, v2f fac, int count, cvs_stream_t stream) {
    return scale_batch_frames(targets, tp, sources, sp, fac, count, 0, stream, "cvs_scale_bilinear_f32_batch_dev");
}

CVS_EXPORT void video_scale_bilinear_f32(rgba_frame_f32 *target, v2f tp, rgba_frame_f32 *source, v2f sp, v2f fac) {
    cvs_bridge br;
    rgba_frame_f32 ft, fs;
    cvs_bridge_open(&br);
    CVS_BRIDGE_FRAME(&br, ft, target, CVS_BRIDGE_UPLOAD);
    /* the scaler does not run in place: a source that is the target keeps a block of its own */
    CVS_BRIDGE_FRAME(&br, fs, source, CVS_BRIDGE_PRIVATE | (box2i_is_empty(&source->current_window) ? 0 : CVS_BRIDGE_UPLOAD));
    CVS_BRIDGE_CALL(&br, cvs_scale_bilinear_f32_dev, &ft, tp, &fs, sp, fac);
    target->current_window = ft.current_window;
    if (cvs_bridge_close(&br, target->data) != 0) box2i_set_empty(&target->current_window);
}

CVS_EXPORT void video_scale_bilinear_f32_pull(rgba_frame_f32 *target, v2f tp, video_source *source, int frame,
                                              box2i *source_rect, v2f sp, v2f fac) {
    if (fac.x == 0.0f || fac.y == 0.0f) { box2i_set_empty(&target->current_window); return; }   /* video_scale.c:290-293 */
    if (fac.x == 1.0f && fac.y == 1.0f && tp.x == sp.x && tp.y == sp.y) { video_get_frame_f32(source, frame, target); return; }
    const box2i *tf = &target->full_window;
    /* before the pull rectangle is formed: (int) of a float beyond 2^31 is undefined, and the scaler below would refuse these */
    if (cvs_coords_refused("video_scale_bilinear_f32_pull", "target", tf, NULL, CVS_RESAMPLE_MAX_COORD) ||
        cvs_point_refused("video_scale_bilinear_f32_pull", "the target point", tp, CVS_RESAMPLE_MAX_COORD) ||
        cvs_point_refused("video_scale_bilinear_f32_pull", "the source point", sp, CVS_RESAMPLE_MAX_COORD)) {
        box2i_set_empty(&target->current_window);
        return;
    }
    rgba_frame_f32 tmp;
    box2i_set(&tmp.full_window,
              (int)(sp.x - (tp.x - tf->min.x) / fac.x) - 1, (int)(sp.y - (tp.y - tf->min.y) / fac.y) - 1,
              (int)(sp.x + (tf->max.x - tp.x) / fac.x) + 1, (int)(sp.y + (tf->max.y - tp.y) / fac.y) + 1);
    box2i_intersect(&tmp.full_window, &tmp.full_window, source_rect);
    tmp.current_window = tmp.full_window;
    size_t n = cvs_box_pixels(&tmp.full_window);
    tmp.data = malloc(sizeof(rgba_f32) * (n ? n : 1));
    if (!tmp.data) { box2i_set_empty(&target->current_window); return; }
    video_get_frame_f32(source, frame, &tmp);
    video_scale_bilinear_f32(target, tp, &tmp, sp, fac);
    free(tmp.data);
}

/* ---------------------------------------------------------------- fused separable FIR (kernels/fir_ops.hip: k_fir2d)
 * The blur and the Lanczos resampler: one tap table per axis (fir_tables.c), or a register-window kernel where one tap
 * list serves every line. */

/* The same two cached tables as two launches through an f32 frame in HBM (gather_pass): what a table pair falls back to
 * when neither fused kernel takes it (footprints beyond the LDS and tap lists beyond the sweep kernel's registers: a
 * Lanczos below about 0.2x).  Slower than either, but asynchronous like them: no allocation, upload or wait on the way.
 * Same sums in the same order: x pass, then y pass, f32 between them. */
static int fir_two_launches(const any_frame *t, const any_frame *src, const box2i *rect, const cvk_fir_axis *h, const cvk_fir_axis *v, hipStream_t s) {
    const box2i *sw = &src->cur;
    any_frame mid = { NULL, *sw, *sw, 0 };
    box2i_set(&mid.full, rect->min.x, sw->min.y, rect->max.x, sw->max.y);
    mid.data = cvs_pool_malloc(cvs_box_pixels(&mid.full) * sizeof(rgba_f32), s);
    if (!mid.data) return -1;
    int rc = gather_pass(&mid, src, h, 1, rect->min.x, rect->max.x, sw->min.y, sw->max.y, s);
    if (rc == 0) rc = gather_pass(t, &mid, v, 0, rect->min.y, rect->max.y, rect->min.x, rect->max.x, s);
    cvs_pool_free(mid.data, s);
    if (rc != 0) { cvs_set_error("FIR gather launch failed: %s", hipGetErrorString((hipError_t)rc)); return -1; }
    t_fir_kernel = CVS_FIR_KERNEL_TWO_PASS;
    return 0;
}

/* 0 = launched, 1 = does not fit an LDS tile (caller falls back), <0 = error */
static int fir2d_launch(const any_frame *t, const any_frame *src, const box2i *rect, const cvs_fir_table *h, const cvs_fir_table *v, hipStream_t s) {
    cvk_fir2d_params fp = fir2d_params(t, src, rect->min.x, rect->min.y, rect->max.x, rect->max.y, h, v);
    fp.max_sh = v->max_foot > 0 ? v->max_foot : 1;
    /* First choice: the gather per target line (sweep_hv_ops.hip; plain flavour), whenever first taps never decrease down the
     * vertical table and the lists fit an instance; then the LDS tiles (both flavours) while the footprint of a 32 x 16 tile
     * fits; else 1: the caller runs the two passes through an f32 frame.  cvs_fir_path_override() pins one of the three
     * (parity tests of each, A/B runs).  (A lane-per-pixel sweep, k_fir_stream, stood between the first two until round 4: it
     * took table pairs whose tiles need more than 64 KiB once the gather had refused them -- lists longer than 24 -- and was
     * retired with that corner: those go to the tiles up to 150 KiB and to the two passes beyond.) */
    const int force = atomic_load(&g_fir_path);
    if (force & CVS_FIR_PATH_PASSES) return 1;
    const bool pinned = (force & (CVS_FIR_PATH_TILED | CVS_FIR_PATH_HV)) != 0;
    if (cvs_arith() == CVS_ARITH_SEPARATE && ((force & CVS_FIR_PATH_HV) || !pinned) && cvk_fir_hv_supported(&fp)) {
        int rc = cvk_fir_hv(&fp, cvs_cus(), s);
        if (rc == 0) { t_fir_kernel = CVS_FIR_KERNEL_HV; return 0; }
        fir_launch_fell_through("k_fir_hv", rc);              /* did not launch: the tiles decide */
    }
    if (CVK(cvk_fir2d_lds_bytes)(&fp) > 150 * 1024 || h->axis.stride > 64 || v->axis.stride > 64) return 1;
    int rc = CVK(cvk_fir2d)(&fp, s);
    if (rc != 0) { cvs_set_error("fused FIR launch failed: %s", hipGetErrorString((hipError_t)rc)); return -1; }
    t_fir_kernel = CVS_FIR_KERNEL_TILED;
    return 0;
}

/* the table pair h, v over `rect`: fir2d_launch, else the two passes; lets go of both tables */
static int fir_pair_launch(const any_frame *t, const any_frame *src, const box2i *rect, cvs_fir_table *h, cvs_fir_table *v, hipStream_t s) {
    int rc = fir2d_launch(t, src, rect, h, v, s);
    if (rc == 1) rc = fir_two_launches(t, src, rect, &h->axis, &v->axis, s);
    cvs_fir_table_release(h, s); cvs_fir_table_release(v, s);
    return rc;
}

/* cvs_fir_path_override's pins of the register-window kernels' form, as the kernels' flags */
static int blur_column_pins(void) {
    const int pin = atomic_load(&g_fir_path);
    return (pin & CVS_FIR_PATH_ONE_COLUMN ? CVK_BLUR_ONE_COLUMN : 0) | (pin & CVS_FIR_PATH_TWO_COLUMNS ? CVK_BLUR_TWO_COLUMNS : 0);
}

static bool blur_has_fast_kernel(const float *taps, int ntaps) {
    bool finite = true;
    for (int k = 0; k < ntaps; k++) finite = finite && isfinite(taps[k]);
    return finite && CVK(cvk_blur_supported)(ntaps, 1) && !(atomic_load(&g_fir_path) & CVS_FIR_PATH_TABLES);
}

/* The Lanczos resampler halving on both axes, behind the one-list blur taps[0..ntaps) (one tap of weight 1: the resampler
 * alone), as one sweep over f16 frames (blur_halve_ops.hip): every line centre t / 0.5 is an integer, so every line gets
 * the taps of offset 0 and reads source lines 2t - centre + k (plan_lanczos with frac == 0).  True, with *hp filled for
 * `t` from `src` (within its window cur), when the call has that form; whether a kernel has an instance for hp->ntaps1
 * and hp->ntaps2 is the caller's to ask. */
static bool halving_sweep(cvk_blur_halve_params *hp, float fx, float fy, int ksize, const float *taps, int ntaps, const any_frame *t, const any_frame *src) {
    if (fx != 0.5f || fy != 0.5f || (atomic_load(&g_fir_path) & CVS_FIR_PATH_TABLES)) return false;
    const box2i *tf = &t->full, *sw = &src->cur;
    fir_filter f = { NULL, 0, 0 };
    filter_createLanczos(0.5f, ksize, 0.0f, &f);
    bool usable = f.coeff && f.center == f.width / 2 && f.width <= 16 && ntaps <= 16 &&       /* (taps1, taps2 hold 16) */
                  tf->min.x > -(1 << 22) && tf->max.x < (1 << 22) && tf->min.y > -(1 << 22) && tf->max.y < (1 << 22);
    for (int k = 0; usable && k < f.width; k++) usable = isfinite(f.coeff[k]);
    for (int k = 0; usable && k < ntaps; k++) usable = isfinite(taps[k]);
    if (usable) {
        memset(hp, 0, sizeof *hp);
        hp->target = cvs_view(t->data, tf);
        hp->source = cvs_view(src->data, &src->full);
        hp->in_half = 1; hp->out_half = 1;
        hp->tx0 = tf->min.x; hp->ty0 = tf->min.y; hp->tx1 = tf->max.x; hp->ty1 = tf->max.y;
        hp->sx0 = sw->min.x; hp->sy0 = sw->min.y; hp->sx1 = sw->max.x; hp->sy1 = sw->max.y;
        hp->ntaps1 = ntaps; hp->ntaps2 = f.width;
        memcpy(hp->taps1, taps, sizeof(float) * (size_t)ntaps);
        memcpy(hp->taps2, f.coeff, sizeof(float) * (size_t)f.width);
        hp->flags = blur_column_pins();
    }
    filter_free(&f);
    return usable;
}

/* the sweep halving_sweep() planned, blur and all (the caller has asked cvk_blur_halve_supported) */
static int halving_launch(const cvk_blur_halve_params *hp, hipStream_t s) {
    int rc = CVK(cvk_blur_halve)(hp, cvs_cus(), s);
    if (rc != 0) { cvs_set_error("blur + halving launch failed: %s", hipGetErrorString((hipError_t)rc)); return -1; }
    t_fir_kernel = CVK(cvk_blur_halve_takes_pairs)(hp) ? CVS_FIR_KERNEL_HALVE_PAIR : CVS_FIR_KERNEL_HALVE;
    return 0;
}

/* The blur of `src` (within its window cur) into the rectangle `win` of `t`.  `over`: nover f16 buffers with the target's
 * layout, blended over the blur result before the store (f16 in/out only); `batch`: the frames of one launch, or NULL. */
static int blur_fused(const any_frame *t, const any_frame *src, const box2i *win, const float *taps, int ntaps,
                      const void *const *over, int nover, const cvk_frame_batch *batch, hipStream_t s) {
    const box2i *sw = &src->cur;
    /* one tap list for every line: the register-window kernel, when it has an instance for this length */
    if (blur_has_fast_kernel(taps, ntaps)) {
        cvk_blur_params bp;
        memset(&bp, 0, sizeof bp);
        bp.nover = nover;
        for (int l = 0; l < nover; l++) bp.over[l] = over[l];
        bp.target = cvs_view(t->data, &t->full);
        bp.source = cvs_view(src->data, &src->full);
        bp.in_half = src->half; bp.out_half = t->half;
        bp.tx0 = win->min.x; bp.ty0 = win->min.y; bp.tx1 = win->max.x; bp.ty1 = win->max.y;
        bp.sx0 = sw->min.x; bp.sy0 = sw->min.y; bp.sx1 = sw->max.x; bp.sy1 = sw->max.y;
        bp.ntaps = ntaps;
        memcpy(bp.taps, taps, sizeof(float) * (size_t)ntaps);
        if (batch) {
            if (!(ntaps & 1) || ntaps > 31) return 1;                 /* the batched form exists for the odd lists of blur_kernel.hpp */
            bp.batch = *batch;
        }
        bp.flags = blur_column_pins();
        int rc = CVK(cvk_blur)(&bp, cvs_cus(), s);
        if (rc != 0) { cvs_set_error("blur launch failed: %s", hipGetErrorString((hipError_t)rc)); return -1; }
        t_fir_kernel = CVK(cvk_blur_takes_pairs)(&bp) ? CVS_FIR_KERNEL_WINDOW_PAIR : CVS_FIR_KERNEL_WINDOW;
        return 0;
    }
    if (nover > 0 || batch) return 1;   /* the gather kernel has no epilogue and takes one frame: the caller goes node by node / frame by frame */
    cvs_fir_table h, v;
    if (cvs_fir_table_blur(taps, ntaps, win->min.x, win->max.x, sw->min.x, sw->max.x, CVK_FIR2D_TILE_X, &h) != 0) return -1;
    if (cvs_fir_table_blur(taps, ntaps, win->min.y, win->max.y, sw->min.y, sw->max.y, CVK_FIR2D_TILE_Y, &v) != 0) { cvs_fir_table_release(&h, s); return -1; }
    return fir_pair_launch(t, src, win, &h, &v, s);
}

/* the Lanczos resample of `src` (within its window cur) onto the whole of `t` */
static int lanczos_fused(const any_frame *t, const any_frame *src, float fx, float fy, int ksize, hipStream_t s) {
    const box2i *tfull = &t->full, *sw = &src->cur;
    /* halving on both axes: the decimating register-window kernel */
    const float identity = 1.0f;
    cvk_blur_halve_params hp;
    if (halving_sweep(&hp, fx, fy, ksize, &identity, 1, t, src) && CVK(cvk_blur_supported)(hp.ntaps2, 2)) {
        int rc, kernel;
        if (src->half && t->half && CVK(cvk_blur_halve_takes_pairs)(&hp)) {
            /* f16 frames: config 3's two-column sweep behind the identity blur (one tap of weight 1: x * 1.0f is x) */
            rc = CVK(cvk_blur_halve_pair)(&hp, cvs_cus(), s);
            kernel = CVS_FIR_KERNEL_HALVE_PAIR;
        } else {
            cvk_blur_params bp;
            memset(&bp, 0, sizeof bp);
            bp.target = hp.target; bp.source = hp.source;
            bp.in_half = src->half; bp.out_half = t->half;
            bp.tx0 = hp.tx0; bp.ty0 = hp.ty0; bp.tx1 = hp.tx1; bp.ty1 = hp.ty1;
            bp.sx0 = hp.sx0; bp.sy0 = hp.sy0; bp.sx1 = hp.sx1; bp.sy1 = hp.sy1;
            bp.ntaps = hp.ntaps2; bp.step = 2;
            memcpy(bp.taps, hp.taps2, sizeof(float) * (size_t)hp.ntaps2);
            rc = CVK(cvk_blur)(&bp, cvs_cus(), s);
            kernel = CVS_FIR_KERNEL_WINDOW;
        }
        if (rc != 0) { cvs_set_error("resample launch failed: %s", hipGetErrorString((hipError_t)rc)); return -1; }
        t_fir_kernel = kernel;
        return 0;
    }
    cvs_fir_table h, v;
    if (cvs_fir_table_lanczos(fx, ksize, tfull->min.x, tfull->max.x, sw->min.x, sw->max.x, CVK_FIR2D_TILE_X, &h) != 0) return -1;
    if (cvs_fir_table_lanczos(fy, ksize, tfull->min.y, tfull->max.y, sw->min.y, sw->max.y, CVK_FIR2D_TILE_Y, &v) != 0) { cvs_fir_table_release(&h, s); return -1; }
    return fir_pair_launch(t, src, tfull, &h, &v, s);
}

/* cvs_fir_blur_f32_dev / _f16_dev.  Between two f16 frames: what video_get_frame_f16 on a blur whose input is an f16 source
 * computes (widen, framework.h f16->f32 path; both passes in f32; truncate on the way out), in one launch. */
static int fir_blur(void *target, const void *source, const float *taps, int ntaps, int half, cvs_stream_t stream, const char *what) {
    frame_ref t, src;
    if (entry_refused(target, source, half, what, &t, &src, CVS_MAX_COORD)) return -1;
    if (ntaps < 1 || !taps) { cvs_set_error("blur: need at least one tap"); box2i_set_empty(t.cur); return -1; }
    hipStream_t s = cvs_pick_stream(stream);
    box2i win;
    box2i_intersect(&win, src.cur, t.full);
    *t.cur = win;
    if (box2i_is_empty(&win)) return 0;
    const any_frame tf = any_of(&t, half), sf = any_of(&src, half);      /* (taken after the window: the kernels' target view carries none) */
    int rc = blur_fused(&tf, &sf, &win, taps, ntaps, NULL, 0, NULL, s);
    if (rc != 0) box2i_set_empty(t.cur);
    return rc;
}

CVS_EXPORT int cvs_fir_blur_f32_dev(rgba_frame_f32 *target, const rgba_frame_f32 *source, const float *taps, int ntaps, cvs_stream_t stream) {
    return fir_blur(target, source, taps, ntaps, 0, stream, "cvs_fir_blur_f32_dev");
}

CVS_EXPORT int cvs_fir_blur_f16_dev(rgba_frame_f16 *target, const rgba_frame_f16 *source, const float *taps, int ntaps, cvs_stream_t stream) {
    return fir_blur(target, source, taps, ntaps, 1, stream, "cvs_fir_blur_f16_dev");
}

/* cvs_unsharp_mask_f32_dev / _f16_dev (DESIGN.md "Unsharp mask"): the blur entries' windows and refusals; per colour channel
 * d = s - B, out = |d| < threshold ? s : s + amount * d with B the blur above, alpha the source's.  One sweep (unsharp_ops.hip)
 * for the tap lists it has instances for; every other list: the blur above into a pooled f32 frame over the window, then the
 * mask alone -- same f32 values through the same expression, the same codes. */
static int unsharp_mask(void *target, const void *source, const float *taps, int ntaps, float amount, float threshold, int half,
                        cvs_stream_t stream, const char *what) {
    frame_ref t, src;
    if (entry_refused(target, source, half, what, &t, &src, CVS_MAX_COORD)) return -1;
    if (ntaps < 1 || !taps) { cvs_set_error("unsharp mask: need at least one tap"); box2i_set_empty(t.cur); return -1; }
    hipStream_t s = cvs_pick_stream(stream);
    box2i win;
    box2i_intersect(&win, src.cur, t.full);
    *t.cur = win;
    /* the tap list picks the path; a window without pixels is taken by that path too (nothing to launch) */
    const bool fused = blur_has_fast_kernel(taps, ntaps) && CVK(cvk_unsharp_supported)(ntaps);
    t_fir_kernel = fused ? CVS_FIR_KERNEL_UNSHARP : CVS_FIR_KERNEL_NONE;
    if (box2i_is_empty(&win)) return 0;
    const any_frame tf = any_of(&t, half), sf = any_of(&src, half);
    int rc;
    if (fused) {
        cvk_unsharp_params up;
        memset(&up, 0, sizeof up);
        up.target = cvs_view(tf.data, &tf.full);
        up.source = cvs_view(sf.data, &sf.full);
        up.half = half;
        up.tx0 = win.min.x; up.ty0 = win.min.y; up.tx1 = win.max.x; up.ty1 = win.max.y;
        up.sx0 = sf.cur.min.x; up.sy0 = sf.cur.min.y; up.sx1 = sf.cur.max.x; up.sy1 = sf.cur.max.y;
        up.ntaps = ntaps;
        up.amount = amount; up.threshold = threshold;
        memcpy(up.taps, taps, sizeof(float) * (size_t)ntaps);
        rc = CVK(cvk_unsharp)(&up, cvs_cus(), s);
        if (rc != 0) { cvs_set_error("unsharp mask launch failed: %s", hipGetErrorString((hipError_t)rc)); rc = -1; }
    } else {
        any_frame mid = { NULL, win, win, 0 };
        mid.data = cvs_pool_malloc(cvs_box_pixels(&win) * sizeof(rgba_f32), s);
        if (!mid.data) { box2i_set_empty(t.cur); return -1; }
        rc = blur_fused(&mid, &sf, &win, taps, ntaps, NULL, 0, NULL, s);
        if (rc == 0) {
            const cvk_rect r = { win.min.x, win.min.y, win.max.x, win.max.y };
            rc = CVK(cvk_unsharp_combine)(cvs_view(tf.data, &tf.full), cvs_view(sf.data, &sf.full), cvs_view(mid.data, &mid.full), r, half, amount, threshold, s);
            if (rc != 0) { cvs_set_error("unsharp mask launch failed: %s", hipGetErrorString((hipError_t)rc)); rc = -1; }
        }
        cvs_pool_free(mid.data, s);
    }
    if (rc != 0) box2i_set_empty(t.cur);
    return rc;
}

CVS_EXPORT int cvs_unsharp_mask_f32_dev(rgba_frame_f32 *target, const rgba_frame_f32 *source, const float *taps, int ntaps, float amount, float threshold, cvs_stream_t s) {
    return unsharp_mask(target, source, taps, ntaps, amount, threshold, 0, s, "cvs_unsharp_mask_f32_dev");
}

CVS_EXPORT int cvs_unsharp_mask_f16_dev(rgba_frame_f16 *target, const rgba_frame_f16 *source, const float *taps, int ntaps, float amount, float threshold, cvs_stream_t s) {
    return unsharp_mask(target, source, taps, ntaps, amount, threshold, 1, s, "cvs_unsharp_mask_f16_dev");
}

/* A workspace whose lowest item is a blur node on an f16 source and whose higher items are f16 frames, pulled as
 * f16: workspace.c:530-544 fetches the base as f32 (the blur's own format, no rounding), blends every higher
 * item over it with video_mix_over_f32 at mix 1.0, and main.c:43-71 truncates the result.  One launch when every
 * window is the whole output frame; otherwise the same nodes one by one on f32 frames. */
CVS_EXPORT int cvs_blur_over_f16_dev(rgba_frame_f16 *out, const rgba_frame_f16 *source, const float *taps, int ntaps,
                                     const rgba_frame_f16 *const *overlays, int noverlays, cvs_stream_t stream) {
    /* out may be one of the overlays -- a lane reads an overlay's pixel where it writes, before it writes, and node by node
     * the output is written last -- but not the source, which the blur gathers from */
    if (out->data && out->data == source->data) {
        cvs_set_error("cvs_blur_over_f16_dev: the target is the source's buffer: the operation is not in place");
        box2i_set_empty(&out->current_window);
        return -1;
    }
    if (cvs_enter() != 0) { box2i_set_empty(&out->current_window); return -1; }
    CVS_REQUIRE_INSIDE(source, out, "cvs_blur_over_f16_dev");
    CVS_REQUIRE_COORDS(source, 1, out, "cvs_blur_over_f16_dev", "source");
    CVS_REQUIRE_COORDS(out, 0, out, "cvs_blur_over_f16_dev", "out");
    for (int l = 0; l < noverlays && overlays; l++) CVS_REQUIRE_COORDS(overlays[l], 1, out, "cvs_blur_over_f16_dev", "an overlay");
    if (ntaps < 1 || !taps || noverlays < 0 || (noverlays > 0 && !overlays)) { cvs_set_error("blur+over: bad arguments"); box2i_set_empty(&out->current_window); return -1; }
    if (noverlays == 0) return cvs_fir_blur_f16_dev(out, source, taps, ntaps, stream);       /* a stack of one: the blur node pulled as f16 */
    hipStream_t s = cvs_pick_stream(stream);
    const box2i *full = &out->full_window;
    if (box2i_is_empty(full)) { box2i_set_empty(&out->current_window); return 0; }
    const any_frame o = { out->data, *full, *full, 1 }, src = { (void *)source->data, source->full_window, source->current_window, 1 };
    box2i win;
    box2i_intersect(&win, &source->current_window, full);
    bool whole = noverlays <= CVK_BLUR_MAX_OVER && memcmp(&win, full, sizeof win) == 0;
    const void *bufs[CVK_BLUR_MAX_OVER];
    for (int l = 0; whole && l < noverlays; l++) {
        whole = memcmp(&overlays[l]->full_window, full, sizeof *full) == 0 && memcmp(&overlays[l]->current_window, full, sizeof *full) == 0;
        bufs[l] = overlays[l]->data;
    }
    int rc = 1;
    if (whole && noverlays > 0) rc = blur_fused(&o, &src, &win, taps, ntaps, bufs, noverlays, NULL, s);
    if (rc == 0) { out->current_window = *full; return 0; }
    if (rc < 0) { box2i_set_empty(&out->current_window); return rc; }

    rgba_frame_f32 acc = { cvs_pool_malloc(cvs_box_pixels(full) * sizeof(rgba_f32), s), *full, *full };
    rgba_frame_f32 tmp = { noverlays > 0 ? cvs_pool_malloc(cvs_box_pixels(full) * sizeof(rgba_f32), s) : NULL, *full, *full };
    rc = (acc.data && (tmp.data || noverlays == 0)) ? 0 : -1;
    if (rc == 0) {
        box2i_set_empty(&acc.current_window);
        if (!box2i_is_empty(&win)) {
            const any_frame a = { acc.data, *full, win, 0 };
            acc.current_window = win;
            rc = blur_fused(&a, &src, &win, taps, ntaps, NULL, 0, NULL, s);
        }
    }
    for (int l = 0; rc == 0 && l < noverlays; l++) {
        rc = cvs_frame_f16_to_f32_dev(&tmp, overlays[l], s);
        if (rc == 0) rc = cvs_mix_over_f32_dev(&acc, &tmp, 1.0f, s);
    }
    if (rc == 0) rc = cvs_frame_f32_to_f16_dev(out, &acc, s);
    cvs_pool_free(acc.data, s); cvs_pool_free(tmp.data, s);
    if (rc != 0) box2i_set_empty(&out->current_window);
    return rc;
}

/* cvs_resample_lanczos_f32_dev / _f16_dev.  Between two f16 frames: what an f16 pull of a Lanczos node over a half-native
 * source computes -- widen (main.c:105-144), the two f32 passes, truncate (main.c:43-71) -- with the widen on the kernel's
 * loads and the truncate on its stores: 8 B read per source pixel + 8 B written per target pixel, no f32 frame anywhere. */
static int resample_lanczos(void *target, const void *source, float fx, float fy, int ksize, int half, cvs_stream_t stream, const char *what) {
    frame_ref t, src;
    if (entry_refused(target, source, half, what, &t, &src, CVS_RESAMPLE_MAX_COORD)) return -1;
    if (!(fx > 0.0f) || !(fy > 0.0f) || ksize < 1 || box2i_is_empty(src.cur) || box2i_is_empty(t.full)) {
        box2i_set_empty(t.cur);
        return 0;
    }
    hipStream_t s = cvs_pick_stream(stream);
    const any_frame tf = any_of(&t, half), sf = any_of(&src, half);
    int rc = lanczos_fused(&tf, &sf, fx, fy, ksize, s);
    if (rc == 0) *t.cur = *t.full;
    else box2i_set_empty(t.cur);
    return rc;
}

CVS_EXPORT int cvs_resample_lanczos_f32_dev(rgba_frame_f32 *target, const rgba_frame_f32 *source, float fx, float fy, int ksize, cvs_stream_t stream) {
    return resample_lanczos(target, source, fx, fy, ksize, 0, stream, "cvs_resample_lanczos_f32_dev");
}

CVS_EXPORT int cvs_resample_lanczos_f16_dev(rgba_frame_f16 *target, const rgba_frame_f16 *source, float fx, float fy, int ksize, cvs_stream_t stream) {
    return resample_lanczos(target, source, fx, fy, ksize, 1, stream, "cvs_resample_lanczos_f16_dev");
}

/* BASELINE config 3 on f16 frames: widen -> blur (f32) -> Lanczos resample (f32) -> truncate, as two fused
 * launches with one f32 intermediate; the widen and the truncate ride on the first load and the last store. */
CVS_EXPORT int cvs_blur_lanczos_f16_dev(rgba_frame_f16 *target, const rgba_frame_f16 *source, const float *taps, int ntaps,
                                        float fx, float fy, int ksize, cvs_stream_t stream) {
    if (target->data && target->data == source->data) {
        cvs_set_error("cvs_blur_lanczos_f16_dev: the target is the source's buffer: the operation is not in place");
        box2i_set_empty(&target->current_window);
        return -1;
    }
    if (cvs_enter() != 0) { box2i_set_empty(&target->current_window); return -1; }
    CVS_REQUIRE_INSIDE(source, target, "cvs_blur_lanczos_f16_dev");
    if (cvs_coords_refused("cvs_blur_lanczos_f16_dev", "source", &source->full_window, &source->current_window, CVS_RESAMPLE_MAX_COORD) ||
        cvs_coords_refused("cvs_blur_lanczos_f16_dev", "target", &target->full_window, NULL, CVS_RESAMPLE_MAX_COORD)) {
        box2i_set_empty(&target->current_window);
        return -1;
    }
    if (ntaps < 1 || !taps || !(fx > 0.0f) || !(fy > 0.0f) || ksize < 1) { cvs_set_error("blur+lanczos: bad arguments"); box2i_set_empty(&target->current_window); return -1; }
    if (box2i_is_empty(&source->current_window) || box2i_is_empty(&target->full_window)) { box2i_set_empty(&target->current_window); return 0; }
    hipStream_t s = cvs_pick_stream(stream);
    /* the blurred frame covers the source's current window (blur: output window = source window) */
    const box2i *sw = &source->current_window;
    const any_frame tf = { target->data, target->full_window, target->full_window, 1 }, sf = { (void *)source->data, source->full_window, *sw, 1 };
    /* a one-tap "blur" with weight 1 is the identity (0.0f + x * 1.0f == x): the resampler alone, f16 to f16 */
    if (ntaps == 1 && taps[0] == 1.0f) return cvs_resample_lanczos_f16_dev(target, source, fx, fy, ksize, stream);
    /* halving on both axes after an odd blur: one sweep, no intermediate frame (blur_halve_ops.hip) */
    cvk_blur_halve_params hp;
    if ((ntaps & 1) && halving_sweep(&hp, fx, fy, ksize, taps, ntaps, &tf, &sf) && CVK(cvk_blur_halve_supported)(ntaps, hp.ntaps2)) {
        const int rc = halving_launch(&hp, s);
        if (rc == 0) target->current_window = target->full_window;
        else box2i_set_empty(&target->current_window);
        return rc;
    }
    any_frame mid = { NULL, *sw, *sw, 0 };
    mid.data = cvs_pool_malloc(cvs_box_pixels(sw) * sizeof(rgba_f32), s);
    if (!mid.data) { box2i_set_empty(&target->current_window); return -1; }
    int rc = blur_fused(&mid, &sf, sw, taps, ntaps, NULL, 0, NULL, s);
    if (rc == 0) rc = lanczos_fused(&tf, &mid, fx, fy, ksize, s);
    if (rc == 0) target->current_window = target->full_window;
    cvs_pool_free(mid.data, s);
    if (rc != 0) box2i_set_empty(&target->current_window);
    return rc;
}

/* cvs_blur_over_f16_dev for `count` independent frames in as few launches as possible: frames that share one geometry
 * (every window equal to the first frame's, whole-frame layers) and do not feed each other go CVK_FRAME_BATCH at a time
 * into ONE launch whose segments are sized for the whole batch (fewer halo rows re-filtered per frame); anything else is
 * carried out frame by frame, exactly as `count` single calls would.  overlays: count x noverlays pointers, frame-major. */
CVS_EXPORT int cvs_blur_over_f16_batch_dev(rgba_frame_f16 *const *outs, const rgba_frame_f16 *const *sources, const float *taps, int ntaps,
                                           const rgba_frame_f16 *const *overlays, int noverlays, int count, cvs_stream_t stream) {
    const char *what = "cvs_blur_over_f16_batch_dev";
    if (count <= 0) return 0;
    if (ntaps < 1 || !taps || noverlays < 0 || (noverlays > 0 && !overlays)) { cvs_set_error("%s: bad arguments", what); return -1; }
    for (int i = 0; i < count; i++)
        for (int l = 0; l < noverlays; l++)
            if (!overlays[(size_t)i * noverlays + l]) { cvs_set_error("%s: layer %d of frame %d is a null pointer", what, l, i); return -1; }
    if (batch_refused(outs, sources, count, 1, what, CVS_MAX_COORD)) return -1;
    for (int i = 0; i < count * noverlays; i++)
        if (cvs_coords_refused(what, "an overlay", &overlays[i]->full_window, &overlays[i]->current_window, CVS_MAX_COORD)) { batch_empty_from(outs, 0, count, 1); return -1; }
    hipStream_t s = cvs_pick_stream(stream);
    const box2i *full = &outs[0]->full_window;
    bool uniform = count > 1 && noverlays >= 1 && noverlays <= CVK_BLUR_MAX_OVER && !box2i_is_empty(full) && blur_has_fast_kernel(taps, ntaps) && (ntaps & 1);
    for (int i = 0; uniform && i < count; i++) {
        uniform = same_box(&outs[i]->full_window, full) && same_box(&sources[i]->full_window, &sources[0]->full_window) &&
                  same_box(&sources[i]->current_window, full) && same_box(&sources[0]->full_window, full);
        for (int l = 0; uniform && l < noverlays; l++) {
            const rgba_frame_f16 *ov = overlays[(size_t)i * noverlays + l];
            uniform = same_box(&ov->full_window, full) && same_box(&ov->current_window, full);
        }
    }
    int rc = 0, done = 0;
    const size_t bytes = cvs_box_pixels(full) * sizeof(rgba_f16);
    while (uniform && rc == 0 && done < count) {
        const int n = count - done < CVK_FRAME_BATCH ? count - done : CVK_FRAME_BATCH;
        cvk_frame_batch b;
        if (!batch_group(&b, outs, sources, 1, done, n, bytes, bytes, overlays, noverlays)) break;     /* the rest frame by frame */
        const any_frame t = { b.target[0], *full, *full, 1 }, src = { (void *)b.source[0], sources[done]->full_window, sources[done]->current_window, 1 };
        rc = blur_fused(&t, &src, full, taps, ntaps, b.over[0], noverlays, &b, s);
        if (rc == 1) { rc = 0; break; }
        if (rc == 0) { for (int i = 0; i < n; i++) outs[done + i]->current_window = *full; done += n; }
    }
    for (; rc == 0 && done < count; done++)
        rc = cvs_blur_over_f16_dev(outs[done], sources[done], taps, ntaps, noverlays ? overlays + (size_t)done * noverlays : NULL, noverlays, stream);
    if (rc != 0) batch_empty_from(outs, done, count, 1);
    return rc;
}

/* cvs_blur_lanczos_f16_dev for `count` independent frames: the one-sweep form (odd blur, halving on both axes) takes
 * CVK_FRAME_BATCH frames of one geometry per launch; anything else frame by frame. */
CVS_EXPORT int cvs_blur_lanczos_f16_batch_dev(rgba_frame_f16 *const *targets, const rgba_frame_f16 *const *sources, int count,
                                              const float *taps, int ntaps, float fx, float fy, int ksize, cvs_stream_t stream) {
    const char *what = "cvs_blur_lanczos_f16_batch_dev";
    if (count <= 0) return 0;
    if (ntaps < 1 || !taps || !(fx > 0.0f) || !(fy > 0.0f) || ksize < 1) { cvs_set_error("%s: bad arguments", what); return -1; }
    if (batch_refused(targets, sources, count, 1, what, CVS_RESAMPLE_MAX_COORD)) return -1;
    hipStream_t s = cvs_pick_stream(stream);
    int rc = 0, done = 0;
    const box2i *tf = &targets[0]->full_window, *sw = &sources[0]->current_window;
    bool uniform = count > 1 && (ntaps & 1) && !(ntaps == 1 && taps[0] == 1.0f) && !box2i_is_empty(sw) && !box2i_is_empty(tf);
    for (int i = 1; uniform && i < count; i++)
        uniform = same_box(&targets[i]->full_window, tf) && same_box(&sources[i]->full_window, &sources[0]->full_window) &&
                  same_box(&sources[i]->current_window, sw);
    const any_frame t0 = { targets[0]->data, *tf, *tf, 1 }, s0 = { (void *)sources[0]->data, sources[0]->full_window, *sw, 1 };
    cvk_blur_halve_params hp;
    if (uniform && halving_sweep(&hp, fx, fy, ksize, taps, ntaps, &t0, &s0) && CVK(cvk_blur_halve_supported)(ntaps, hp.ntaps2)) {
        const size_t sbytes = cvs_box_pixels(&sources[0]->full_window) * sizeof(rgba_f16), tbytes = cvs_box_pixels(tf) * sizeof(rgba_f16);
        while (rc == 0 && done < count) {
            const int n = count - done < CVK_FRAME_BATCH ? count - done : CVK_FRAME_BATCH;
            if (!batch_group(&hp.batch, targets, sources, 1, done, n, tbytes, sbytes, NULL, 0)) break;
            /* hp is frame 0's otherwise: cvs_view's pitch and extent come from the box alone, the same for every frame here */
            hp.target.data = hp.batch.target[0];
            hp.source.data = (void *)hp.batch.source[0];
            if ((rc = halving_launch(&hp, s)) != 0) break;
            for (int i = 0; i < n; i++) targets[done + i]->current_window = targets[done + i]->full_window;
            done += n;
        }
    }
    for (; rc == 0 && done < count; done++)
        rc = cvs_blur_lanczos_f16_dev(targets[done], sources[done], taps, ntaps, fx, fy, ksize, stream);
    if (rc != 0) batch_empty_from(targets, done, count, 1);
    return rc;
}
