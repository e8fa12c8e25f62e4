/*
 * internal.h -- shared by the host C files of libcanvas_hip.so.  Not installed.
 */
#ifndef CVS_INTERNAL_H
#define CVS_INTERNAL_H

#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "canvas_hip.h"
#include "../kernels/kernels.h"

/* ---- error plumbing: frame functions return void in the reference and signal failure through an
 * empty current_window (src/cprocess/main.c:35-38); the message goes to cvs_last_error() and, like
 * a g_warning, to stderr. */
void cvs_set_error(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
void cvs_clear_error(void);
/* a notice for the log handler (or stderr) that is NOT an error of the call in progress: cvs_last_error() is left alone */
void cvs_log_warning(const char *fmt, ...) __attribute__((format(printf, 1, 2)));

#define CVS_HIP(expr)                                                                          \
    do {                                                                                       \
        hipError_t cvs_e_ = (expr);                                                            \
        if (cvs_e_ != hipSuccess) {                                                            \
            cvs_set_error("%s: %s (%s:%d)", #expr, hipGetErrorString(cvs_e_), __FILE__, __LINE__); \
            return (int)cvs_e_ ? (int)cvs_e_ : -1;                                             \
        }                                                                                      \
    } while (0)

/* runtime.c: see there -- 1 when a graph being captured on `st` took over the hold on a cached table */
int cvs_capture_hold(hipStream_t st, void (*release)(void *), void *arg);

#define CVS_KERNEL(expr)                                                                       \
    do {                                                                                       \
        int cvs_k_ = (expr);                                                                   \
        if (cvs_k_ != 0) {                                                                     \
            cvs_set_error("%s: %s (%s:%d)", #expr, hipGetErrorString((hipError_t)cvs_k_), __FILE__, __LINE__); \
            return cvs_k_;                                                                     \
        }                                                                                      \
    } while (0)

/* The arithmetic flavour of the call the calling thread is in (canvas_hip.h cvs_set_arithmetic; snapshot taken by
 * cvs_enter()), and the launcher of that flavour: CVK(cvk_blur)(&bp, cus, s) is cvk_blur or cvk_blur_fma (kernels.h). */
int cvs_arith(void);
#define CVK(name) (cvs_arith() ? name##_fma : name)

/* Device contexts (runtime.c): the id of the context the calling thread's current call runs in -- set by cvs_enter().
 * Whatever a file keeps ON the device for the library's own use (cached tables) is kept per context: arrays of
 * CVS_MAX_CONTEXTS, indexed with cvs_ctx(). */
#define CVS_MAX_CONTEXTS 64
int cvs_ctx(void);

/* binds the calling thread to its context's device (cvs_set_context, else the default context; lazily opens context 0 on
 * CVS_DEVICE, default 0) and takes the snapshots of the call: context id, arithmetic flavour.  0 on success. */
int cvs_enter(void);
/* the stream to enqueue on: the caller's, or this thread's own when NULL */
hipStream_t cvs_pick_stream(cvs_stream_t s);
int cvs_cus(void);

/* width and height in 64 bit: max - min + 1 of a box2i does not fit an int for every box (canvas_hip.h box2i_get_size does it
 * in int, as the reference's does, and is for boxes inside the coordinate contract) */
static inline long long cvs_box_width(const box2i *b) { return box2i_is_empty(b) ? 0 : (long long)b->max.x - b->min.x + 1; }
static inline long long cvs_box_height(const box2i *b) { return box2i_is_empty(b) ? 0 : (long long)b->max.y - b->min.y + 1; }
static inline size_t cvs_box_pixels(const box2i *b) { return (size_t)cvs_box_width(b) * (size_t)cvs_box_height(b); }

static inline cvk_view cvs_view(void *data, const box2i *full) {
    cvk_view v;
    v.data = data;
    v.pitch = full->max.x < full->min.x ? 0 : (int)((long long)full->max.x - full->min.x + 1);     /* (fits: cvs_coords_refused) */
    v.fx0 = full->min.x; v.fy0 = full->min.y; v.fx1 = full->max.x; v.fy1 = full->max.y;
    return v;
}

static inline cvk_rect cvs_rect(const box2i *b) {
    cvk_rect r = { b->min.x, b->min.y, b->max.x, b->max.y };
    return r;
}

static inline bool cvs_box_contains(const box2i *outer, const box2i *inner) {
    return box2i_is_empty(inner) ||
           (inner->min.x >= outer->min.x && inner->min.y >= outer->min.y && inner->max.x <= outer->max.x && inner->max.y <= outer->max.y);
}

/* A frame whose current_window reaches outside its own buffer would send a kernel out of bounds: refuse it here,
 * loudly, with the output marked empty.  (The reference would read past the buffer.) */
#define CVS_REQUIRE_INSIDE(in_frame, out_frame, what)                                                      \
    do {                                                                                                   \
        if (!cvs_box_contains(&(in_frame)->full_window, &(in_frame)->current_window)) {                   \
            cvs_set_error("%s: the input's current_window lies outside its buffer", what);                \
            box2i_set_empty(&(out_frame)->current_window);                                                 \
            return -1;                                                                                     \
        }                                                                                                  \
    } while (0)

/* The coordinate contract (canvas_hip.h, beside the frame structs; DESIGN.md "Coordinates"): kernels and launchers form
 * y1 + 1, x + 127, y0 + seg - 1, window + halo in `int`, which is exact only while the coordinates leave headroom.  An operand
 * outside +-lim, or a buffer whose width or height does not fit an int, is refused here, before anything is launched. */
static inline bool cvs_box_within(const box2i *b, int lim) {
    return box2i_is_empty(b) || (b->min.x >= -lim && b->min.y >= -lim && b->max.x <= lim && b->max.y <= lim);
}
/* true, with the error set, for a frame operand the contract excludes.  `cur`: NULL where the entry does not read the
 * operand's current_window (a pure output).  Empty windows are exempt. */
static inline bool cvs_coords_refused(const char *what, const char *operand, const box2i *full, const box2i *cur, int lim) {
    const box2i *bad = !cvs_box_within(full, lim) ? full : (cur && !cvs_box_within(cur, lim) ? cur : NULL);
    if (bad) {
        cvs_set_error("%s: %s: %s (%d, %d)-(%d, %d) has a coordinate beyond +-%d%s", what, operand, bad == full ? "full_window" : "current_window",
                      bad->min.x, bad->min.y, bad->max.x, bad->max.y, lim, lim == CVS_MAX_COORD ? " (CVS_MAX_COORD)" : ", where a float no longer holds every integer");
        return true;
    }
    if (cvs_box_width(full) > 0x7fffffffLL || cvs_box_height(full) > 0x7fffffffLL) {
        cvs_set_error("%s: %s: full_window is %lld x %lld, which no int holds", what, operand, cvs_box_width(full), cvs_box_height(full));
        return true;
    }
    return false;
}
/* The filters of the two warps (host/transform.c, host/perspective.c), said once so that their windows cannot drift apart: which
 * values of `filter` there are; how far from a source coordinate a filter's taps reach (nearest: half a pixel; bilinear: i .. i + 1;
 * Catmull-Rom: i - 1 .. i + 2), which S is grown by for the target window; and the pad of the source window around the mapped
 * corners of a target window. */
static inline bool cvs_warp_filter_known(int filter) { return filter == CVS_TRANSFORM_NEAREST || filter == CVS_TRANSFORM_BILINEAR || filter == CVS_TRANSFORM_CATMULL_ROM; }
static inline double cvs_warp_filter_reach(int filter) { return filter == CVS_TRANSFORM_CATMULL_ROM ? 2.0 : (filter == CVS_TRANSFORM_BILINEAR ? 1.0 : 0.5); }
static inline double cvs_warp_filter_pad(int filter) { return filter == CVS_TRANSFORM_CATMULL_ROM ? 3.0 : 2.0; }
#define CVS_WARP_FILTER_REFUSAL "%s: filter %d is none of CVS_TRANSFORM_NEAREST, CVS_TRANSFORM_BILINEAR and CVS_TRANSFORM_CATMULL_ROM"

static inline bool cvs_point_refused(const char *what, const char *operand, v2f p, int lim) {
    if (p.x >= -(float)lim && p.x <= (float)lim && p.y >= -(float)lim && p.y <= (float)lim) return false;
    cvs_set_error("%s: %s: point (%g, %g) lies beyond +-%d", what, operand, p.x, p.y, lim);
    return true;
}
/* a frame of either format; reads_cur: the entry reads its current_window (an input, an output worked on in place) */
#define CVS_REQUIRE_COORDS(frame, reads_cur, out_frame, what, operand)                                                         \
    do {                                                                                                                       \
        if (cvs_coords_refused(what, operand, &(frame)->full_window, (reads_cur) ? &(frame)->current_window : NULL, CVS_MAX_COORD)) { \
            box2i_set_empty(&(out_frame)->current_window);                                                                     \
            return -1;                                                                                                         \
        }                                                                                                                      \
    } while (0)

/* ---- staging of one flat host array (halfconv.c, display.c; the bridge below is built on it): H2D -> kernels -> D2H */
typedef struct {
    void *dev;            /* device copy of the whole buffer (from the stream-ordered pool); NULL for a zero-byte one */
    size_t bytes;
    hipStream_t stream;   /* the stream it was staged on: the block goes back to the pool on it */
} cvs_staged;

int cvs_stage_in(cvs_staged *st, const void *host, size_t bytes, int upload, hipStream_t s);
int cvs_stage_out(cvs_staged *st, void *host, hipStream_t s);      /* D2H + sync */
void cvs_stage_free(cvs_staged *st);

/* ---- bridge.c: what every reference-named entry point on host frames does around its `_dev` twin.  Open, add the frames
 * (and coded planes) the call touches, run the twin, close.  The first step that fails is kept in `rc` and every later step
 * is skipped, so a caller never tracks which blocks exist; close frees them all, whatever happened.
 *     cvs_bridge br;  rgba_frame_f32 fo, fb;
 *     cvs_bridge_open(&br);
 *     CVS_BRIDGE_FRAME(&br, fo, out, CVS_BRIDGE_UPLOAD);
 *     CVS_BRIDGE_FRAME(&br, fb, b, box2i_is_empty(&b->current_window) ? 0 : CVS_BRIDGE_UPLOAD);
 *     CVS_BRIDGE_CALL(&br, cvs_mix_over_f32_dev, &fo, &fb, mix_b);
 *     out->current_window = fo.current_window;
 *     if (cvs_bridge_close(&br, out->data) != 0) box2i_set_empty(&out->current_window);                                  */
enum {
    CVS_BRIDGE_UPLOAD = 1,       /* the host bytes go up (once per block) */
    CVS_BRIDGE_PRIVATE = 2,      /* never the block of an earlier frame: for a twin that may not run in place */
    CVS_BRIDGE_BLOCKS = 4
};
typedef struct {
    hipStream_t stream;
    int rc, n;
    struct { const void *host; int uploaded; cvs_staged st; } blk[CVS_BRIDGE_BLOCKS];
} cvs_bridge;

int cvs_bridge_open(cvs_bridge *b);      /* cvs_enter + the thread's stream; the result is also b->rc */
/* device copy of a host buffer, NULL for a zero-byte one: the same buffer (pointer and size) added twice is one block */
void *cvs_bridge_frame(cvs_bridge *b, const void *host, size_t bytes, int flags);
/* three coded planes in one block, each on a 256-byte boundary: lines[p] rows of host->stride[p] bytes, uploaded or not.
 * *dev is *host with the device pointers and those line counts; _back downloads what *dev describes into host's planes */
void cvs_bridge_planes(cvs_bridge *b, coded_image *dev, const coded_image *host, const int lines[3], bool upload);
void cvs_bridge_planes_back(cvs_bridge *b, coded_image *host, const coded_image *dev);
/* rows and columns `window` of the added buffer `host` (px bytes per pixel, covering `full`) come back; then a wait */
int cvs_bridge_pull_window(cvs_bridge *b, void *host, const box2i *full, const box2i *window, size_t px);
/* the added buffer `out_host` comes back whole, then a wait (NULL: neither); every block is freed; returns rc */
int cvs_bridge_close(cvs_bridge *b, void *out_host);

static inline size_t cvs_frame_bytes(const box2i *full, size_t px) { return cvs_box_pixels(full) * px; }
/* dst = the device twin of host frame *src (either format): the same windows, the data pointer from the bridge.  A buffer
 * outside the coordinate contract fails the bridge before a byte is staged for it (the `_dev` twin would refuse it, and names
 * itself when a current_window is what breaks the contract). */
#define CVS_BRIDGE_FRAME(b, dst, src, flags)                                                                                  \
    do {                                                                                                                      \
        (dst) = *(src);                                                                                                       \
        if ((b)->rc == 0 && cvs_coords_refused("host frame", #src, &(src)->full_window, NULL, CVS_MAX_COORD)) (b)->rc = -1;   \
        (dst).data = cvs_bridge_frame(b, (src)->data, cvs_frame_bytes(&(src)->full_window, sizeof *(src)->data), flags);      \
    } while (0)
/* fn(args..., the bridge's stream) unless an earlier step failed */
#define CVS_BRIDGE_CALL(b, fn, ...) do { if ((b)->rc == 0) (b)->rc = fn(__VA_ARGS__, (b)->stream); } while (0)

/* coded planes of a w x h luma raster with cw x ch chroma: which of the two things an entry asks of them fails first */
enum { CVS_PLANES_OK = 0, CVS_PLANES_MISSING, CVS_PLANES_SMALL };
int cvs_planes_check(const coded_image *image, int w, int h, int cw, int ch);
static inline cvk_dv_planes cvs_planes_view(const coded_image *p) {
    cvk_dv_planes v = { p->data[0], p->data[1], p->data[2], p->stride[0], p->stride[1], p->stride[2] };
    return v;
}

/* ---- ycc_common.c: what the Y'CbCr edges share (mpeg2.c, ycc422.c, ycc420.c) ---- */
/* the nine coefficients row by row, Y'CbCr -> R'G'B' (import) or R'G'B' -> Y'CbCr (export): Rec.2020 with CVS_YCC_REC2020, Rec.709
 * with CVS_YCC_REC709, else Rec.601 (an entry refuses the flags it does not take before it asks) */
const float *cvs_ycc_to_rgb(int flags);
const float *cvs_rgb_to_ycc(int flags);
/* the tail of cvs_ycc42x_layout: `planes` with s and l copied to whichever of the caller's arrays is there; -1 for planes == 0 (the
 * layout or the size was refused, error set) */
int cvs_ycc_layout_out(int planes, const int s[3], const int l[3], int strides[3], int line_counts[3]);
/* everything an entry asks of the image, given the layout's planes, least strides, line counts and the alignment of bases and
 * strides; 0 and *view filled, or -1 with the error set */
int cvs_ycc_image_check(const char *what, const coded_image *image, int planes, const int strides[3], const int lines[3], int align, const char *layout_name,
                        int width, int height, cvk_ycc_image *view);
/* *w = `window` clipped to the width x height raster at the origin; true where nothing is left (or `window` itself is empty) */
bool cvs_raster_window(const box2i *window, int width, int height, box2i *w);
/* the same as the rectangle an export kernel reads inside: pixels outside the current window (and outside the raster) count as
 * black; {0, 0, -1, -1} where nothing is left */
cvk_rect cvs_raster_rect(const box2i *window, int width, int height);
/* The half table of an edge, the separate flavour's in both flavours: the pixels must not depend on the flavour.  The contracted
 * build of linear -> Rec.709 fuses a * pow - b and differs at code 0x789b; the two build Rec.709 -> linear alike today, the rule
 * keeps it so.  NULL with the error set. */
const half *cvs_ycc_export_lut(void);      /* linear -> Rec.709 */
const half *cvs_ycc_import_lut(void);      /* Rec.709 -> linear (scene) */

/* ---- display.c: the display edge's cached 64 KiB byte table of (pre_lut, ramp), for the scopes.  rendering_intent 0: the
 * gamma-0.45 ramp, > 0: the widget's.  _lock returns the table with the cache's lock HELD (an eviction cannot rewrite it), or
 * NULL with the error set and the lock released; _unlock goes behind the launch that reads the table and, when that launch was
 * recorded into a graph on `s` (enqueued), lets the graph hold the table until it is destroyed. */
const uint8_t *cvs_display_table_lock(int pre_lut, float rendering_intent, int *slot);
void cvs_display_table_unlock(int slot, bool enqueued, hipStream_t s);

/* device LUT for an id, NULL for CVS_LUT_NONE; builds the tables on first use */
const half *cvs_lut_dev_or_null(int which);
/* the table as the separate-arithmetic flavour builds it, whatever the call's flavour (cvs_lut_device follows the flavour:
 * linear -> Rec.709 and linear -> sRGB differ between the two) */
const half *cvs_lut_device_separate(int which);

/* a * b + c where the reference's C has it in ONE expression (video_scale.c:65,257-277): rounded twice as its gcc build does,
 * or once -- the fused multiply-add its clang build emits -- in the contracted flavour (canvas_hip.h cvs_set_arithmetic).
 * The host C is compiled with -ffp-contract=off, so the first form never fuses by itself. */
static inline float madd_as(int contracted, float a, float b, float c) { return contracted ? fmaf(a, b, c) : a * b + c; }

/* ---- fir_tables.c: the separable FIR kernels' tap tables, one per axis, planned on the host and cached on the device per
 * context.  A lookup returns 0 and the table PINNED: it stays on the device until cvs_fir_table_release() says the launch
 * that reads it is on its stream (or hands the hold to the graph being captured there).  On failure pin is -1 and the error
 * is set.  Target lines t0..t1 read source lines s0..s1; `tile`: the k_fir2d tile edge along this axis (max_foot's unit). */
typedef struct {
    cvk_fir_axis axis;
    int max_foot;             /* most source lines any tile of the table reads */
    int used_lo, used_hi;     /* target lines that receive at least one tap */
    int pin;
} cvs_fir_table;
/* the blur: the same taps for every line, centre ntaps / 2 */
int cvs_fir_table_blur(const float *taps, int ntaps, int t0, int t1, int s0, int s1, int tile, cvs_fir_table *out);
/* the Lanczos resampler: per target line filter_createLanczos(factor, ksize, frac(t / factor)) */
int cvs_fir_table_lanczos(float factor, int ksize, int t0, int t1, int s0, int s1, int tile, cvs_fir_table *out);
/* one pass of video_scale_bilinear_f32 (video_scale.c:34-229) in the call's arithmetic flavour; count_touch: an in-range tap
 * marks its target line as used even when the other axis is empty (the vertical pass).  Tile edge CVK_FIR2D_TILE_X. */
int cvs_fir_table_triangle(float tmin, float smin, float factor, int s0, int s1, int t0, int t1, bool count_touch, cvs_fir_table *out);
void cvs_fir_table_release(cvs_fir_table *t, hipStream_t s);

#endif
