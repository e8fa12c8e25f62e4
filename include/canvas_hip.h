/*
 * canvas_hip.h -- C-ABI of the MI355X (gfx950) implementation of Canvas's per-pixel video path.
 *
 * One shared library, libcanvas_hip.so, exports
 *   (1) the symbol set of the reference's src/cprocess for this path, with the same names,
 *       argument meaning and error behaviour, working on HOST frames (each call stages the
 *       frames to HBM, runs the HIP kernels, and copies the result back: drop-in, PCIe-bound);
 *   (2) `cvs_*_dev` twins of the same operations on frames that already live in HBM
 *       (frame->data is a device pointer), taking a stream: zero-copy, what bench.py measures;
 *   (3) the fused colour-matrix + alpha-over chain, single and batched.
 * There is no CPU implementation behind any of these: without a HIP device every pixel entry
 * point fails (empty current_window / non-zero status, message in cvs_last_error()).
 *
 * Struct layouts, field order and names are those of the reference's include/framework.h so
 * that code compiled against it keeps working:
 *   rational, v2i, box2i, v2f, box2f ........ framework.h:46-75
 *   box2i_* / min / max / clamp helpers ..... framework.h:77-149
 *   rgba_f16, rgba_u8, rgba_f32, frames ..... framework.h:155-177
 *   video_frame_source_funcs, video_source .. framework.h:185-194, 210-213
 *   fir_filter .............................. framework.h:618-627
 * GL types are gone: slot 3 of the vtable (get_frame_gl, framework.h:193) keeps its position
 * and becomes the device-frame entry, announced by VIDEO_SOURCE_FLAG_DEVICE in `flags`
 * (framework.h:190 reserves that word).
 */
#ifndef CANVAS_HIP_H
#define CANVAS_HIP_H

#include <stdint.h>
#include <stddef.h>
#include <stdbool.h>

#if defined(__cplusplus)
extern "C" {
#endif

#define CVS_EXPORT __attribute__((visibility("default")))
#define NS_PER_SEC INT64_C(1000000000)

/* ------------------------------------------------------------------ value types */

typedef uint16_t half;                 /* include/half.h:26 */
#define HALF_COUNT 65536

typedef struct { int32_t n; uint32_t d; } rational;
typedef struct { int32_t x, y; } v2i;
typedef struct { v2i min, max; } box2i;        /* inclusive; empty when max < min on either axis */
typedef struct { float x, y; } v2f;
typedef struct { v2f min, max; } box2f;

typedef struct { half r, g, b, a; } rgba_f16;  /* 8 bytes, channel order r,g,b,a */
typedef struct { uint8_t r, g, b, a; } rgba_u8;
typedef struct { float r, g, b, a; } rgba_f32; /* 16 bytes */

/* A frame is a caller-owned buffer covering full_window (rows packed, stride = its width);
 * the callee fills some sub-rectangle and reports it in current_window.  Pixels outside
 * current_window are undefined.
 *
 * Where `data` may lie (device and host entries alike; tests/test_placement_gpu.py holds every windowed cvs_*_dev entry to
 * it on frames packed into one arena):
 *   - `data` may be ANY address aligned to one pixel: 8 bytes for rgba_frame_f16, 16 bytes for rgba_frame_f32.  Nothing more
 *     is asked -- a ring of odd-width half frames packed back to back puts every second one at 8 modulo 16, and that is a
 *     legal frame.  Where a kernel has a form that moves two half pixels as one 16-byte access, the library looks at the
 *     address (and at the pitch and the window's first column) and takes that form only where every such access is aligned;
 *     the pixels are the same either way.
 *   - coded planes (coded_image.data[]) and the byte targets of cvs_frame_to_bytes_dev / cvs_frame_to_rgba8_intent_dev take
 *     any address of their element type: any byte address for planes, 4 bytes for the 32-bit display pixels.
 *   - no entry reads or writes a byte outside the buffers it is handed: full_window's width * height pixels from `data`,
 *     stride * line_count bytes of a plane, the current window's pixel count * 4 bytes of a byte target.  What lies around a
 *     frame may be another frame.
 *   - an address below the pixel's alignment (a half frame at 2 modulo 8, a float frame at 4 modulo 16) is outside the
 *     contract.
 *
 * Where a frame may lie on the canvas (tests/test_far_windows_gpu.py holds every windowed cvs_*_dev entry to it on frames moved
 * up to the bound; DESIGN.md "Coordinates" has the audit behind the value):
 *   - every coordinate of a non-empty full_window, and of a non-empty current_window the entry reads, lies within
 *     +-CVS_MAX_COORD; so does every coordinate of an explicit window an entry does not merely clip (the window of
 *     cvs_fill_solid_* is clipped to the frame by comparisons alone and may be INT_MIN..INT_MAX, "everywhere"; the `place` of
 *     cvs_scope_render_f16_dev, canvas_scope.h, is clipped to the target and fixes the picture's origin: it may overhang the
 *     bound by less than the picture's size, and is refused where no pixel of it lies within the bound) and every v2f point.  A
 *     buffer's width and height are computed in 64 bit and must fit an int.  Empty windows are exempt, whatever they hold.
 *   - an entry handed anything else returns -1 with cvs_last_error() naming the entry and the operand, every output's
 *     current_window empty and nothing launched; the video_* entries on host frames refuse the same before they stage a byte.
 *   - inside the bound every `int` a kernel forms from a coordinate -- plus a halo, a tile, a segment, a lane's overshoot -- is
 *     exact: the bound leaves 2^30 - 1 of headroom and the largest such sum adds a few thousand.
 *   - the entries that form positions in `float`, as the reference's v2f interface does, hold a tighter bound of their own,
 *     inside which a float holds every integer: CVS_TRANSFORM_MAX_COORD for cvs_transform_*, CVS_RESAMPLE_MAX_COORD for the
 *     bilinear scaler and the Lanczos resamplers (their windows; the points they are handed lie within it as well).
 *
 * How tall or wide a window may be (tests/test_extents_gpu.py holds the frame-taking cvs_*_dev entries to it at 65 535,
 * 65 536 and 70 001 rows, at 70 001 and 131 073 columns and at the row counts where a launcher's own arithmetic changes;
 * DESIGN.md "Extents" has the launcher-by-launcher table):
 *   - ANY extent.  Every entry computes any non-empty window the coordinate bounds above admit, whatever its height and
 *     width: a strip two pixels wide and 70 001 rows tall, a scan line 131 073 pixels long are legal frames.  There is no
 *     limit on the rows or columns of a window beside those bounds and the memory behind the buffer (a frame beyond 4 GiB is
 *     out of scope), and no entry refuses a window for its size.  How the launchers get there differs: the row
 *     streams, the unsharp combine, the transform and the matte keep to 65 535 workgroups along y and fold the rest (longer
 *     segments, a walk inside the kernel, one launch per band); the others (copies, conversions, fills, gain, the f32 mixers, the
 *     weave, the table FIR passes, the enlarging scaler's tiles) launch one row of workgroups per row, or per segment of
 *     rows, of the window and rest on the HIP runtime taking more of them than hipDeviceProp_t::maxGridSize[1] states, which
 *     it does on gfx950 (measured to 1 048 577).  A runtime that refused such a launch would make the entry fail with its
 *     message, not compute wrong pixels. */
enum { CVS_MAX_COORD = 1 << 30, CVS_RESAMPLE_MAX_COORD = 1 << 23 };
typedef struct { rgba_f16 *data; box2i full_window; box2i current_window; } rgba_frame_f16;
typedef struct { rgba_f32 *data; box2i full_window; box2i current_window; } rgba_frame_f32;

/* Device-resident frame handed through vtable slot 3. */
enum { CVS_FORMAT_F16 = 1, CVS_FORMAT_F32 = 2 };
typedef struct {
    void *data;            /* device pointer, layout as the host frame of `format` */
    int format;            /* set by the caller: which layout `data` has room for */
    box2i full_window;
    box2i current_window;
    void *stream;          /* hipStream_t the callee must enqueue on (NULL = the library's stream) */
} rgba_frame_dev;

typedef void (*video_get_frame_func)(void *self, int frame_index, rgba_frame_f16 *frame);
typedef void (*video_get_frame_32_func)(void *self, int frame_index, rgba_frame_f32 *frame);
typedef void (*video_get_frame_dev_func)(void *self, int frame_index, rgba_frame_dev *frame);

#define VIDEO_SOURCE_FLAG_DEVICE 0x1   /* slot 3 is a device-frame entry */

typedef struct {
    int flags;
    video_get_frame_func get_frame;
    video_get_frame_32_func get_frame_32;
    video_get_frame_dev_func get_frame_dev;     /* was get_frame_gl */
} video_frame_source_funcs;

typedef struct { void *obj; video_frame_source_funcs *funcs; } video_source;

typedef struct { float *coeff; int width; int center; } fir_filter;

/* ------------------------------------------------------------------ inline helpers (framework.h:55-149,196-208) */

static inline void v2i_add(v2i *r, const v2i *a, const v2i *b) { r->x = a->x + b->x; r->y = a->y + b->y; }
static inline void v2i_subtract(v2i *r, const v2i *a, const v2i *b) { r->x = a->x - b->x; r->y = a->y - b->y; }

#if !defined(__cplusplus)
static inline int min(int a, int b) { return a < b ? a : b; }
static inline int max(int a, int b) { return a > b ? a : b; }
static inline int clamp(int v, int lo, int hi) { return min(max(v, lo), hi); }
#endif
static inline float minf(float a, float b) { return a < b ? a : b; }
static inline float maxf(float a, float b) { return a > b ? a : b; }
static inline float clampf(float v, float lo, float hi) { return minf(maxf(v, lo), hi); }

static inline void box2i_set(box2i *b, int x0, int y0, int x1, int y1) { b->min.x = x0; b->min.y = y0; b->max.x = x1; b->max.y = y1; }
static inline void box2i_set_empty(box2i *b) { box2i_set(b, 0, 0, -1, -1); }
static inline bool box2i_is_empty(const box2i *b) { return b->max.x < b->min.x || b->max.y < b->min.y; }
static inline void box2i_intersect(box2i *r, const box2i *a, const box2i *b) {
    int x0 = a->min.x > b->min.x ? a->min.x : b->min.x, y0 = a->min.y > b->min.y ? a->min.y : b->min.y;
    int x1 = a->max.x < b->max.x ? a->max.x : b->max.x, y1 = a->max.y < b->max.y ? a->max.y : b->max.y;
    box2i_set(r, x0, y0, x1, y1);
}
static inline void box2i_union(box2i *r, const box2i *a, const box2i *b) {
    int x0 = a->min.x < b->min.x ? a->min.x : b->min.x, y0 = a->min.y < b->min.y ? a->min.y : b->min.y;
    int x1 = a->max.x > b->max.x ? a->max.x : b->max.x, y1 = a->max.y > b->max.y ? a->max.y : b->max.y;
    box2i_set(r, x0, y0, x1, y1);
}
/* an inverted axis is turned into the gap between the two spans it came from */
static inline void box2i_normalize(box2i *b) {
    if (b->min.x > b->max.x) { int32_t t = b->min.x - 1; b->min.x = b->max.x + 1; b->max.x = t; }
    if (b->min.y > b->max.y) { int32_t t = b->min.y - 1; b->min.y = b->max.y + 1; b->max.y = t; }
}
static inline void box2i_get_size(const box2i *b, v2i *r) {
    r->x = b->max.x < b->min.x ? 0 : b->max.x - b->min.x + 1;
    r->y = b->max.y < b->min.y ? 0 : b->max.y - b->min.y + 1;
}
static inline rgba_f16 *video_get_pixel_f16(rgba_frame_f16 *f, int x, int y) {
    return &f->data[(ptrdiff_t)(y - f->full_window.min.y) * (f->full_window.max.x - f->full_window.min.x + 1) + x - f->full_window.min.x];
}
static inline rgba_f32 *video_get_pixel_f32(rgba_frame_f32 *f, int x, int y) {
    return &f->data[(ptrdiff_t)(y - f->full_window.min.y) * (f->full_window.max.x - f->full_window.min.x + 1) + x - f->full_window.min.x];
}

/* ------------------------------------------------------------------ (1) reference symbol set, HOST frames
 * Each entry names the reference definition it replaces. */

/* src/cprocess/half.c:87-105 -- function-pointer globals, valid after init_half() */
CVS_EXPORT void init_half(void);
CVS_EXPORT extern void (*half_convert_from_float)(half *out, const float *in, int count);       /* truncating, half.c:47-51 */
CVS_EXPORT extern void (*half_convert_to_float)(float *out, const half *in, int count);         /* exact, half.c:31-37 */
CVS_EXPORT extern void (*half_convert_from_float_fast)(half *out, const float *in, int count);  /* half.c:53-59 */
CVS_EXPORT extern void (*half_convert_to_float_fast)(float *out, const half *in, int count);    /* half.c:39-45 */
CVS_EXPORT extern void (*half_lookup)(const half *table, half *out, const half *in, int count); /* half.c:82-85 */

static inline void rgba_f32_to_f16(rgba_f16 *out, const rgba_f32 *in, int count) { half_convert_from_float(&out->r, &in->r, count * 4); }
static inline void rgba_f16_to_f32(rgba_f32 *out, const rgba_f16 *in, int count) { half_convert_to_float(&out->r, &in->r, count * 4); }

/* src/cprocess/main.c:23-31 */
CVS_EXPORT int64_t get_frame_time(const rational *frame_rate, int frame);
CVS_EXPORT int get_time_frame(const rational *frame_rate, int64_t time);
/* src/cprocess/clock.c:28-52 */
CVS_EXPORT int64_t gettime(void);

/* src/cprocess/main.c:33-76,105-144 -- vtable dispatch + format conversion; NULL source => empty window */
CVS_EXPORT void video_get_frame_f16(video_source *source, int frame_index, rgba_frame_f16 *frame);
CVS_EXPORT void video_get_frame_f32(video_source *source, int frame_index, rgba_frame_f32 *frame);
/* src/cprocess/main.c:78-103,146-172 -- the forced pull through vtable slot 3 that force_gl=True asks for
 * (src/process/RgbaFrameF16.c:247-249): here slot 3 is the device slot; a source without one is pulled the
 * ordinary way instead of yielding an empty window */
CVS_EXPORT void video_get_frame_f16_gl(video_source *source, int frame_index, rgba_frame_f16 *frame);
CVS_EXPORT void video_get_frame_f32_gl(video_source *source, int frame_index, rgba_frame_f32 *frame);
/* device twin: fills a device frame through slot 3 when the source has one, else pulls a host
 * frame and uploads it */
CVS_EXPORT void video_get_frame_dev(video_source *source, int frame_index, rgba_frame_dev *frame);

/* src/cprocess/video_mix.c:27-44, 73-105, 107-235, 46-71, 237-370 */
CVS_EXPORT void video_copy_frame_f16(rgba_frame_f16 *out, rgba_frame_f16 *in);
CVS_EXPORT void video_copy_frame_alpha_f32(rgba_frame_f32 *out, rgba_frame_f32 *in, float alpha);
/* include/framework.h:236 declares video_attenuate_f32 and no reference source defines it; here it is the in-place
 * case of video_copy_frame_alpha_f32 (video_mix.c:73-105 with out == in): alpha 1 leaves the frame alone, alpha 0
 * empties its window, anything between multiplies the alpha channel over the current window. */
CVS_EXPORT void video_attenuate_f32(rgba_frame_f32 *frame, float alpha);
CVS_EXPORT void video_mix_cross_f32(rgba_frame_f32 *out, rgba_frame_f32 *a, rgba_frame_f32 *b, float mix_b);
CVS_EXPORT void video_mix_cross_f32_pull(rgba_frame_f32 *out, video_source *a, int frame_a, video_source *b, int frame_b, float mix_b);
CVS_EXPORT void video_mix_over_f32(rgba_frame_f32 *out, rgba_frame_f32 *b, float mix_b);

/* src/cprocess/video_scale.c:231-286, 288-319 */
CVS_EXPORT void video_scale_bilinear_f32(rgba_frame_f32 *target, v2f target_point, rgba_frame_f32 *source, v2f source_point, v2f factors);
CVS_EXPORT void video_scale_bilinear_f32_pull(rgba_frame_f32 *target, v2f target_point, video_source *source, int frame,
                                              box2i *source_rect, v2f source_point, v2f factors);

/* src/cprocess/gammatab.c:83-110, 128-159, 171-198, 223-250, 13-38 */
CVS_EXPORT void video_transfer_rec709_to_linear_scene(half *out, const half *in, size_t count);
CVS_EXPORT void video_transfer_rec709_to_linear_display(half *out, const half *in, size_t count);
CVS_EXPORT void video_transfer_linear_to_rec709(half *out, const half *in, size_t count);
CVS_EXPORT void video_transfer_linear_to_sRGB(half *out, const half *in, size_t count);
CVS_EXPORT const uint8_t *video_get_gamma45_ramp(void);

/* src/cprocess/color.c:104-137, 140-165 (exported there, missing from framework.h) */
CVS_EXPORT void video_color_rgb_to_xyz_sdtv(rgba_frame_f16 *frame);
CVS_EXPORT void video_color_xyz_to_srgb(rgba_frame_f16 *frame);

/* src/cprocess/filter.c:24-76, 78-148, 150-153 */
CVS_EXPORT void filter_createTriangle(float sub, float offset, fir_filter *filter);
CVS_EXPORT void filter_createLanczos(float sub, int kernel_size, float offset, fir_filter *filter);
CVS_EXPORT void filter_free(fir_filter *filter);

/* src/cprocess/video_filter.c:27-39 + src/cprocess/gl.c:584 -- the reference only has this as a
 * GLSL program (video_filter_gain_offset_gl); same formula and window rule, f16 frames */
CVS_EXPORT void video_filter_gain_offset_f16(rgba_frame_f16 *out, rgba_frame_f16 *in, float gain, float offset);

/* src/process/SolidColorVideoSource.c:52-101 (the fill loops; parameter fetch stays with the caller) */
CVS_EXPORT void video_fill_solid_f16(rgba_frame_f16 *frame, const box2i *window, const rgba_f32 *color);
CVS_EXPORT void video_fill_solid_f32(rgba_frame_f32 *frame, const box2i *window, const rgba_f32 *color);

/* src/cprocess/workspace.c (video half): item bookkeeping :107-492, stack :494-550, source :604-613 */
typedef struct workspace_t_tag workspace_t;
typedef struct workspace_item_t_tag workspace_item_t;
CVS_EXPORT workspace_t *workspace_create(void);
CVS_EXPORT int workspace_get_length(workspace_t *workspace);
CVS_EXPORT workspace_item_t *workspace_add_item(workspace_t *self, void *source, int64_t x, int64_t width, int64_t offset, int64_t z, void *tag);
CVS_EXPORT workspace_item_t *workspace_get_item(workspace_t *self, int index);
CVS_EXPORT void workspace_remove_item(workspace_item_t *item);
CVS_EXPORT void workspace_as_video_source(workspace_t *workspace, video_source *source);
CVS_EXPORT void workspace_free(workspace_t *workspace);
CVS_EXPORT void workspace_get_item_pos(workspace_item_t *item, int64_t *x, int64_t *width, int64_t *z);
CVS_EXPORT int64_t workspace_get_item_offset(workspace_item_t *item);
CVS_EXPORT void workspace_set_item_offset(workspace_item_t *item, int64_t offset);
CVS_EXPORT void *workspace_get_item_source(workspace_item_t *item);
CVS_EXPORT void workspace_set_item_source(workspace_item_t *item, void *source);
CVS_EXPORT void *workspace_get_item_tag(workspace_item_t *item);
CVS_EXPORT void workspace_set_item_tag(workspace_item_t *item, void *tag);
CVS_EXPORT void workspace_update_item(workspace_item_t *item, int64_t *x, int64_t *width, int64_t *z, int64_t *offset, void **source, void **tag);

/* ------------------------------------------------------------------ (2) device runtime + device-frame twins */

typedef void *cvs_stream_t;            /* hipStream_t */

enum { CVS_LUT_NONE = -1, CVS_LUT_REC709_TO_LINEAR_SCENE = 0, CVS_LUT_REC709_TO_LINEAR_DISPLAY = 1,
       CVS_LUT_LINEAR_TO_REC709 = 2, CVS_LUT_LINEAR_TO_SRGB = 3, CVS_LUT_COUNT = 4 };

/* Arithmetic flavour.  The reference has two builds (SConstruct:46-48,75-83): gcc -std=c99, which rounds every multiply and
 * every add on its own, and clang -- preferred when it is installed -- which contracts a * b + c inside one expression into
 * a fused multiply-add: the matrix rows (src/cprocess/color.c:34-42), the blend numerators (src/cprocess/video_mix.c:193-205,
 * 323-337), every FIR accumulation t += s * coeff (src/cprocess/video_scale.c:82-85), the scaler's line centres (:65) and
 * intermediate window (:257-277), two of the transfer functions (src/cprocess/gammatab.c:58-66,201-211).
 *   CVS_ARITH_SEPARATE   (default)  bit-equal to the gcc build;
 *   CVS_ARITH_CONTRACTED            bit-equal to the clang build (half the FIR instructions: the faster of the two).
 * Process-wide; every entry point reads it once on entry, so change it between calls, not while other threads are inside the
 * library.  Tables that depend on it are cached per flavour.  The environment variable CVS_ARITHMETIC=contracted selects the
 * second flavour at start-up.  cvs_set_arithmetic returns the previous mode, or -1 for an unknown one (nothing changes). */
enum { CVS_ARITH_SEPARATE = 0, CVS_ARITH_CONTRACTED = 1 };
CVS_EXPORT int cvs_set_arithmetic(int mode);
CVS_EXPORT int cvs_get_arithmetic(void);

CVS_EXPORT int cvs_init(int device);                   /* 0 on success; idempotent per device */
CVS_EXPORT int cvs_device_count(void);
CVS_EXPORT int cvs_current_device(void);               /* HIP device of the calling thread's context, -1 before any */

/* Device contexts: several GPUs in one process.  A context is one HIP device plus everything the library keeps on it (scratch
 * pool, cached transfer / tap / byte tables, one stream per calling thread).  cvs_init(device) opens -- or finds -- a context
 * on `device` and makes it the DEFAULT: what every thread runs in that never chose another (and all a single-GPU host ever
 * needs).  cvs_context_open(device) opens a further one, on another GPU of the node or on the same one again (two contexts on
 * one device share nothing but the device); its id (0 .. 63) or -1.  cvs_set_context(ctx) binds the calling thread (-1: back to
 * the default) and returns what it was bound to (-2 for an unknown id, nothing changes).  Every entry point runs in the calling
 * thread's context; frames, streams and events belong to the context (device) they were created in.
 * Frames are independent random-access units (docs/sphinx/framework.rst:16-18): a host shards by giving frame g to context
 * cvs_frame_owner(g, n) -- one thread per context, as the reference's pull queue gives frames to its pool threads
 * (src/process/VideoPullQueue.c:99-113); the graph's parameters are host values and every context builds the device tables it
 * needs on first use.  Nothing is exchanged between devices. */
CVS_EXPORT int cvs_context_open(int device);
CVS_EXPORT int cvs_context_count(void);
CVS_EXPORT int cvs_context_device(int ctx);
CVS_EXPORT int cvs_set_context(int ctx);
CVS_EXPORT int cvs_current_context(void);
CVS_EXPORT int cvs_frame_owner(int64_t frame_index, int nowners);        /* frame_index mod nowners (non-negative); -1 for nowners <= 0 */
CVS_EXPORT const char *cvs_last_error(void);
CVS_EXPORT void cvs_clear_last_error(void);                                           /* forget the calling thread's message */
/* Diagnostics: every failure message (the text of cvs_last_error) is also handed to the installed handler, or written to
 * stderr when there is none.  The handler may be called from any thread that calls into the library.  The reference
 * logs through g_log in per-file domains (e.g. src/cprocess/video_reconstruct.c:23-24); here the domain is always
 * "fluggo.media.cprocess". */
enum { CVS_LOG_ERROR = 0, CVS_LOG_WARNING = 1, CVS_LOG_INFO = 2 };
typedef void (*cvs_log_func)(const char *domain, int level, const char *message, void *user_data);
CVS_EXPORT void cvs_set_log_handler(cvs_log_func handler, void *user_data);           /* thread-local, "" when none */
CVS_EXPORT const char *cvs_device_name(void);
CVS_EXPORT int cvs_compute_units(void);

CVS_EXPORT void *cvs_malloc(size_t bytes);
CVS_EXPORT void cvs_free(void *dev);
/* recycled scratch for per-frame intermediates (no device sync on free, unlike hipFree); a block
 * handed to a different stream than it was last used on waits for that stream first */
/* HIP graphs: record a sequence of device-frame calls on a stream once, replay it with one submission (worth it when
 * the sequence is launch-bound: many short kernels on small frames).  The contract, which tests/test_graph_replay_gpu.py holds
 * every cvs_*_dev entry of this header and the workspace's device slot to (tests/test_scope_harness_gpu.py holds
 * the entries of canvas_scope.h to it with the same code):
 *   - capturing thread = calling thread, one capture per thread at a time; between begin and end only `cvs_*_dev` entry points
 *     (and video_get_frame_dev over sources whose device slots make such calls) on the capturing stream.  A call that names
 *     another stream, or none, is not recorded: it runs at once.
 *   - the same sequence must have run once before on the same geometry (tables, pool blocks, code objects exist: recording then
 *     allocates nothing and waits for nothing).
 *   - recording runs nothing.  Return codes and current windows are those of the direct call and are final when the call
 *     returns; a call that refuses records nothing.  Frame pointers, windows and parameters are baked in (host arrays such as
 *     taps and matrices are read while recording and may go away); frame CONTENTS are read at replay time.
 *   - scratch blocks the sequence took from the pool, and the cached tap and byte tables its kernels read, stay with the graph
 *     until cvs_graph_destroy: at most 64 blocks and 64 table holds per graph (a call pinned to the table kernels holds two tap
 *     tables).  A capture that needs more fails at cvs_graph_end -- NULL, "too many scratch blocks or cached tables" -- with
 *     every block back in the pool and every hold released; the thread can record again at once.  A table held by a graph is
 *     never evicted: with all 8 byte-table slots, or all 128 tap-table slots, of a context held by graphs, a call that needs
 *     another table fails with a message and writes nothing.
 *   - cvs_graph_end returns NULL (message in cvs_last_error) and leaves the thread not capturing on every failure.
 *   - a graph belongs to the device context it was recorded in.  cvs_graph_launch and cvs_graph_destroy may be called by a
 *     thread bound to another context: they act in the graph's context (its device, its pool; a NULL stream is the calling
 *     thread's own stream THERE) and leave the caller bound as it was.  cvs_graph_destroy waits for the graph's device first. */
typedef void *cvs_graph_t;
CVS_EXPORT int cvs_graph_begin(cvs_stream_t stream);
CVS_EXPORT cvs_graph_t cvs_graph_end(cvs_stream_t stream);          /* NULL on failure */
CVS_EXPORT int cvs_graph_launch(cvs_graph_t graph, cvs_stream_t stream);
CVS_EXPORT void cvs_graph_destroy(cvs_graph_t graph);
CVS_EXPORT int cvs_mem_info(size_t *free_bytes, size_t *total_bytes);     /* HBM free / total on the bound device */
CVS_EXPORT void *cvs_pool_malloc(size_t bytes, cvs_stream_t s);
CVS_EXPORT void cvs_pool_free(void *dev, cvs_stream_t s);
CVS_EXPORT void cvs_pool_trim(void);
/* for a thread that is about to end: waits for what it queued and destroys the stream it was lent in each context */
CVS_EXPORT void cvs_thread_release(void);
CVS_EXPORT int cvs_memcpy_h2d(void *dev, const void *host, size_t bytes, cvs_stream_t s);
CVS_EXPORT int cvs_memcpy_d2h(void *host, const void *dev, size_t bytes, cvs_stream_t s);
CVS_EXPORT int cvs_memcpy_d2d(void *dst, const void *src, size_t bytes, cvs_stream_t s);
CVS_EXPORT int cvs_memset(void *dev, int value, size_t bytes, cvs_stream_t s);
CVS_EXPORT cvs_stream_t cvs_stream_create(void);
CVS_EXPORT void cvs_stream_destroy(cvs_stream_t s);
CVS_EXPORT int cvs_stream_sync(cvs_stream_t s);
/* HIP events on a stream, for callers that time kernels without linking HIP themselves */
typedef void *cvs_event_t;
CVS_EXPORT cvs_event_t cvs_event_create(void);
CVS_EXPORT void cvs_event_destroy(cvs_event_t e);
CVS_EXPORT int cvs_event_record(cvs_event_t e, cvs_stream_t s);
CVS_EXPORT int cvs_event_sync(cvs_event_t e);
CVS_EXPORT float cvs_event_elapsed_ms(cvs_event_t start, cvs_event_t stop);   /* < 0 on error */

/* the four transfer tables, resident in HBM after first use (128 KiB each); host copy for callers
 * that want to ship them elsewhere (multi-GPU parameter broadcast) */
CVS_EXPORT const half *cvs_lut_device(int which);
CVS_EXPORT const half *cvs_lut_host(int which);
/* install a table built elsewhere (rank 0 broadcasts, the others install); 65536 entries */
CVS_EXPORT int cvs_lut_install(int which, const half *table_host);

/* flat arrays in HBM */
CVS_EXPORT int cvs_half_to_float_dev(float *out, const half *in, size_t count, cvs_stream_t s);
CVS_EXPORT int cvs_float_to_half_dev(half *out, const float *in, size_t count, cvs_stream_t s);
CVS_EXPORT int cvs_half_to_float_fast_dev(float *out, const half *in, size_t count, cvs_stream_t s);
CVS_EXPORT int cvs_float_to_half_fast_dev(half *out, const float *in, size_t count, cvs_stream_t s);
CVS_EXPORT int cvs_half_lookup_dev(const half *table_dev, half *out, const half *in, size_t count, cvs_stream_t s);

/* frames in HBM (frame->data is a device pointer); window logic runs on the host exactly as in
 * the reference and the structs are updated before the call returns; pixels are enqueued on `s` */

/* Operands that share a buffer (DESIGN.md "Operands that share a buffer"; tests/alias_cases.py holds this block to the library).
 * Frames are the caller's device pointers, so one buffer can be handed to a device entry twice.  Two frame operands SHARE A
 * BUFFER when their `data` pointers are equal and their `full_window`s are equal: one struct handed in for both parameters,
 * or two structs (whatever their `current_window`s).  For every pair of frame operands of every cvs_*_dev entry -- a frame the
 * entry writes against one it reads, or two it reads -- exactly one of three things holds, whatever path, kernel or
 * cvs_fir_path_override() pin takes the call; the lists name the entry and its pairs by their parameters (a table of frame
 * pointers pairs with itself; a cvs_chain_job is its `out` and its `layers`), those of the extension headers included:
 *   - IN PLACE: the entry computes, bit for bit, windows included, what the same call gives on a distinct copy of the input.
 *   - REFUSED: the entry returns nonzero before any device call, table look-up or pool allocation; cvs_last_error() names the
 *     entry and says "the target is the source's buffer: the operation is not in place" or "the output cannot be one of the
 *     inputs"; the written frame's current_window is empty; no buffer is touched.  A batch refuses as a whole, with every
 *     target's window empty, when any frame's target is that frame's source.
 *   - SHARED: both operands are only read, and may be one buffer.
 * An entry never returns 0 with pixels that differ from the out-of-place call.  Not covered, and the caller's error wherever
 * an entry's own text does not say otherwise (the chain, the scaler batches): equal `data` under different `full_window`s,
 * buffers that overlap at a shifted address, and two operands that are both written.
 *   in place:
 *     cvs_half_lookup_dev (out, in); cvs_copy_frame_f16_dev (out, in); cvs_copy_frame_alpha_f32_dev (out, in);
 *     cvs_gain_offset_f16_dev (out, in); cvs_color_matrix_f16_to_dev (out, in);
 *     cvs_mix_cross_f32_dev (out, a) (out, b); cvs_mix_over_f32_dev (out, b); cvs_mix_cross_f16_dev (out, a) (out, b);
 *     cvs_chain_color_over_f16_dev (out, layers); cvs_chroma_key_f16_dev (target, source); cvs_chroma_key_f32_dev (target, source);
 *     cvs_lut3d_f16_dev (target, source); cvs_lut3d_f32_dev (target, source);
 *     cvs_blur_over_f16_dev (out, overlays); cvs_blur_over_f16_batch_dev (outs, overlays)
 *   refused:
 *     cvs_weave_fields_f16_dev (frame, other); cvs_field_to_frame_f16_dev (out, in); cvs_soften_fields_f16_dev (out, in);
 *     cvs_interlace_fields_f16_dev (out, even) (out, odd);
 *     cvs_matte_refine_f16_dev (target, source); cvs_matte_refine_f32_dev (target, source);
 *     cvs_transform_f16_dev (target, source); cvs_transform_f32_dev (target, source);
 *     cvs_perspective_f16_dev (target, source); cvs_perspective_f32_dev (target, source);
 *     cvs_deinterlace_adaptive_f16_dev (out, prev) (out, cur) (out, next);
 *     cvs_fir_blur_f32_dev (target, source); cvs_fir_blur_f16_dev (target, source);
 *     cvs_unsharp_mask_f32_dev (target, source); cvs_unsharp_mask_f16_dev (target, source);
 *     cvs_resample_lanczos_f32_dev (target, source); cvs_resample_lanczos_f16_dev (target, source);
 *     cvs_scale_bilinear_f32_dev (target, source); cvs_scale_bilinear_f16_dev (target, source);
 *     cvs_scale_bilinear_f32_batch_dev (targets, sources); cvs_scale_bilinear_f16_batch_dev (targets, sources);
 *     cvs_blur_lanczos_f16_dev (target, source); cvs_blur_lanczos_f16_batch_dev (targets, sources);
 *     cvs_blur_over_f16_dev (out, source); cvs_blur_over_f16_batch_dev (outs, sources)
 *   shared:
 *     cvs_mix_cross_f32_dev (a, b); cvs_mix_cross_f16_dev (a, b); cvs_chain_color_over_f16_dev (layers, layers);
 *     cvs_interlace_fields_f16_dev (even, odd); cvs_deinterlace_adaptive_f16_dev (prev, cur) (prev, next) (cur, next);
 *     cvs_scale_bilinear_f32_batch_dev (sources, sources); cvs_scale_bilinear_f16_batch_dev (sources, sources);
 *     cvs_blur_lanczos_f16_batch_dev (sources, sources); cvs_blur_over_f16_dev (source, overlays) (overlays, overlays);
 *     cvs_blur_over_f16_batch_dev (sources, sources) (sources, overlays) (overlays, overlays)
 * Every other device entry takes one frame, or frames against operands of another type. */
CVS_EXPORT int cvs_frame_f16_to_f32_dev(rgba_frame_f32 *out, const rgba_frame_f16 *in, cvs_stream_t s);   /* main.c:115-139 */
CVS_EXPORT int cvs_frame_f32_to_f16_dev(rgba_frame_f16 *out, const rgba_frame_f32 *in, cvs_stream_t s);   /* main.c:43-71 */
CVS_EXPORT int cvs_copy_frame_f16_dev(rgba_frame_f16 *out, const rgba_frame_f16 *in, cvs_stream_t s);
CVS_EXPORT int cvs_copy_frame_alpha_f32_dev(rgba_frame_f32 *out, const rgba_frame_f32 *in, float alpha, cvs_stream_t s);
CVS_EXPORT int cvs_mix_cross_f32_dev(rgba_frame_f32 *out, const rgba_frame_f32 *a, const rgba_frame_f32 *b, float mix_b, cvs_stream_t s);
CVS_EXPORT int cvs_mix_over_f32_dev(rgba_frame_f32 *out, const rgba_frame_f32 *b, float mix_b, cvs_stream_t s);
/* colour matrix with the color.c structure; m is column-major as color.c passes it:
 * m[0..2] = coefficients multiplying r (a.x a.y a.z), m[3..5] those of g, m[6..8] those of b */
CVS_EXPORT int cvs_color_matrix_f16_dev(rgba_frame_f16 *frame, const float m[9], int pre_lut, int post_lut, cvs_stream_t s);
/* the same filter, out of place: out.current = out.full ∩ in.current, one pass */
CVS_EXPORT int cvs_color_matrix_f16_to_dev(rgba_frame_f16 *out, const rgba_frame_f16 *in, const float m[9], int pre_lut, int post_lut, cvs_stream_t s);
CVS_EXPORT int cvs_gain_offset_f16_dev(rgba_frame_f16 *out, const rgba_frame_f16 *in, float gain, float offset, cvs_stream_t s);
CVS_EXPORT int cvs_fill_solid_f16_dev(rgba_frame_f16 *frame, const box2i *window, const rgba_f32 *color, cvs_stream_t s);
CVS_EXPORT int cvs_fill_solid_f32_dev(rgba_frame_f32 *frame, const box2i *window, const rgba_f32 *color, cvs_stream_t s);
/* the f16 twin: widen on load, truncate on store (the f16 pull of a scaler node over a half-native source) */
CVS_EXPORT int cvs_scale_bilinear_f16_dev(rgba_frame_f16 *target, v2f tp, const rgba_frame_f16 *source, v2f sp, v2f fac, cvs_stream_t stream);
/* The two device entries of the scaler for `count` INDEPENDENT frames (a pull queue's frames in flight): frames of one geometry
 * whose buffers do not overlap go up to eight at a time into one launch where the tile kernel takes the call (vertical pass
 * first -- video_scale.c:252 -- and short tap lists: enlarging; 1080p -> 4K: 0.0173 -> see DESIGN.md 4.4 per frame); every
 * other combination is carried out frame by frame, exactly as `count` single calls.  Results are those of the single calls,
 * bit for bit; a NULL entry or a source window outside its buffer refuses the whole call before any launch. */
CVS_EXPORT int cvs_scale_bilinear_f32_batch_dev(rgba_frame_f32 *const *targets, v2f target_point, const rgba_frame_f32 *const *sources, v2f source_point,
                                                v2f factors, int count, cvs_stream_t stream);
CVS_EXPORT int cvs_scale_bilinear_f16_batch_dev(rgba_frame_f16 *const *targets, v2f target_point, const rgba_frame_f16 *const *sources, v2f source_point,
                                                v2f factors, int count, cvs_stream_t stream);
CVS_EXPORT int cvs_scale_bilinear_f32_dev(rgba_frame_f32 *target, v2f target_point, const rgba_frame_f32 *source, v2f source_point, v2f factors, cvs_stream_t s);
/* separable FIR blur at factor 1 (absent from the reference; defined in DESIGN.md) and the Lanczos
 * gather resampler built on filter_createLanczos */
CVS_EXPORT int cvs_fir_blur_f32_dev(rgba_frame_f32 *target, const rgba_frame_f32 *source, const float *taps_host, int ntaps, cvs_stream_t s);
/* DV 4:1:1 edge: planar 8-bit Y'CbCr (Y 720x480, Cb and Cr 180x480) <-> half RGBA on the fixed NTSC DV raster
 * whose first line sits at y = -1.  coded_image: include/framework.h:468-476; alloc: video_subsample.c:23-68. */
#define CODED_IMAGE_MAX_PLANES 4
typedef struct {
    void *data[CODED_IMAGE_MAX_PLANES];
    int stride[CODED_IMAGE_MAX_PLANES];
    int line_count[CODED_IMAGE_MAX_PLANES];
    void (*free_func)(void *image);          /* GFreeFunc */
} coded_image;
CVS_EXPORT coded_image *coded_image_alloc(const int *strides, const int *line_counts, int count);
CVS_EXPORT coded_image *coded_image_alloc0(const int *strides, const int *line_counts, int count);
CVS_EXPORT void video_reconstruct_dv(rgba_frame_f16 *frame, coded_image *planar);       /* video_reconstruct.c:50-137 */
CVS_EXPORT coded_image *video_subsample_dv(rgba_frame_f16 *frame);                      /* video_subsample.c:99-187; encodes the frame's rows in place, as there */
/* device frame + device planes (planar->data[] are device pointers) */
CVS_EXPORT int cvs_reconstruct_dv_dev(rgba_frame_f16 *frame, const coded_image *planar, cvs_stream_t stream);
CVS_EXPORT int cvs_subsample_dv_dev(coded_image *planar, rgba_frame_f16 *frame, int encode_input_in_place, cvs_stream_t stream);
/* MPEG-2 4:2:0 edge, interlaced chroma siting (video_subsample.c:189-526, video_subsample_mpeg2_gl: GLSL only in the reference;
 * the contract, rounding included, is DESIGN.md "MPEG-2 4:2:0 subsample").  Planar 8-bit Y'CbCr: Y' width x height, Cb and Cr
 * width/2 x height/2, raster origin at frame (0, 0); pixels outside the current window encode as black; Rec.601 matrix as the
 * reference uses it (:405-410); the caller's frame is only read.  width even >= 2, height a multiple of 4 >= 4, else -1.
 * video_subsample_mpeg2: host frame, the reference's 720x480, planes allocated as video_subsample_dv's; NULL on failure.
 * cvs_subsample_mpeg2_dev: device planes (strides and line counts at least the raster's) and device frame; 0 on success. */
CVS_EXPORT coded_image *video_subsample_mpeg2(rgba_frame_f16 *frame);
CVS_EXPORT int cvs_subsample_mpeg2_dev(coded_image *planar, const rgba_frame_f16 *frame, int width, int height, cvs_stream_t stream);
/* MPEG-2 4:2:0 import edge: planar 8-bit Y'CbCr -> half RGBA, the way in for the 4:2:0 images a decoder hands out (no reference
 * code: its libav decoder produces them, src/libav/AVVideoDecoder.c:75-97, and nothing turns them into frames; the contract,
 * rounding included, is DESIGN.md "MPEG-2 4:2:0 reconstruction").  Planes: Y' width x height, Cb and Cr width/2 x height/2;
 * strides and line counts may exceed the raster.  The raster's origin is frame (0, 0): current_window = full_window clipped to
 * [0, width-1] x [0, height-1], and only those pixels are written (those outside keep what they held); an empty intersection
 * is not an error (0, empty window).  Per pixel: studio-range decode by correctly rounded division (video_reconstruct.c:32-39),
 * chroma interpolated vertically by the siting in `flags` and horizontally between even-column samples, the matrix evaluated as
 * video_reconstruct.c:114-122 does with every product and sum rounded on its own in both arithmetic flavours, truncation to
 * half and the Rec.709 -> linear (scene) table over all four halfs (the separate flavour's table in both).
 * flags: 0 = interlaced siting (the exact inverse of cvs_subsample_mpeg2_dev's) and the Rec.601 matrix (video_reconstruct.c:
 * 55-59); CVS_YCC_PROGRESSIVE: MPEG-2 progressive / H.264 siting (chroma between luma rows 2c and 2c+1); CVS_YCC_REC709: the
 * Rec.709 matrix (:62-66).  Interlaced needs width even >= 2 and height a multiple of 4 >= 4, progressive width even >= 2 and
 * height even >= 2; other sizes, other flag bits, missing or short planes: cvs_set_error, -1 and an empty current_window.
 * cvs_reconstruct_mpeg2_dev: device planes (planar->data[] are device pointers) and device frame; 0 on success.
 * video_reconstruct_mpeg2: host frame and host planes, 720x480, interlaced, Rec.601; on failure an empty current_window. */
enum { CVS_YCC_PROGRESSIVE = 1, CVS_YCC_REC709 = 2 };
CVS_EXPORT int cvs_reconstruct_mpeg2_dev(rgba_frame_f16 *frame, const coded_image *planar, int width, int height, int flags, cvs_stream_t stream);
CVS_EXPORT void video_reconstruct_mpeg2(rgba_frame_f16 *frame, coded_image *planar);

/* 2:3 pulldown removal (src/process/Pulldown23RemovalFilter.c:43-107; the reference keeps this inside the Python
 * node, the arithmetic and the field weave are entry points here so that the node is a thin caller).
 * cvs_pulldown23_frames: output frame -> source frame(s) for cadence phase `offset` (:51-71); returns 1 when the
 *   frame is woven from two (odd rows from *first, even rows from *second), else 0 and *first alone.
 * cvs_weave_fields_f16_dev: :88-104 on device frames -- `other` must be allocated for exactly frame->current_window,
 *   as the reference allocates it; the even rows (first even y >= min.y) of the frame are replaced.  The reference
 *   addresses the second buffer from x = 0 instead of min.x (:101); inside the allocation that shift is reproduced,
 *   outside it (and outside other->current_window, uninitialised in the reference) the pixel is zero. */
CVS_EXPORT int cvs_pulldown23_frames(int offset, int frame_index, int *first, int *second);
CVS_EXPORT int cvs_weave_fields_f16_dev(rgba_frame_f16 *frame, const rgba_frame_f16 *other, cvs_stream_t stream);

/* Field conversions: between woven (interlaced) frames -- field 1 on the even rows, field 2 on the odd rows, upper field first
 * (fluggo/editor/plugins/_source.py:125-126) -- and whole pictures.  No reference code (the design lists the conversions,
 * docs/sphinx/feature-proposal/canvas.rst:283-303, and the editor names them, fluggo/editor/model/sources.py:536-542); the
 * contract, rounding included, is DESIGN.md "Field conversions" and what follows.
 * All three device entries: f16 device frames; 0 on success, -1 with a message in cvs_last_error on failure, and
 * out->current_window is set on every path (empty on failure).  The inputs are only read; `out` may not share its buffer with an
 * input; an input whose current_window lies outside its full_window is refused.  Windows are arbitrary (negative coordinates,
 * full windows larger than current windows); pixels of `out` outside its new current_window keep what they held.  Row parity
 * is that of the absolute coordinate: y & 1 in two's complement, so row -1 is odd.  All four channels are treated alike (alpha
 * is filtered as a channel, nothing is premultiplied: what video_scale.c does).  Arithmetic is f32 on exactly widened halfs, the
 * result truncated to half as everywhere (half.c:47-51).  Every product is by 0.5 or 0.25 and exact for every finite half, so
 * CVS_ARITH_SEPARATE and CVS_ARITH_CONTRACTED give the same bits: these entries do not depend on cvs_set_arithmetic.
 *
 * cvs_field_to_frame_f16_dev: one field made into a whole picture (bob and discard-a-field deinterlacing).  field: 0 = the even
 *   rows, 1 = the odd rows, anything else is an error.  current_window = out->full_window ∩ in->current_window.  Rows of it with
 *   (y & 1) == field are copied code for code.  Every other row is made from rows y - 1 and y + 1 of `in`, each used if it lies
 *   inside in->current_window (whether or not inside out->full_window): both -- t = upper * 0.5f; u = lower * 0.5f; r = t + u
 *   (one rounding); one -- that row's codes; none (a one-row window of the other parity) -- four zero halfs.
 * cvs_soften_fields_f16_dev: vertical [1/4, 1/2, 1/4], so that one-row detail of a progressive picture does not flicker at field
 *   rate once the frame is shown interlaced (the design's "weave interlace").  Same window rule.  With a, b, c rows y - 1, y,
 *   y + 1 of `in`: t = a * 0.25f; t = t + b * 0.5f; t = t + c * 0.25f (two roundings); a neighbour outside in->current_window is
 *   replaced by row y itself.
 * cvs_interlace_fields_f16_dev: two pictures woven into one frame (bob interlacing, 2:3 pulldown addition).  current_window =
 *   out->full_window ∩ the bounding box of the inputs' non-empty current windows (empty when both are).  Even rows come from
 *   `even`, odd rows from `odd`, code for code; a pixel outside the providing frame's current_window is four zero halfs.  `even`
 *   and `odd` may be the same frame.  Unlike cvs_weave_fields_f16_dev nothing is asked of how the inputs were allocated and
 *   there is no x = 0 addressing quirk.
 * cvs_pulldown23_add_frames: host arithmetic, the inverse of cvs_pulldown23_frames: output frame `frame_index` of a 2:3 cadence
 *   with phase `offset` (0..4) takes its even rows from source frame *even_source and its odd rows from *odd_source.  Returns 1
 *   when the two differ, 0 when they are the same frame, -1 (nothing written) for an offset outside 0..4.  Cadence AA BB BC CD DD
 *   (Pulldown23RemovalFilter.c:56-60): add0(i) = 4 * floor(i / 5) + ([0, 1, 1, 2, 3], [0, 1, 2, 3, 3])[i mod 5], and
 *   add(offset, i) = add0(i + offset) - [0, 1, 2, 3, 3][offset]; negative frame indices continue the cadence backwards. */
CVS_EXPORT int cvs_field_to_frame_f16_dev(rgba_frame_f16 *out, const rgba_frame_f16 *in, int field, cvs_stream_t stream);
CVS_EXPORT int cvs_soften_fields_f16_dev(rgba_frame_f16 *out, const rgba_frame_f16 *in, cvs_stream_t stream);
CVS_EXPORT int cvs_interlace_fields_f16_dev(rgba_frame_f16 *out, const rgba_frame_f16 *even, const rgba_frame_f16 *odd, cvs_stream_t stream);
CVS_EXPORT int cvs_pulldown23_add_frames(int offset, int frame_index, int *even_source, int *odd_source);

/* Display / export edge: the current window of an f16 frame as 4 bytes per pixel, packed row by row.
 * pre_lut: a transfer table applied to all four halfs first (CVS_LUT_NONE for none); then a half->u8 ramp.
 *
 * cvs_frame_to_bytes_dev / video_frame_to_bytes use the gamma-0.45 ramp of video_get_gamma45_ramp():
 *   CVS_DISPLAY_RGBA8: bytes r,g,b,a -- with CVS_LUT_NONE the exporter's conversion (src/libav/writeVideo.c:328-340,
 *     whose own ramp at :108-115 holds the same bytes).
 *   CVS_DISPLAY_ARGB32_PREMUL: a<<24 | (r*a>>8)<<16 | (g*a>>8)<<8 | (b*a>>8), what RgbaFrameF16.to_argb32_bytes
 *     returns (src/process/RgbaFrameF16.c:114-149).
 * cvs_frame_to_rgba8_intent_dev / video_frame_to_rgba8_intent use the software widget's ramp,
 *   lrint(clamp(x^rendering_intent * 255, 0, 255)) (src/cprocess/widget_gl.c:955-968): with CVS_LUT_LINEAR_TO_SRGB
 *   and the widget's default intent 1.25 (:428-429) they are its frame conversion (:291-307), bytes r,g,b,a. */
enum { CVS_DISPLAY_RGBA8 = 0, CVS_DISPLAY_ARGB32_PREMUL = 1 };
CVS_EXPORT int cvs_frame_to_bytes_dev(void *dst_dev, const rgba_frame_f16 *frame, int pre_lut, int mode, cvs_stream_t stream);
CVS_EXPORT int video_frame_to_bytes(void *dst_host, const rgba_frame_f16 *host_frame, int pre_lut, int mode);
CVS_EXPORT int cvs_frame_to_rgba8_intent_dev(void *dst_dev, const rgba_frame_f16 *frame, int pre_lut, float rendering_intent, cvs_stream_t stream);
CVS_EXPORT int video_frame_to_rgba8_intent(void *dst_host, const rgba_frame_f16 *host_frame, int pre_lut, float rendering_intent);

/* blur node between two f16 frames (widen on load, f32 passes, truncate on store), one launch */
CVS_EXPORT int cvs_fir_blur_f16_dev(rgba_frame_f16 *target, const rgba_frame_f16 *source, const float *taps, int ntaps, cvs_stream_t stream);
/* Unsharp mask (DESIGN.md "Unsharp mask").  B = the blur of `source` exactly as cvs_fir_blur_*_dev computes it (same window:
 * source.current_window clipped to target.full_window; same sums, in the arithmetic flavour in force).  Then per pixel of that
 * window, in f32, every operation rounded on its own in both flavours:
 *     for c in r, g, b:  d = s.c - B.c;  out.c = fabsf(d) < threshold ? s.c : s.c + amount * d;      out.a = s.a
 * (a NaN d takes the sharpening branch; amount 0 returns the source's colours; threshold <= 0 sharpens everywhere).  f16 targets
 * are truncated at the store, once.  Windows, refusals and return values as the blur entries'.  Odd lists of 3..13 finite taps
 * run as ONE launch without an intermediate frame (cvs_fir_last_kernel() == CVS_FIR_KERNEL_UNSHARP -- the tap list decides,
 * so also for a call whose window holds no pixel and that launches nothing); every other list as the
 * blur into a pooled f32 frame followed by the mask, with the same result wherever both can run.  Not in place. */
CVS_EXPORT int cvs_unsharp_mask_f32_dev(rgba_frame_f32 *target, const rgba_frame_f32 *source, const float *taps, int ntaps, float amount, float threshold, cvs_stream_t s);
CVS_EXPORT int cvs_unsharp_mask_f16_dev(rgba_frame_f16 *target, const rgba_frame_f16 *source, const float *taps, int ntaps, float amount, float threshold, cvs_stream_t s);
/* Chroma key (DESIGN.md "Chroma key"): alpha from a picture's distance to a key colour in the Pb, Pr plane, with spill
 * suppression.  Frames are un-premultiplied, so the key scales alpha and leaves colour alone but for the despill; the over
 * entries then composite the result as it is.  win = source.current_window ∩ target.full_window; on success
 * target.current_window = win (0 is returned for an empty one too), pixels of `target` outside it keep what they held.  -1 with
 * a message and an empty target window for a NULL pointer, a source window outside its full window, a non-finite key[], a
 * non-finite or negative tolerance, softness or spill_range, and a failed launch.  `target` may be the source frame itself.
 * Per pixel s of win, in f32 (a half widened exactly), every operation rounded on its own in both arithmetic flavours, with
 * the Rec.709 R'G'B' -> Y'PbPr rows c0 = 0.2126f, 0.7152f, 0.0722f; c1 = -0.114572f, -0.385428f, 0.5f; c2 = 0.5f, -0.454153f,
 * -0.045847f and kpb, kpr the key colour's pb, pr by the same expressions:
 *     pb = (s.r*c10 + s.g*c11) + s.b*c12 ;  pr = (s.r*c20 + s.g*c21) + s.b*c22
 *     dx = pb - kpb ; dy = pr - kpr ; d = sqrtf(dx*dx + dy*dy)                  (correctly rounded)
 *     ramp(t) = (t < 1) ? ((t > 0) ? t : 0) : 1                                   (NaN -> 1: such a pixel is kept)
 *     m = softness > 0 ? ramp((d - tolerance) * (1.0f / softness)) : (d <= tolerance ? 0 : 1) ;   a' = s.a * m
 *     spill > 0:  q = spill_range > 0 ? ramp((d - tolerance) * (1.0f / spill_range)) : (d <= tolerance ? 0 : 1)
 *                 ws = spill * (1 - q) ;  y = (s.r*c00 + s.g*c01) + s.b*c02 ;  for c in r, g, b:  e = y - s.c ; f = ws * e ; c' = s.c + f
 *     else        c' = s.c, code for code
 *     out = (flags & CVS_KEY_SHOW_MATTE) ? (a', a', a', 1) : (r', g', b', a')
 * f16 targets are truncated once, at the store. */
enum { CVS_KEY_SHOW_MATTE = 1 };
typedef struct cvs_chroma_key {
    float key[3];       /* the colour to remove, in the frame's own RGB */
    float tolerance;    /* chroma distance up to which a pixel is removed entirely */
    float softness;     /* width of the ramp from removed to kept beyond tolerance; 0 = hard edge */
    float spill;        /* strength of the spill suppression; clamped to [0, 1] by the entry */
    float spill_range;  /* distance beyond tolerance over which suppression fades to none; 0 = none beyond */
    int   flags;
} cvs_chroma_key;
CVS_EXPORT int cvs_chroma_key_f32_dev(rgba_frame_f32 *target, const rgba_frame_f32 *source, const cvs_chroma_key *key, cvs_stream_t s);
CVS_EXPORT int cvs_chroma_key_f16_dev(rgba_frame_f16 *target, const rgba_frame_f16 *source, const cvs_chroma_key *key, cvs_stream_t s);
/* Matte refine (DESIGN.md "Matte refine"): the three controls that follow a keyer -- clip (black and white levels on the
 * matte), choke (shrink or grow it by whole pixels) and feather (blur the matte only) -- on the alpha channel of un-premultiplied
 * frames, in one launch; colour is carried through code for code.  S = source.current_window, win = S clipped to
 * target.full_window; on success target.current_window = win (0 is returned for an empty one too, and nothing is launched), pixels
 * of `target` outside it keep what they held.  Every stage is defined over the whole of S and the output is its crop to win.
 * -1 with a message and an empty target window, before the device is touched, for: a NULL frame or a NULL `m`; a source window
 * outside its full window; |choke| > CVS_MATTE_MAX_CHOKE; ntaps < 0, even, or > CVS_MATTE_MAX_TAPS, ntaps > 0 with NULL taps, a
 * non-finite tap; non-finite black or white, or white <= black; a bit of flags other than CVS_MATTE_SHOW; target->data ==
 * source->data (the operation is not in place; partly overlapping buffers are the caller's error and are not detected).
 * Per pixel, in f32 (a half widened exactly), every operation rounded on its own in both arithmetic flavours, with r = |choke|,
 * c = (ntaps - 1) / 2 and inv = 1.0f / (white - black):
 *     a0 = s.a, a NaN alpha counting as 0
 *     a1 = (black == 0 && white == 1) ? a0 : ramp((a0 - black) * inv)         ramp(t) = (t < 1) ? ((t > 0) ? t : 0) : 1
 *     a2(x, y) = choke > 0 ? min : choke < 0 ? max : identity  of a1 over {(x+i, y+j) : |i| <= r, |j| <= r} clipped to S
 *                (samples outside S are skipped, not taken as transparent)
 *     h(x, y)  = t after: t = 0; for k = 0 .. ntaps-1: if (x+k-c, y) in S: p = a2(x+k-c, y) * taps[k]; t = t + p
 *     a3(x, y) = t after: t = 0; for k = 0 .. ntaps-1: if (x, y+k-c) in S: p = h(x, y+k-c) * taps[k]; t = t + p      (ntaps == 0: a2)
 *     out = (flags & CVS_MATTE_SHOW) ? (a3, a3, a3, 1) : (s.r, s.g, s.b, a3)
 * f16 targets are truncated once, at the store.  The sign of a zero that a minimum or maximum returns is not pinned. */
enum { CVS_MATTE_SHOW = 1 };
enum { CVS_MATTE_MAX_CHOKE = 16, CVS_MATTE_MAX_TAPS = 25 };
typedef struct cvs_matte {
    float black, white;   /* matte levels: alpha <= black -> 0, >= white -> 1; 0 and 1 switch the stage off */
    int   choke;          /* > 0 shrinks the matte (minimum over a square), < 0 grows it (maximum); |choke| <= 16 */
    int   ntaps;          /* feather: 0 = none, else an odd count 1..25 of finite taps, normalised by the caller */
    const float *taps;    /* host pointer */
    int   flags;
} cvs_matte;
CVS_EXPORT int cvs_matte_refine_f32_dev(rgba_frame_f32 *target, const rgba_frame_f32 *source, const cvs_matte *m, cvs_stream_t s);
CVS_EXPORT int cvs_matte_refine_f16_dev(rgba_frame_f16 *target, const rgba_frame_f16 *source, const cvs_matte *m, cvs_stream_t s);
/* Affine transform (DESIGN.md "Affine transform"): rotate, scale, mirror and move a layer of un-premultiplied pixels, the
 * bilinear and the Catmull-Rom filter weighted by alpha so that a layer's edge keeps its colour and only its alpha falls off.  Integer coordinates
 * are sample positions.  `m` maps TARGET coordinates to SOURCE coordinates.  S = source.current_window; the entry writes
 * win = cvs_transform_target_window(t, S, target.full_window) and sets target.current_window = win (0 is returned for an empty
 * one too, and nothing is launched); pixels of `target` outside win keep what they held.  The output is the crop of the
 * infinite-plane result to win.
 * -1 with a message and an empty target window, before the device is touched, for: a NULL frame or a NULL `t`; a source window
 * outside its full window; a filter other than the three; flags != 0; a non-finite m[k]; m0*m4 - m1*m3 (in double) zero or not
 * finite; a coordinate of S or of target.full_window beyond +-CVS_TRANSFORM_MAX_COORD (every coordinate is then an exact
 * float); target->data == source->data.
 * Per pixel, in f32 (a half widened exactly), every operation rounded on its own in both arithmetic flavours:
 *     x, y = (float) of the target pixel's coordinates
 *     u = (m0*x + m1*y) + m2 ;  v = (m3*x + m4*y) + m5
 *     in(i, j) = S.min.x <= i <= S.max.x and S.min.y <= j <= S.max.y, compared as floats (false for NaN and +-Inf)
 *     NEAREST:   i = floorf(u + 0.5f), j = floorf(v + 0.5f);  out = in(i, j) ? source(i, j) code for code : (0, 0, 0, 0)
 *     BILINEAR:  i = floorf(u), j = floorf(v);  a = u - i;  b = v - j;  wa = 1 - a;  wb = 1 - b
 *                a == 0 and b == 0 (on a sample):  out = in(i, j) ? source(i, j) code for code : (0, 0, 0, 0)
 *                else A = R = G = B = 0;  for (w, di, dj) in (wa*wb, 0, 0), (a*wb, 1, 0), (wa*b, 0, 1), (a*b, 1, 1), in this order:
 *                         if in(i + di, j + dj):  p = source(i + di, j + dj);  q = w * p.a;  A = A + q;
 *                                                 R = R + q*p.r;  G = G + q*p.g;  B = B + q*p.b
 *                     out = A != 0 ? (R / A, G / A, B / A, A) : (0, 0, 0, 0)
 *     CATMULL_ROM (DESIGN.md "Catmull-Rom warps"; the cubic that interpolates: on a sample it returns the sample):
 *                i = floorf(u), j = floorf(v);  a = u - i;  b = v - j
 *                weights of a fraction t (wx[0..3] from a, wy[0..3] from b), Horner, in this order:
 *                    w0 = ((-0.5f*t + 1.0f)*t - 0.5f)*t        w1 = ((1.5f*t - 2.5f)*t)*t + 1.0f
 *                    w2 = ((-1.5f*t + 2.0f)*t + 0.5f)*t        w3 = ((0.5f*t - 0.5f)*t)*t
 *                a == 0 and b == 0:  out = in(i, j) ? source(i, j) code for code : (0, 0, 0, 0)
 *                else A = R = G = B = 0;  lo_c = +inf, hi_c = -inf per colour channel;  lo_a = +inf, hi_a = -inf
 *                     for l in 0..3 (rows j-1+l), for k in 0..3 (columns i-1+k), in this order:
 *                         p = source(i-1+k, j-1+l) if in(...);  counts = in(...) and p.a > 0       (false for a NaN alpha)
 *                         if counts:  q = (wx[k]*wy[l]) * p.a;  A = A + q;  R = R + q*p.r;  G = G + q*p.g;  B = B + q*p.b
 *                                     lo_c = fmin(lo_c, p.c);  hi_c = fmax(hi_c, p.c)               per colour channel
 *                         ta = counts ? p.a : 0;  lo_a = fmin(lo_a, ta);  hi_a = fmax(hi_a, ta)      all 16 positions
 *                     out = A > 0 ? (clamp(R/A, lo_r, hi_r), clamp(G/A, ..), clamp(B/A, ..), clamp(A, lo_a, hi_a)) : (0, 0, 0, 0)
 *                     clamp(t, lo, hi) = fmin(fmax(t, lo), hi);  fmin / fmax: a NaN operand loses
 *                The clamp rule: the result never leaves the range of the 4 x 4 samples it was made from -- no negative light out
 *                of non-negative light, no alpha above the layer's own, an opaque interior stays opaque, a flat colour flat.
 * Taps outside S are skipped and never read.  f16 targets are truncated once, at the store (the copy paths move the code).  The
 * payload of a NaN is not pinned, nor the sign of a zero that a minimum or maximum of the clamp rule returns.  The value of
 * CVS_TRANSFORM_CATMULL_ROM is the filter's support in samples per axis (6 is left
 * for a Lanczos-3 filter); 2, 3 and every other value are refused. */
enum { CVS_TRANSFORM_NEAREST = 0, CVS_TRANSFORM_BILINEAR = 1 };
enum { CVS_TRANSFORM_CATMULL_ROM = 4 };
enum { CVS_TRANSFORM_MAX_COORD = 1 << 23 };
typedef struct cvs_transform {
    float m[6];     /* TARGET -> SOURCE:  u = (m[0]*x + m[1]*y) + m[2];   v = (m[3]*x + m[4]*y) + m[5] */
    int   filter;
    int   flags;    /* none defined: must be 0 */
} cvs_transform;
CVS_EXPORT int cvs_transform_f32_dev(rgba_frame_f32 *target, const rgba_frame_f32 *source, const cvs_transform *t, cvs_stream_t s);
CVS_EXPORT int cvs_transform_f16_dev(rgba_frame_f16 *target, const rgba_frame_f16 *source, const cvs_transform *t, cvs_stream_t s);
/* Pure host arithmetic in double, no device needed.
 * _from_parts: the coefficients of the layer transform  target = position + R(rotation) * diag(scale) * (p - anchor), rotation
 * in degrees, clockwise on screen (y down), multiples of 90 degrees exact; inverted and rounded to f32 once.  0 on success,
 * 1 with `m` untouched when a scale is exactly 0 (degenerate: nothing to draw), -1 with a message for a non-finite input or
 * result.
 * _target_window: the target pixels that can have a tap inside `source_current`, clipped to `target_full` (DESIGN.md has the
 * formula).  _source_window: the source pixels the taps of `target_window` can touch.  Both return 0, or -1 with a message and
 * an empty box for a NULL argument, a filter other than the three, a non-finite coefficient or a determinant that is zero or not
 * finite. */
CVS_EXPORT int cvs_transform_from_parts(const double anchor[2], const double scale[2], double rotation_degrees, const double position[2], float m[6]);
CVS_EXPORT int cvs_transform_target_window(const cvs_transform *t, const box2i *source_current, const box2i *target_full, box2i *win);
CVS_EXPORT int cvs_transform_source_window(const cvs_transform *t, const box2i *target_window, box2i *need);
/* f16 pull of a workspace whose lowest item is a blur node on `source` and whose higher items are `overlays`
 * (bottom first); the blur result stays f32 until the final truncation, as workspace.c:530-544 would have it */
CVS_EXPORT int cvs_blur_over_f16_dev(rgba_frame_f16 *out, const rgba_frame_f16 *source, const float *taps, int ntaps,
                                     const rgba_frame_f16 *const *overlays, int noverlays, cvs_stream_t stream);
CVS_EXPORT int cvs_resample_lanczos_f32_dev(rgba_frame_f32 *target, const rgba_frame_f32 *source, float factor_x, float factor_y, int kernel_size, cvs_stream_t s);
/* the same between f16 frames (widen on load, f32 passes, truncate on store): an f16 pull of the node over a half-native source */
CVS_EXPORT int cvs_resample_lanczos_f16_dev(rgba_frame_f16 *target, const rgba_frame_f16 *source, float factor_x, float factor_y, int kernel_size, cvs_stream_t s);
/* BASELINE config 3 on f16 frames: widen -> blur -> Lanczos resample -> truncate, f32 in between, two launches */
CVS_EXPORT int cvs_blur_lanczos_f16_dev(rgba_frame_f16 *target, const rgba_frame_f16 *source, const float *taps_host, int ntaps,
                                        float factor_x, float factor_y, int kernel_size, cvs_stream_t s);
/* The two entries above for `count` INDEPENDENT frames (a pull queue's frames in flight, a render farm's batch): frames
 * of one geometry that do not feed each other go up to eight at a time into one launch, whose row segments are sized for
 * the whole batch and re-filter fewer halo rows per frame (config 3: 0.084 -> 0.067 ms per 4K frame); every other
 * combination is carried out frame by frame, exactly as `count` single calls.  Results are those of the single calls, bit
 * for bit.  overlays: count x noverlays pointers, frame-major. */
CVS_EXPORT int cvs_blur_over_f16_batch_dev(rgba_frame_f16 *const *outs, const rgba_frame_f16 *const *sources, const float *taps, int ntaps,
                                           const rgba_frame_f16 *const *overlays, int noverlays, int count, cvs_stream_t stream);
CVS_EXPORT int cvs_blur_lanczos_f16_batch_dev(rgba_frame_f16 *const *targets, const rgba_frame_f16 *const *sources, int count,
                                              const float *taps_host, int ntaps, float fx, float fy, int ksize, cvs_stream_t stream);

/* The separable FIR entry points choose among four kernels: the register-window kernel (one tap list for
 * every line), and for per-line tables the gather per target line, tiles in LDS, and the sweep with a lane per pixel.
 * All compute the same sums in the same order -- results are bit-equal, which the parity tests show by pinning each kernel
 * in turn through this call.  It changes speed only, never pixels; process-wide; 0 restores the automatic choice. */
enum { CVS_FIR_PATH_AUTO = 0, CVS_FIR_PATH_PASSES = 1 /* no launch that does both passes: the reference's two passes through an f32 frame */, CVS_FIR_PATH_TILED = 2, CVS_FIR_PATH_TABLES = 4 /* skip the register-window kernel */,
       CVS_FIR_PATH_HV = 16 /* per-line gather, horizontal pass first (the automatic first choice) */,
       CVS_FIR_PATH_ONE_COLUMN = 32 /* the register-window kernels (blur, blur + halving) with one column per lane, never two */,
       CVS_FIR_PATH_TWO_COLUMNS = 64 /* ... with two columns per lane wherever that form takes the launch, narrow frames included */,
       CVS_FIR_PATH_STRIPS = 128 /* the vertical-first triangle scaler on k_fir_vh's strips even where its tile form (k_fir_tile_vh) would take the call */,
       CVS_FIR_PATH_TILES = 256 /* ... on the tile form wherever it takes the call (left alone, the library uses it where it measured faster: floats, and halfs up to about a 4K target) */ };
CVS_EXPORT void cvs_fir_path_override(int mode);
/* Which kernel the calling thread's last FIR launch (scaler, blur, Lanczos resample, blur + resample) went to -- what a
 * test pinned to one kernel asserts, and what tells a silent fallback from the intended kernel.  A fused kernel that was
 * chosen and then failed to launch is reported through the log handler before the next one is tried. */
enum { CVS_FIR_KERNEL_NONE = 0,
       CVS_FIR_KERNEL_WINDOW = 1,      /* k_blur: one tap list for every line, vertical window in registers */
       CVS_FIR_KERNEL_HALVE = 2,       /* k_blur_halve: blur + Lanczos halving in one sweep */
       /* 3: the channel-pair sweep of rounds 2-3 (k_fir_lanes), retired in round 4 in favour of k_fir_hv */
       CVS_FIR_KERNEL_VH = 4,          /* k_fir_vh: the triangle scaler with the vertical pass first */
       CVS_FIR_KERNEL_TILED = 5,       /* k_fir2d: LDS tiles */
       CVS_FIR_KERNEL_RETIRED_6 = 6,   /* (k_fir_stream, lane-per-pixel sweep: retired in round 4) */
       CVS_FIR_KERNEL_TWO_PASS = 7,    /* two k_fir launches through an f32 frame (cached tables) */
       CVS_FIR_KERNEL_PASS = 8,        /* k_fir: one pass of the triangle scaler (both passes: two of these) */
       CVS_FIR_KERNEL_HV = 9,          /* k_fir_hv: per-line tables, horizontal pass first, gather per target line */
       CVS_FIR_KERNEL_WINDOW_PAIR = 10,    /* k_blur_pair: the register-window blur with two columns per lane (f16, up to 13 taps) */
       CVS_FIR_KERNEL_HALVE_PAIR = 11,     /* k_blur_halve_pair: blur + Lanczos halving with two source columns per lane (f16) */
       CVS_FIR_KERNEL_TILE_VH = 12,        /* k_fir_tile_vh: the triangle scaler, vertical pass first, a workgroup per 128 x 16 tile (enlarging) */
       CVS_FIR_KERNEL_UNSHARP = 13 };      /* k_unsharp: register-window blur and unsharp mask in one sweep (the mask's other path reports the blur kernel it used) */
CVS_EXPORT int cvs_fir_last_kernel(void);
/* How many FIR launches of the calling thread were chosen for a fused kernel that then did not launch and went to the next
 * kernel in line (same pixels, slower): each is also reported to the log handler as a warning.  A successful call leaves
 * cvs_last_error() empty either way. */
CVS_EXPORT int cvs_fir_fell_through_count(void);

/* ------------------------------------------------------------------ (3) fused chain: BASELINE config 2
 * out = f16( over-stack_{k=0..n-1}( f32( colour(layer_k) ) ) ), i.e. what the reference computes with
 * color.c on every layer, workspace.c:530-544 over the layers bottom-to-top and main.c:43-71 on the
 * result -- in ONE kernel: 8 B read per layer pixel, 8 B written per output pixel. */
#define CVS_CHAIN_MAX_LAYERS 8
typedef struct {
    rgba_frame_f16 *out;                               /* device frame; current_window is set */
    const rgba_frame_f16 *layers[CVS_CHAIN_MAX_LAYERS];/* device frames, bottom first */
    int nlayers;
} cvs_chain_job;
/* m == NULL: no colour stage -- the plain workspace stack of f16 layers (both tables must then be CVS_LUT_NONE).
 * Jobs are carried out as if one after the other: a job may read or overwrite what an earlier job of the same call
 * wrote (the library starts a new launch there); `out` may be one of the job's own layers (in place), but must not
 * overlap a layer at a shifted address (such a job takes the node-by-node path). */
CVS_EXPORT int cvs_chain_color_over_f16_dev(const cvs_chain_job *jobs, int njobs, const float m[9],
                                            int pre_lut, int post_lut, cvs_stream_t s);
/* how the last chain call ran: 1 = single fused kernel, 0 = node-by-node device kernels
 * (windows did not all cover the output's full window) */
CVS_EXPORT int cvs_chain_last_was_fused(void);
/* 1 when the calling thread's last scaler call (cvs_scale_bilinear_*_dev, video_scale_bilinear_f32) ran both passes in one
 * launch (sweep_vh_ops.hip when the vertical pass comes first, sweep_ops.hip otherwise; factors >= ~0.3); tests and tools */
CVS_EXPORT int cvs_scale_last_was_fused(void);
/* kernel launches the calling thread's last fused chain call was cut into (about eight 4K frames' worth of bytes each) */
CVS_EXPORT int cvs_chain_last_launch_count(void);
/* crossfade of two f16 frames, f16 result: widen, video_mix_cross_f32 (video_mix.c:107-235), truncate -- one launch when
 * every window is the whole output frame */
CVS_EXPORT int cvs_mix_cross_f16_dev(rgba_frame_f16 *out, const rgba_frame_f16 *a, const rgba_frame_f16 *b, float mix_b, cvs_stream_t stream);

#if defined(__cplusplus)
}
#endif
#endif
