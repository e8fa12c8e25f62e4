/*
 * pyext.h -- internals of the fluggo.media.process extension module built on libcanvas_hip.so.
 *
 * Every node type (filter / source) renders into a DEVICE frame: its vtable carries
 * VIDEO_SOURCE_FLAG_DEVICE and a slot-3 entry, so a graph of these nodes stays in HBM from the
 * sources to the consumer.  The host slots the reference's vtable also has (get_frame /
 * get_frame_32) are thin edges over the same render: allocate a device frame, render, copy back once.
 */
#ifndef CANVAS_PYEXT_H
#define CANVAS_PYEXT_H

#define PY_SSIZE_T_CLEAN
#include "pyframework.h"
#include "canvas_scope.h"
#include "canvas_perspective.h"
#include <pthread.h>

/* Node locks and the GIL.  Worker threads (pull queue, playback) hold the reader side of a node's rwlock across a pull,
 * and a pull may need the GIL (a source or a frame function written in Python).  Python-called methods take either side
 * with the GIL held.  The one rule that keeps the pair (lock, GIL) free of cycles: NOBODY BLOCKS ON A NODE LOCK WHILE
 * HOLDING THE GIL.  Both sides try first and, if the lock is busy, wait for it with the GIL released.  A thread may then
 * wait for the GIL while it holds the lock (the writer coming back from its wait, a worker's reader calling into
 * Python): whoever has the GIL at that moment either runs on or gives it up before it blocks on the lock, so the wait ends.
 * (The first form released the GIL only on the writer side: a writer coming back for the GIL with the lock in hand met
 * a reader that had blocked on the lock with the GIL in hand -- anim.add() against get_values() from a callback.) */
static inline void py_wrlock_nogil(pthread_rwlock_t *lock) {
    if (pthread_rwlock_trywrlock(lock) == 0) return;
    Py_BEGIN_ALLOW_THREADS
    pthread_rwlock_wrlock(lock);
    Py_END_ALLOW_THREADS
}
/* reader side: called from worker threads without the GIL and from Python-called code with it */
static inline void py_rdlock(pthread_rwlock_t *lock) {
    if (pthread_rwlock_tryrdlock(lock) == 0) return;
    if (PyGILState_Check()) {
        Py_BEGIN_ALLOW_THREADS
        pthread_rwlock_rdlock(lock);
        Py_END_ALLOW_THREADS
    } else {
        pthread_rwlock_rdlock(lock);
    }
}

/* a node's native render: fill `frame` (device, of the node's native format) for frame_index */
typedef void (*node_render_func)(PyObject *self, int frame_index, rgba_frame_dev *frame);

/* shared plumbing (pymodule.c) */
void node_get_frame_dev(PyObject *self, int frame_index, rgba_frame_dev *frame, int native_format, node_render_func render);
void node_get_frame_host16(PyObject *self, int frame_index, rgba_frame_f16 *frame, int native_format, node_render_func render);
void node_get_frame_host32(PyObject *self, int frame_index, rgba_frame_f32 *frame, int native_format, node_render_func render);
size_t frame_bytes(const box2i *full, int format);

/* one static vtable + capsule per type, exposed through the `_video_frame_source_funcs` attribute */
PyObject *pyext_capsule_getter(PyObject *self, void *closure);      /* closure = PyObject** (capsule slot) */
int pyext_add_type(PyObject *module, const char *name, PyTypeObject *type);
int pyext_make_capsule(PyObject **slot, video_frame_source_funcs *funcs);

/* a keyword that names one of a few values: the table ends with a NULL name.  *value = the value of `given` (absent: `def`); false
 * with a ValueError that names the choices, as in: Node: layout must be "planar8", "planar10", "uyvy" or "v210", not 'x' */
typedef struct { const char *name; int value; } pyext_choice;
bool pyext_choose(const char *node, const char *what, PyObject *given, const pyext_choice *choices, int def, int *value);

/* a node with one upstream source (pysources.c): the struct every such type starts with, the `source` attribute's getter and
 * setter and the set_source(source) method table; reader lock around any upstream pull, writer lock where the source changes */
typedef struct { PyObject_HEAD pthread_rwlock_t lock; video_source *source; } node1;
PyObject *node1_get_source(node1 *self, void *closure);
PyObject *node1_set_source(node1 *self, PyObject *args);
int node1_set_source_attr(node1 *self, PyObject *value, void *closure);
extern PyMethodDef node1_methods[];
/* a "number or frame function" attribute of such a node: `value` is parsed into a holder of its own with no lock held (a value
 * that is refused leaves the old one, and parsing may run Python code), swapped in under the writer lock, and what the
 * attribute held is released after unlocking.  None and NULL give the constant 0, as py_framefunc_take_source does: a node
 * that refuses them says so before it calls.  0, or -1 with a Python error set */
int node1_set_holder(node1 *self, FrameFunctionHolder *holder, PyObject *value);
PyObject *node1_get_scalar(node1 *self, void *holder_offset);       /* getter: the frame function, or the constant as a float */
#define NODE1_HOLDER(type, member) ((void *)offsetof(type, member))
#define NODE1_HOLDER_AT(self, offset) ((FrameFunctionHolder *)((char *)(self) + (size_t)(offset)))

/* a source that fills the f16 host slot only is half-native: its f32 pull is "pull f16, widen" (main.c:105-144) */
static inline bool half_native(const video_source *src) { return src && src->funcs && src->funcs->get_frame && !src->funcs->get_frame_32; }
/* the device slot of a node1 whose own format is f32 and whose render takes either: an f16 pull over a half-native source is
 * rendered as f16 directly (the entry widens, works and truncates in one launch), any other goes through the f32 render */
void node1_get_frame_dev_half_direct(PyObject *self, int frame_index, rgba_frame_dev *frame, node_render_func render);

/* the geometry nodes' shared core (pywarp.c; pytransform.c and pyperspective.c keep what differs).  A node is a table of parts
 * -- each a constant of its shape or a frame function -- and a filter; a pull is warp_render over the node's warp_ops. */
enum { WARP_BOX2I, WARP_PAIR, WARP_NUMBER };
enum { WARP_PARTS = 5 };
typedef struct { const char *name; int shape; } warp_part;
/* given[k]: the constant as it was handed over (what the attribute reads back), NULL where the holder has a frame function */
typedef struct { node1 n; const warp_part *table; FrameFunctionHolder part[WARP_PARTS]; PyObject *given[WARP_PARTS]; int filter; } warp_node;
/* what a node's `plan` works out of one frame under the reader lock: the coefficients the entry takes; `need`, the source
 * window the taps of the frame asked for can touch; `rect`, what may be pulled of it; `layer`, the window the node reports;
 * sound: there is a map at all; refused: need clipped to rect is a window the entry will refuse (it is not pulled, the entry
 * is still called, for its message) */
typedef struct {
    union { cvs_transform affine; cvs_perspective pin; } c;
    box2i need, rect, layer;
    bool sound, refused;
} warp_plan;
typedef struct {
    void (*plan)(warp_node *self, int frame_index, const box2i *full, warp_plan *p);
    int (*entry)(int format, void *out, const void *in, const warp_plan *p, void *stream);    /* rgba_frame_f16 or _f32, by format */
    int (*fill_layer)(rgba_frame_dev *f, const box2i *layer);                                  /* the node's window rule */
} warp_ops;
void warp_node_init(warp_node *self, const warp_part *table);
void warp_node_dealloc(warp_node *self);
/* parts first .. first + count - 1 from values[]: all of them or, with a Python error set, none; locked: the node is alive */
int warp_parts_set(warp_node *self, int first, int count, PyObject **values, bool locked);
PyObject *warp_get_part(warp_node *self, void *index);              /* getter and setter of one part, closure: its index */
int warp_set_part(warp_node *self, PyObject *value, void *index);
PyObject *warp_get_filter(warp_node *self, void *closure);
int warp_set_filter(warp_node *self, PyObject *value, void *closure);
int warp_filter_from(PyObject *v);                                  /* "nearest" / "bilinear" / "catmull-rom" -> CVS_TRANSFORM_*, or -1 with a Python error set */
void warp_render(warp_node *self, int frame_index, rgba_frame_dev *f, const warp_ops *ops);
/* transparent black over `all` minus `win` (win inside all, or empty) in at most four strips, windows left alone: 0, or -1 */
int warp_clear_around(rgba_frame_dev *f, const box2i *all, const box2i *win);

/* frame objects (pyframes.c) */
PyObject *py_RgbaFrameF16_new(box2i *full_window, rgba_frame_f16 **frame);
PyObject *py_RgbaFrameF32_new(box2i *full_window, rgba_frame_f32 **frame);
PyObject *py_get_frame_f16(PyObject *self, PyObject *args, PyObject *kw);
PyObject *py_get_frame_f32(PyObject *self, PyObject *args, PyObject *kw);
PyObject *py_get_frame_argb32(PyObject *self, PyObject *args, PyObject *kw);
PyObject *py_get_frame_rgba8(PyObject *self, PyObject *args, PyObject *kw);
PyObject *py_get_scope(PyObject *self, PyObject *args, PyObject *kw);

/* the scopes' names and defaults (pyscope.c), shared by the node and by source.get_scope; -1 / false with a ValueError set */
int py_scope_kind(const char *name);
int py_scope_display(const char *name);
bool py_scope_columns_ok(int kind, int columns);
void py_scope_fill(cvs_scope *p, int kind, int columns, int widget, int skip, const box2i *region);

/* a channel set as the nodes take it (pymedian.c): a string of distinct letters from "rgba", at least one, <-> a CVS_MEDIAN_*
 * mask; the letters read back in the order r, g, b, a.  -1 with a TypeError or ValueError set */
int py_channels_parse(PyObject *obj);
PyObject *py_channels_string(int mask);

/* coded planes staged on the device (pydv.c), shared by every reconstruction and subsample node: see there */
typedef int (*py_planes_recon)(rgba_frame_f16 *out, const coded_image *dev, const void *node, cvs_stream_t s);
typedef int (*py_planes_sub)(coded_image *dev, const rgba_frame_f16 *in, const void *node, cvs_stream_t s);
void py_planes_render(CodedImageSourceHolder *source, int planes, py_planes_recon entry, const void *node, int frame_index, rgba_frame_dev *f);
coded_image *py_planes_from_source(video_source *source, int frame, const box2i *window, const int strides[3], const int lines[3], int count,
                                   py_planes_sub entry, const void *node);

int init_frames(PyObject *module);
int init_framefuncs(PyObject *module);
int init_animation(PyObject *module);
int init_dv(PyObject *module);
int init_sources(PyObject *module);
int init_fields(PyObject *module);
int init_deint(PyObject *module);
int init_blur(PyObject *module);
int init_key(PyObject *module);
int init_matte(PyObject *module);
int init_median(PyObject *module);
int init_temporal(PyObject *module);
int init_transform(PyObject *module);
int init_scope(PyObject *module);
int init_lut3d(PyObject *module);
int init_primary(PyObject *module);
int init_secondary(PyObject *module);
int init_perspective(PyObject *module);
int init_workspace(PyObject *module);
int init_ycc422(PyObject *module);
int init_ycc420(PyObject *module);

/* node vtable boilerplate: DEFINE_NODE_VTABLE(Prefix, CVS_FORMAT_F16 or _F32, host16?, host32?) */
#define DEFINE_NODE_VTABLE(P, NATIVE, HOST16, HOST32)                                                          \
    static void P##_slot_dev(PyObject *self, int i, rgba_frame_dev *f) { node_get_frame_dev(self, i, f, NATIVE, P##_render); }   \
    static void P##_slot_16(PyObject *self, int i, rgba_frame_f16 *f) { node_get_frame_host16(self, i, f, NATIVE, P##_render); } \
    static void P##_slot_32(PyObject *self, int i, rgba_frame_f32 *f) { node_get_frame_host32(self, i, f, NATIVE, P##_render); } \
    static video_frame_source_funcs P##_funcs = {                                                             \
        .flags = VIDEO_SOURCE_FLAG_DEVICE,                                                                    \
        .get_frame = (HOST16) ? (video_get_frame_func)P##_slot_16 : NULL,                                     \
        .get_frame_32 = (HOST32) ? (video_get_frame_32_func)P##_slot_32 : NULL,                               \
        .get_frame_dev = (video_get_frame_dev_func)P##_slot_dev };                                            \
    static PyObject *P##_capsule;
/* the same for a node1 with node1_get_frame_dev_half_direct in the device slot: DEFINE_NODE_VTABLE_HALF_DIRECT(Prefix) */
#define DEFINE_NODE_VTABLE_HALF_DIRECT(P)                                                                      \
    static void P##_slot_dev(PyObject *self, int i, rgba_frame_dev *f) { node1_get_frame_dev_half_direct(self, i, f, P##_render); } \
    static void P##_slot_32(PyObject *self, int i, rgba_frame_f32 *f) { node_get_frame_host32(self, i, f, CVS_FORMAT_F32, P##_render); } \
    static video_frame_source_funcs P##_funcs = {                                                             \
        .flags = VIDEO_SOURCE_FLAG_DEVICE, .get_frame_32 = (video_get_frame_32_func)P##_slot_32,              \
        .get_frame_dev = (video_get_frame_dev_func)P##_slot_dev };                                            \
    static PyObject *P##_capsule;

#endif
