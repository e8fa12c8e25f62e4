/*
 * pydeint.c -- the motion-adaptive deinterlacers of fluggo.media.process: the first nodes that look at neighbouring frames in
 * time.
 *
 * The design lists "motion-adaptive ... deinterlacing" among the field conversions (docs/sphinx/feature-proposal/canvas.rst:283-303);
 * the reference built none.  Contract: DESIGN.md "Adaptive deinterlace".  Output frame i of
 *   AdaptiveDeinterlaceFilter(source, field=0, threshold=0.02, softness=0.04)
 *                                       adaptive(source[i - 1], source[i], source[i + 1], field)                     same rate
 *   AdaptiveBobDeinterlaceFilter(source, first_field=0, threshold=0.02, softness=0.04)
 *                                       adaptive(source[s - 1], source[s], source[s + 1], first_field ^ (i & 1)), s = i >> 1
 *                                                                                                                    twice the rate
 * Frame arithmetic floors, as in pyfields.c.  threshold and softness are numbers or frame functions, evaluated at the OUTPUT frame.
 * Both are f16-native on the device slot and thin callers of cvs_deinterlace_adaptive_f16_dev (include/canvas_deinterlace.h).
 * The three source frames are pulled into pooled device scratch over the request grown by one pixel on all four sides (the
 * entry reads a 3 x 3 neighbourhood and the rows above and below), so the result does not depend on how a consumer tiles its
 * requests.  A neighbour whose pull comes back empty, or whose index would leave int, is absent: the start and the end of a
 * clip are deinterlaced against the one neighbour they have.  Locking as in pysources.c and pykey.c.
 */
#include "pyext.h"
#include "canvas_deinterlace.h"
#include <limits.h>
#include <structmember.h>

typedef struct { node1 n; int arg; FrameFunctionHolder threshold, softness; } py_adeint;      /* arg: field or first_field */

static int adeint_init_common(py_adeint *self, PyObject *args, PyObject *kw, char **kwlist) {
    PyObject *src, *threshold = NULL, *softness = NULL;
    self->arg = 0;
    pthread_rwlock_init(&self->n.lock, NULL);
    framefunc_init(&self->threshold, 0.02, 0, 0, 0);
    framefunc_init(&self->softness, 0.04, 0, 0, 0);
    if (!PyArg_ParseTupleAndKeywords(args, kw, "O|iOO", kwlist, &src, &self->arg, &threshold, &softness)) return -1;
    if (self->arg < 0 || self->arg > 1) { PyErr_Format(PyExc_ValueError, "%s must be in 0..1, not %d", kwlist[1], self->arg); return -1; }
    if (!py_video_take_source(src, &self->n.source)) return -1;
    if (threshold && !py_framefunc_take_source(threshold, &self->threshold)) return -1;
    if (softness && !py_framefunc_take_source(softness, &self->softness)) return -1;
    return 0;
}
static void adeint_dealloc(py_adeint *self) {
    py_video_take_source(NULL, &self->n.source);
    py_framefunc_take_source(NULL, &self->threshold);
    py_framefunc_take_source(NULL, &self->softness);
    pthread_rwlock_destroy(&self->n.lock);
    Py_TYPE(self)->tp_free((PyObject *)self);
}

/* one source frame into pooled scratch over `full`; data NULL (no device, no memory) or an empty window: absent */
static rgba_frame_dev pull_scratch(py_adeint *self, int frame_index, const rgba_frame_dev *f, const box2i *full) {
    rgba_frame_dev t = { NULL, CVS_FORMAT_F16, *full, *full, f->stream };
    t.data = cvs_pool_malloc(frame_bytes(full, CVS_FORMAT_F16), f->stream);
    if (!t.data) { box2i_set_empty(&t.current_window); return t; }
    py_rdlock(&self->n.lock);
    video_get_frame_dev(self->n.source, frame_index, &t);
    pthread_rwlock_unlock(&self->n.lock);
    return t;
}

/* output frame `out_index` from source frames source_frame - 1, source_frame, source_frame + 1 */
static void adeint_render_from(py_adeint *self, int out_index, int source_frame, int field, rgba_frame_dev *f) {
    if (box2i_is_empty(&f->full_window)) { box2i_set_empty(&f->current_window); return; }
    box2i grown = f->full_window;
    if (grown.min.x > -CVS_MAX_COORD) grown.min.x--;
    if (grown.min.y > -CVS_MAX_COORD) grown.min.y--;
    if (grown.max.x < CVS_MAX_COORD) grown.max.x++;
    if (grown.max.y < CVS_MAX_COORD) grown.max.y++;
    py_rdlock(&self->n.lock);
    const cvs_deinterlace_adaptive p = { field, framefunc_get_f32(&self->threshold, out_index), framefunc_get_f32(&self->softness, out_index), 0 };
    pthread_rwlock_unlock(&self->n.lock);

    rgba_frame_dev cur = pull_scratch(self, source_frame, f, &grown), prev = { NULL }, next = { NULL };
    rgba_frame_f16 fo = { f->data, f->full_window, f->full_window };
    if (cur.data && !box2i_is_empty(&cur.current_window)) {
        if (source_frame > INT_MIN) prev = pull_scratch(self, source_frame - 1, f, &grown);
        if (source_frame < INT_MAX) next = pull_scratch(self, source_frame + 1, f, &grown);
        rgba_frame_f16 fc = { cur.data, cur.full_window, cur.current_window };
        rgba_frame_f16 fp = { prev.data, prev.full_window, prev.current_window }, fn = { next.data, next.full_window, next.current_window };
        if (cvs_deinterlace_adaptive_f16_dev(&fo, prev.data ? &fp : NULL, &fc, next.data ? &fn : NULL, &p, f->stream) != 0) box2i_set_empty(&fo.current_window);
    } else box2i_set_empty(&fo.current_window);
    f->current_window = fo.current_window;
    cvs_pool_free(cur.data, f->stream); cvs_pool_free(prev.data, f->stream); cvs_pool_free(next.data, f->stream);
}

/* closure: the holder's offset in py_adeint */
static int adeint_set_holder(py_adeint *self, PyObject *v, void *closure) {
    if (!v || v == Py_None) { PyErr_SetString(PyExc_TypeError, "the attribute takes a number or a frame function"); return -1; }
    return node1_set_holder(&self->n, NODE1_HOLDER_AT(self, closure), v);
}
#define ADEINT_HOLDER(member) NODE1_HOLDER(py_adeint, member)

#define ADEINT_TYPE(P, NAME, ARGNAME, DOC)                                                                                         \
    DEFINE_NODE_VTABLE(P, CVS_FORMAT_F16, 1, 0)                                                                                    \
    static void *P##_unused[] __attribute__((unused)) = { (void *)P##_slot_32 };                                                   \
    static PyGetSetDef P##_getset[] = {                                                                                            \
        { VIDEO_FRAME_SOURCE_FUNCS, pyext_capsule_getter, NULL, "Video frame source C API.", &P##_capsule },                       \
        { "source", (getter)node1_get_source, (setter)node1_set_source_attr, "The upstream video source." },                       \
        { "threshold", (getter)node1_get_scalar, (setter)adeint_set_holder,                                                       \
          "Largest difference to the neighbouring frames that still counts as nothing moved (number or frame function).", ADEINT_HOLDER(threshold) }, \
        { "softness", (getter)node1_get_scalar, (setter)adeint_set_holder,                                                        \
          "Width of the ramp from kept to interpolated rows beyond threshold; 0: a hard switch (number or frame function).", ADEINT_HOLDER(softness) }, \
        { NULL } };                                                                                                                \
    static PyMemberDef P##_members[] = { { ARGNAME, T_INT, offsetof(py_adeint, arg), READONLY, DOC }, { NULL } };                  \
    static PyTypeObject py_type_##P = {                                                                                            \
        PyVarObject_HEAD_INIT(NULL, 0)                                                                                             \
        .tp_name = "fluggo.media.process." NAME, .tp_basicsize = sizeof(py_adeint), .tp_flags = Py_TPFLAGS_DEFAULT,                \
        .tp_base = &py_type_VideoSource, .tp_new = PyType_GenericNew, .tp_init = (initproc)P##_init,                               \
        .tp_dealloc = (destructor)adeint_dealloc, .tp_getset = P##_getset, .tp_methods = node1_methods, .tp_members = P##_members, \
    };

/* ---------------------------------------------------------------- AdaptiveDeinterlaceFilter(source, field=0, threshold, softness) */

static int adeint_init(py_adeint *self, PyObject *args, PyObject *kw) {
    static char *kwlist[] = { "source", "field", "threshold", "softness", NULL };
    return adeint_init_common(self, args, kw, kwlist);
}
static void adeint_render(PyObject *o, int i, rgba_frame_dev *f) {
    py_adeint *self = (py_adeint *)o;
    adeint_render_from(self, i, i, self->arg, f);
}
ADEINT_TYPE(adeint, "AdaptiveDeinterlaceFilter", "field", "The field kept: 0 = even rows, 1 = odd rows.")

/* ---------------------------------------------------------------- AdaptiveBobDeinterlaceFilter(source, first_field=0, threshold, softness) */

static int abob_init(py_adeint *self, PyObject *args, PyObject *kw) {
    static char *kwlist[] = { "source", "first_field", "threshold", "softness", NULL };
    return adeint_init_common(self, args, kw, kwlist);
}
static void abob_render(PyObject *o, int i, rgba_frame_dev *f) {
    py_adeint *self = (py_adeint *)o;
    adeint_render_from(self, i, i >> 1, self->arg ^ (i & 1), f);
}
ADEINT_TYPE(abob, "AdaptiveBobDeinterlaceFilter", "first_field", "The field shown first: 0 = even rows, 1 = odd rows.")

int init_deint(PyObject *module) {
    if (pyext_make_capsule(&adeint_capsule, &adeint_funcs) < 0 || pyext_make_capsule(&abob_capsule, &abob_funcs) < 0) return -1;
    if (pyext_add_type(module, "AdaptiveDeinterlaceFilter", &py_type_adeint) < 0 ||
        pyext_add_type(module, "AdaptiveBobDeinterlaceFilter", &py_type_abob) < 0) return -1;
    return 0;
}
