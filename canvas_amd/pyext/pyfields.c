/*
 * pyfields.c -- the field-conversion nodes of fluggo.media.process: between woven (interlaced) frames and whole pictures.
 *
 * The design lists these conversions (docs/sphinx/feature-proposal/canvas.rst:283-303) and the editor names them
 * (fluggo/editor/model/sources.py:536-542: discard_field, bob_deinterlace, bob_interlace, add_pulldown); the reference built
 * only the pulldown removal (pysources.c here).  Output frame i of
 *   DeinterlaceFilter(source, field=0)             field_to_frame(source[i], field)                          same rate
 *   BobDeinterlaceFilter(source, first_field=0)    field_to_frame(source[i >> 1], first_field ^ (i & 1))     twice the rate
 *   WeaveInterlaceFilter(source)                   soften(source[i])                                         same rate
 *   BobInterlaceFilter(source, first_field=0)      rows of parity first_field from source[2i], the others from source[2i + 1]
 *   Pulldown23AdditionFilter(source, offset)       even rows from source[e], odd rows from source[o],
 *                                                  (e, o) = cvs_pulldown23_add_frames(offset, i); one pull when e == o
 * Frame arithmetic floors (negative indices continue the pattern backwards).  All are f16-native on the device slot and thin
 * callers of the library's entries (include/canvas_hip.h "Field conversions"); the source frames are pulled into pooled device
 * scratch on the frame's stream, nothing crosses PCIe between the pull and the result.  Locking as in pysources.c.
 */
#include "pyext.h"
#include <limits.h>
#include <structmember.h>

typedef struct { node1 n; int arg; } py_field;         /* arg: field, first_field or offset */

static rgba_frame_dev scratch_f16(const rgba_frame_dev *f, const box2i *full) {
    rgba_frame_dev t = { NULL, CVS_FORMAT_F16, *full, *full, f->stream };
    t.data = cvs_pool_malloc(frame_bytes(full, CVS_FORMAT_F16), f->stream);
    return t;
}

static void pull_locked(py_field *self, int frame_index, rgba_frame_dev *frame) {
    py_rdlock(&self->n.lock);
    video_get_frame_dev(self->n.source, frame_index, frame);
    pthread_rwlock_unlock(&self->n.lock);
}

static int field_init_common(py_field *self, PyObject *args, PyObject *kw, char **kwlist, const char *format, int lo, int hi) {
    PyObject *src;
    self->arg = 0;
    pthread_rwlock_init(&self->n.lock, NULL);
    if (!PyArg_ParseTupleAndKeywords(args, kw, format, kwlist, &src, &self->arg)) return -1;
    if (self->arg < lo || self->arg > hi) { PyErr_Format(PyExc_ValueError, "%s must be in %d..%d, not %d", kwlist[1], lo, hi, self->arg); return -1; }     /* (a type without the argument has lo == hi == 0) */
    return py_video_take_source(src, &self->n.source) ? 0 : -1;
}
static void field_dealloc(py_field *self) {
    py_video_take_source(NULL, &self->n.source);
    pthread_rwlock_destroy(&self->n.lock);
    Py_TYPE(self)->tp_free((PyObject *)self);
}

/* The two filtering conversions read source rows just outside the rows they produce: the source is pulled into scratch
 * covering the request grown by one row above and below, so the result does not depend on how a consumer tiles its requests.
 * filter(out, in): the library entry, `field` passed through. */
static void render_filtered(py_field *self, int source_frame, rgba_frame_dev *f, int field,
                            int (*filter)(rgba_frame_f16 *, const rgba_frame_f16 *, int, cvs_stream_t)) {
    box2i grown = f->full_window;
    if (grown.min.y > INT_MIN) grown.min.y--;
    if (grown.max.y < INT_MAX) grown.max.y++;
    rgba_frame_dev in = scratch_f16(f, &grown);
    if (!in.data) { box2i_set_empty(&f->current_window); return; }
    pull_locked(self, source_frame, &in);
    rgba_frame_f16 fi = { in.data, in.full_window, in.current_window }, fo = { f->data, f->full_window, f->full_window };
    if (filter(&fo, &fi, field, f->stream) != 0) box2i_set_empty(&fo.current_window);
    f->current_window = fo.current_window;
    cvs_pool_free(in.data, f->stream);
}
static int soften_entry(rgba_frame_f16 *out, const rgba_frame_f16 *in, int unused, cvs_stream_t s) { return cvs_soften_fields_f16_dev(out, in, s); }

/* even rows of `f` from source frame `even_frame`, odd rows from `odd_frame` */
static void render_woven(py_field *self, int even_frame, int odd_frame, rgba_frame_dev *f) {
    rgba_frame_dev te = scratch_f16(f, &f->full_window), to = scratch_f16(f, &f->full_window);
    if (te.data && to.data) {
        pull_locked(self, even_frame, &te);
        pull_locked(self, odd_frame, &to);
        rgba_frame_f16 fe = { te.data, te.full_window, te.current_window }, fd = { to.data, to.full_window, to.current_window };
        rgba_frame_f16 fo = { f->data, f->full_window, f->full_window };
        if (cvs_interlace_fields_f16_dev(&fo, &fe, &fd, f->stream) != 0) box2i_set_empty(&fo.current_window);
        f->current_window = fo.current_window;
    } else box2i_set_empty(&f->current_window);
    cvs_pool_free(te.data, f->stream); cvs_pool_free(to.data, f->stream);
}

#define FIELD_TYPE(P, NAME, ARGNAME, DOC)                                                                                          \
    DEFINE_NODE_VTABLE(P, CVS_FORMAT_F16, 1, 0)                                                                                    \
    static void *P##_unused[] __attribute__((unused)) = { (void *)P##_slot_32 };                                                   \
    static PyGetSetDef P##_getset[] = {                                                                                            \
        { VIDEO_FRAME_SOURCE_FUNCS, pyext_capsule_getter, NULL, "Video frame source C API.", &P##_capsule },                       \
        { "source", (getter)node1_get_source, (setter)node1_set_source_attr, "The upstream video source." },                       \
        { NULL } };                                                                                                                \
    static PyMemberDef P##_members[] = { { ARGNAME, T_INT, offsetof(py_field, arg), READONLY, DOC }, { NULL } };                   \
    static PyTypeObject py_type_##P = {                                                                                            \
        PyVarObject_HEAD_INIT(NULL, 0)                                                                                             \
        .tp_name = "fluggo.media.process." NAME, .tp_basicsize = sizeof(py_field), .tp_flags = Py_TPFLAGS_DEFAULT,                 \
        .tp_base = &py_type_VideoSource, .tp_new = PyType_GenericNew, .tp_init = (initproc)P##_init,                               \
        .tp_dealloc = (destructor)field_dealloc, .tp_getset = P##_getset, .tp_methods = node1_methods, .tp_members = P##_members,  \
    };

/* ---------------------------------------------------------------- DeinterlaceFilter(source, field=0) */

static int deint_init(py_field *self, PyObject *args, PyObject *kw) {
    static char *kwlist[] = { "source", "field", NULL };
    return field_init_common(self, args, kw, kwlist, "O|i", 0, 1);
}
static void deint_render(PyObject *o, int i, rgba_frame_dev *f) {
    py_field *self = (py_field *)o;
    render_filtered(self, i, f, self->arg, cvs_field_to_frame_f16_dev);
}
FIELD_TYPE(deint, "DeinterlaceFilter", "field", "The field kept: 0 = even rows, 1 = odd rows.")

/* ---------------------------------------------------------------- BobDeinterlaceFilter(source, first_field=0) */

static int bobd_init(py_field *self, PyObject *args, PyObject *kw) {
    static char *kwlist[] = { "source", "first_field", NULL };
    return field_init_common(self, args, kw, kwlist, "O|i", 0, 1);
}
static void bobd_render(PyObject *o, int i, rgba_frame_dev *f) {
    py_field *self = (py_field *)o;
    render_filtered(self, i >> 1, f, self->arg ^ (i & 1), cvs_field_to_frame_f16_dev);
}
FIELD_TYPE(bobd, "BobDeinterlaceFilter", "first_field", "The field shown first: 0 = even rows, 1 = odd rows.")

/* ---------------------------------------------------------------- WeaveInterlaceFilter(source) */

static int weave_init(py_field *self, PyObject *args, PyObject *kw) {
    static char *kwlist[] = { "source", NULL };
    return field_init_common(self, args, kw, kwlist, "O", 0, 0);
}
static void weave_render(PyObject *o, int i, rgba_frame_dev *f) { render_filtered((py_field *)o, i, f, 0, soften_entry); }
DEFINE_NODE_VTABLE(weave, CVS_FORMAT_F16, 1, 0)
static void *weave_unused[] __attribute__((unused)) = { (void *)weave_slot_32 };
static PyGetSetDef weave_getset[] = {
    { VIDEO_FRAME_SOURCE_FUNCS, pyext_capsule_getter, NULL, "Video frame source C API.", &weave_capsule },
    { "source", (getter)node1_get_source, (setter)node1_set_source_attr, "The upstream video source." },
    { NULL } };
static PyTypeObject py_type_weave = {
    PyVarObject_HEAD_INIT(NULL, 0)
    .tp_name = "fluggo.media.process.WeaveInterlaceFilter", .tp_basicsize = sizeof(py_field), .tp_flags = Py_TPFLAGS_DEFAULT,
    .tp_base = &py_type_VideoSource, .tp_new = PyType_GenericNew, .tp_init = (initproc)weave_init,
    .tp_dealloc = (destructor)field_dealloc, .tp_getset = weave_getset, .tp_methods = node1_methods,
};

/* ---------------------------------------------------------------- BobInterlaceFilter(source, first_field=0) */

static int bobi_init(py_field *self, PyObject *args, PyObject *kw) {
    static char *kwlist[] = { "source", "first_field", NULL };
    return field_init_common(self, args, kw, kwlist, "O|i", 0, 1);
}
static void bobi_render(PyObject *o, int i, rgba_frame_dev *f) {
    py_field *self = (py_field *)o;
    if (i > INT_MAX / 2 || i < INT_MIN / 2) { box2i_set_empty(&f->current_window); return; }
    const int first = 2 * i, second = 2 * i + 1;
    render_woven(self, self->arg == 0 ? first : second, self->arg == 0 ? second : first, f);
}
FIELD_TYPE(bobi, "BobInterlaceFilter", "first_field", "The rows the first of each two source frames goes to: 0 = even, 1 = odd.")

/* ---------------------------------------------------------------- Pulldown23AdditionFilter(source, offset) */

static int pdadd_init(py_field *self, PyObject *args, PyObject *kw) {
    static char *kwlist[] = { "source", "offset", NULL };
    return field_init_common(self, args, kw, kwlist, "Oi", 0, 4);
}
static void pdadd_render(PyObject *o, int i, rgba_frame_dev *f) {
    py_field *self = (py_field *)o;
    int even, odd;
    const int mixed = cvs_pulldown23_add_frames(self->arg, i, &even, &odd);
    if (mixed < 0) box2i_set_empty(&f->current_window);
    else if (mixed == 0) pull_locked(self, even, f);
    else render_woven(self, even, odd, f);
}
FIELD_TYPE(pdadd, "Pulldown23AdditionFilter", "offset", "Phase of the 2:3 cadence, 0..4.")

int init_fields(PyObject *module) {
    if (pyext_make_capsule(&deint_capsule, &deint_funcs) < 0 || pyext_make_capsule(&bobd_capsule, &bobd_funcs) < 0 ||
        pyext_make_capsule(&weave_capsule, &weave_funcs) < 0 || pyext_make_capsule(&bobi_capsule, &bobi_funcs) < 0 ||
        pyext_make_capsule(&pdadd_capsule, &pdadd_funcs) < 0) return -1;
    if (pyext_add_type(module, "DeinterlaceFilter", &py_type_deint) < 0 || pyext_add_type(module, "BobDeinterlaceFilter", &py_type_bobd) < 0 ||
        pyext_add_type(module, "WeaveInterlaceFilter", &py_type_weave) < 0 || pyext_add_type(module, "BobInterlaceFilter", &py_type_bobi) < 0 ||
        pyext_add_type(module, "Pulldown23AdditionFilter", &py_type_pdadd) < 0) return -1;
    return 0;
}
