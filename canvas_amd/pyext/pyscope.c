/*
 * pyscope.c -- the scopes of fluggo.media.process: a waveform, an RGB parade or a vectorscope of a picture, as a picture.
 *
 * No reference code: the reference has no scope.  Contract: DESIGN.md "Scopes".
 *   VideoScopeFilter(source, kind, source_rect, columns=256, display="export", gain=1/16, skip_transparent=False)
 *                                                                    cvs_scope_counts_f16_dev + cvs_scope_render_f16_dev
 * A pull takes `source` over source_rect as f16 into a pooled frame, counts it into a pooled table and renders the table into the
 * frame asked for, with the picture's top left pixel at (0, 0); nothing comes to the host.  The node is f16-native: an f32 pull
 * is "pull f16, widen" through the usual dispatch.  gain may be a frame function.  "histogram" has no picture (1280 numbers are
 * the caller's to draw: source.get_scope, pyframes.c) and is a ValueError here.
 * Locking as in pykey.c: reader lock around the upstream pull and the parameters, writer lock where either is replaced.
 * A pull never raises: no source, no device or a refusing entry end in an empty window.
 */
#include "pyext.h"

/* the names of the Python layer: kind -> CVS_SCOPE_*, display -> widget?; -1 with a ValueError set */
int py_scope_kind(const char *name) {
    static const char *names[] = { "histogram", "waveform", "parade", "vectorscope" };
    for (int k = 0; k < 4; k++)
        if (strcmp(name, names[k]) == 0) return k;
    PyErr_SetString(PyExc_ValueError, "kind is \"histogram\", \"waveform\", \"parade\" or \"vectorscope\"");
    return -1;
}
int py_scope_display(const char *name) {
    if (strcmp(name, "export") == 0) return 0;
    if (strcmp(name, "widget") == 0) return 1;
    PyErr_SetString(PyExc_ValueError, "display is \"export\" or \"widget\"");
    return -1;
}
/* "export": the exporter's bytes (no table, the gamma-0.45 ramp); "widget": the software widget's (linear -> sRGB, intent 1.25) */
void py_scope_fill(cvs_scope *p, int kind, int columns, int widget, int skip, const box2i *region) {
    p->kind = kind;
    p->pre_lut = widget ? CVS_LUT_LINEAR_TO_SRGB : CVS_LUT_NONE;
    p->rendering_intent = widget ? 1.25f : 0.0f;
    p->columns = columns;
    p->flags = skip ? CVS_SCOPE_SKIP_TRANSPARENT : 0;
    p->region = *region;
}
bool py_scope_columns_ok(int kind, int columns) {
    if ((kind != CVS_SCOPE_WAVEFORM && kind != CVS_SCOPE_PARADE) || (columns >= 1 && columns <= CVS_SCOPE_MAX_COLUMNS)) return true;
    PyErr_Format(PyExc_ValueError, "columns must be 1..%d", CVS_SCOPE_MAX_COLUMNS);
    return false;
}

typedef struct { node1 n; int kind, columns, widget, skip; box2i rect; FrameFunctionHolder gain; } py_scope;

static int scope_init(py_scope *self, PyObject *args, PyObject *kw) {
    static char *kwlist[] = { "source", "kind", "source_rect", "columns", "display", "gain", "skip_transparent", NULL };
    PyObject *src, *rect, *gain = NULL;
    const char *kind, *display = "export";
    int columns = 256, skip = 0;
    pthread_rwlock_init(&self->n.lock, NULL);
    framefunc_init(&self->gain, 1.0 / 16.0, 0, 0, 0);
    if (!PyArg_ParseTupleAndKeywords(args, kw, "OsO|isOp", kwlist, &src, &kind, &rect, &columns, &display, &gain, &skip)) return -1;
    if ((self->kind = py_scope_kind(kind)) < 0 || (self->widget = py_scope_display(display)) < 0) return -1;
    if (self->kind == CVS_SCOPE_HISTOGRAM) { PyErr_SetString(PyExc_ValueError, "a histogram has no picture: use source.get_scope(..., \"histogram\")"); return -1; }
    if (!py_scope_columns_ok(self->kind, columns)) return -1;
    if (!py_parse_box2i(rect, &self->rect)) return -1;
    self->columns = columns;
    self->skip = skip != 0;
    if (gain == Py_None) { PyErr_SetString(PyExc_TypeError, "gain takes a number or a frame function"); return -1; }
    if (gain && !py_framefunc_take_source(gain, &self->gain)) return -1;
    return py_video_take_source(src, &self->n.source) ? 0 : -1;
}
static void scope_dealloc(py_scope *self) {
    py_video_take_source(NULL, &self->n.source);
    py_framefunc_take_source(NULL, &self->gain);
    pthread_rwlock_destroy(&self->n.lock);
    Py_TYPE(self)->tp_free((PyObject *)self);
}

static void scope_render(PyObject *o, int frame_index, rgba_frame_dev *f) {       /* native: f16 */
    py_scope *self = (py_scope *)o;
    py_rdlock(&self->n.lock);
    cvs_scope p;
    py_scope_fill(&p, self->kind, self->columns, self->widget, self->skip, &self->rect);
    const float gain = framefunc_get_f32(&self->gain, frame_index);
    rgba_frame_dev in = { NULL, CVS_FORMAT_F16, self->rect, self->rect, f->stream };
    uint32_t *counts = NULL;
    const size_t n = cvs_scope_count(&p);
    v2i size;
    int rc = -1;
    if (self->n.source && n && !box2i_is_empty(&self->rect) && cvs_scope_picture_size(&p, &size) == 0) {
        in.data = cvs_pool_malloc(frame_bytes(&self->rect, CVS_FORMAT_F16), f->stream);
        counts = cvs_pool_malloc(n * sizeof(uint32_t), f->stream);
        if (in.data && counts) {
            video_get_frame_dev(self->n.source, frame_index, &in);
            const rgba_frame_f16 fi = { in.data, in.full_window, in.current_window };
            rc = cvs_scope_counts_f16_dev(counts, &fi, &p, f->stream);
        }
        if (rc == 0) {
            const box2i place = { { 0, 0 }, { size.x - 1, size.y - 1 } };
            rgba_frame_f16 fo = { f->data, f->full_window, f->full_window };
            rc = cvs_scope_render_f16_dev(&fo, &place, counts, &p, gain, f->stream);
            f->current_window = fo.current_window;
        }
    }
    pthread_rwlock_unlock(&self->n.lock);
    if (rc != 0) box2i_set_empty(&f->current_window);
    cvs_pool_free(counts, f->stream);
    cvs_pool_free(in.data, f->stream);
}
DEFINE_NODE_VTABLE(scope, CVS_FORMAT_F16, 1, 0)
static void *scope_unused[] __attribute__((unused)) = { (void *)scope_slot_32 };

static PyObject *scope_get_kind(py_scope *self, void *c) {
    static const char *names[] = { "histogram", "waveform", "parade", "vectorscope" };
    return PyUnicode_FromString(names[self->kind]);
}
static int scope_set_kind(py_scope *self, PyObject *v, void *c) {
    if (!v || !PyUnicode_Check(v)) { PyErr_SetString(PyExc_TypeError, "kind is a string"); return -1; }
    const int kind = py_scope_kind(PyUnicode_AsUTF8(v));
    if (kind < 0) return -1;
    if (kind == CVS_SCOPE_HISTOGRAM) { PyErr_SetString(PyExc_ValueError, "a histogram has no picture"); return -1; }
    if (!py_scope_columns_ok(kind, self->columns)) return -1;           /* a vectorscope may hold columns a waveform cannot take */
    py_wrlock_nogil(&self->n.lock);
    self->kind = kind;
    pthread_rwlock_unlock(&self->n.lock);
    return 0;
}
static PyObject *scope_get_display(py_scope *self, void *c) { return PyUnicode_FromString(self->widget ? "widget" : "export"); }
static int scope_set_display(py_scope *self, PyObject *v, void *c) {
    if (!v || !PyUnicode_Check(v)) { PyErr_SetString(PyExc_TypeError, "display is a string"); return -1; }
    const int widget = py_scope_display(PyUnicode_AsUTF8(v));
    if (widget < 0) return -1;
    py_wrlock_nogil(&self->n.lock);
    self->widget = widget;
    pthread_rwlock_unlock(&self->n.lock);
    return 0;
}
static PyObject *scope_get_columns(py_scope *self, void *c) { return PyLong_FromLong(self->columns); }
static int scope_set_columns(py_scope *self, PyObject *v, void *c) {
    if (!v || !PyLong_Check(v) || PyBool_Check(v)) { PyErr_SetString(PyExc_TypeError, "columns is an integer"); return -1; }
    const long columns = PyLong_AsLong(v);
    if (columns == -1 && PyErr_Occurred()) return -1;
    if (columns < 1 || columns > CVS_SCOPE_MAX_COLUMNS) { PyErr_Format(PyExc_ValueError, "columns must be 1..%d", CVS_SCOPE_MAX_COLUMNS); return -1; }
    py_wrlock_nogil(&self->n.lock);
    self->columns = (int)columns;
    pthread_rwlock_unlock(&self->n.lock);
    return 0;
}
static PyObject *scope_get_rect(py_scope *self, void *c) { return py_make_box2i(&self->rect); }
static int scope_set_rect(py_scope *self, PyObject *v, void *c) {
    box2i rect;
    if (!v || !py_parse_box2i(v, &rect)) { if (!PyErr_Occurred()) PyErr_SetString(PyExc_TypeError, "source_rect is a box2i"); return -1; }
    py_wrlock_nogil(&self->n.lock);
    self->rect = rect;
    pthread_rwlock_unlock(&self->n.lock);
    return 0;
}
static int scope_set_gain(py_scope *self, PyObject *v, void *c) {
    if (!v || v == Py_None) { PyErr_SetString(PyExc_TypeError, "gain takes a number or a frame function"); return -1; }
    return node1_set_holder(&self->n, &self->gain, v);
}
static PyObject *scope_get_skip(py_scope *self, void *c) { return PyBool_FromLong(self->skip); }
static int scope_set_skip(py_scope *self, PyObject *v, void *c) {
    if (!v || !PyBool_Check(v)) { PyErr_SetString(PyExc_TypeError, "skip_transparent is a bool"); return -1; }
    py_wrlock_nogil(&self->n.lock);
    self->skip = v == Py_True;
    pthread_rwlock_unlock(&self->n.lock);
    return 0;
}

static PyGetSetDef scope_getset[] = {
    { VIDEO_FRAME_SOURCE_FUNCS, pyext_capsule_getter, NULL, "Video frame source C API.", &scope_capsule },
    { "source", (getter)node1_get_source, (setter)node1_set_source_attr, "The upstream video source." },
    { "kind", (getter)scope_get_kind, (setter)scope_set_kind, "\"waveform\", \"parade\" or \"vectorscope\"." },
    { "source_rect", (getter)scope_get_rect, (setter)scope_set_rect, "The part of the source that is measured (box2i)." },
    { "columns", (getter)scope_get_columns, (setter)scope_set_columns, "Output columns of a waveform, of each panel of a parade." },
    { "display", (getter)scope_get_display, (setter)scope_set_display, "\"export\" (the exporter's bytes) or \"widget\" (the software widget's)." },
    { "gain", (getter)node1_get_scalar, (setter)scope_set_gain, "Brightness per counted pixel (number or frame function).", NODE1_HOLDER(py_scope, gain) },
    { "skip_transparent", (getter)scope_get_skip, (setter)scope_set_skip, "Leave out the pixels whose alpha byte is 0." },
    { NULL }
};
static PyTypeObject py_type_Scope = {
    PyVarObject_HEAD_INIT(NULL, 0)
    .tp_name = "fluggo.media.process.VideoScopeFilter", .tp_basicsize = sizeof(py_scope), .tp_flags = Py_TPFLAGS_DEFAULT,
    .tp_base = &py_type_VideoSource, .tp_new = PyType_GenericNew, .tp_init = (initproc)scope_init,
    .tp_dealloc = (destructor)scope_dealloc, .tp_getset = scope_getset, .tp_methods = node1_methods,
};

int init_scope(PyObject *module) {
    if (pyext_make_capsule(&scope_capsule, &scope_funcs) < 0) return -1;
    return pyext_add_type(module, "VideoScopeFilter", &py_type_Scope);
}
