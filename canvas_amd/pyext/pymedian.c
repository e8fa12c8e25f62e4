/*
 * pymedian.c -- the despeckle of fluggo.media.process: a 3 x 3 or 5 x 5 median per channel.
 *
 * No reference code (the reference has no rank filter).  Contract: DESIGN.md "Median".
 *   VideoMedianFilter(source, radius=1, threshold=0.0, channels="rgba")          cvs_median_f32_dev / _f16_dev
 * f32 is the node's own format; an f16 pull over a half-native source goes through the _f16_dev entry in one launch (pymatte.c).
 * The source is pulled over the requested window grown by `radius` on every side into a pooled frame, so a frame pulled in
 * tiles equals the frame pulled whole; the entry then writes the frame asked for.  threshold is a number or a frame function,
 * radius an int (1 or 2), channels a string of distinct letters from "rgba", read back in that order.  Locking as in pymatte.c:
 * reader lock around the upstream pull and the parameters, writer lock where either is replaced.
 */
#include "pyext.h"
#include "canvas_median.h"
#include <limits.h>

typedef struct { node1 n; FrameFunctionHolder threshold; int radius, channels; } py_median;

/* "rgba" letters, each at most once, at least one -> CVS_MEDIAN_* mask; -1 with a Python error set (pyext.h: pytemporal.c's too) */
int py_channels_parse(PyObject *obj) {
    if (!obj || !PyUnicode_Check(obj)) { PyErr_SetString(PyExc_TypeError, "channels is a string of letters from \"rgba\""); return -1; }
    Py_ssize_t n;
    const char *s = PyUnicode_AsUTF8AndSize(obj, &n);
    if (!s) return -1;
    int mask = 0;
    for (Py_ssize_t k = 0; k < n; k++) {
        const char *at = s[k] ? strchr("rgba", s[k]) : NULL;
        const int bit = at ? 1 << (int)(at - "rgba") : 0;
        if (!bit || (mask & bit)) { PyErr_SetString(PyExc_ValueError, "channels takes distinct letters from \"rgba\""); return -1; }
        mask |= bit;
    }
    if (!mask) { PyErr_SetString(PyExc_ValueError, "channels names at least one of \"rgba\""); return -1; }
    return mask;
}
/* an int 1 or 2 -> itself; 0 with a Python error set */
static int parse_radius(PyObject *obj) {
    if (!obj || !PyLong_Check(obj) || PyBool_Check(obj)) { PyErr_SetString(PyExc_TypeError, "radius is an int: 1 (3 x 3) or 2 (5 x 5)"); return 0; }
    const long v = PyLong_AsLong(obj);
    if (v == -1 && PyErr_Occurred()) return 0;
    if (v != 1 && v != 2) { PyErr_SetString(PyExc_ValueError, "radius is 1 (3 x 3) or 2 (5 x 5)"); return 0; }
    return (int)v;
}

static int median_init(py_median *self, PyObject *args, PyObject *kw) {
    static char *kwlist[] = { "source", "radius", "threshold", "channels", NULL };
    PyObject *src, *radius = NULL, *threshold = NULL, *channels = NULL;
    pthread_rwlock_init(&self->n.lock, NULL);
    framefunc_init(&self->threshold, 0.0, 0, 0, 0);
    self->radius = 1;
    self->channels = CVS_MEDIAN_ALL;
    if (!PyArg_ParseTupleAndKeywords(args, kw, "O|OOO", kwlist, &src, &radius, &threshold, &channels)) return -1;
    if (radius && !(self->radius = parse_radius(radius))) return -1;
    if (channels && (self->channels = py_channels_parse(channels)) < 0) return -1;
    if (!py_video_take_source(src, &self->n.source)) return -1;
    if (threshold && (threshold == Py_None || !py_framefunc_take_source(threshold, &self->threshold))) { if (!PyErr_Occurred()) PyErr_SetString(PyExc_TypeError, "threshold takes a number or a frame function"); return -1; }
    return 0;
}
static void median_dealloc(py_median *self) {
    py_video_take_source(NULL, &self->n.source);
    py_framefunc_take_source(NULL, &self->threshold);
    pthread_rwlock_destroy(&self->n.lock);
    Py_TYPE(self)->tp_free((PyObject *)self);
}

static int grow_down(int v, int by) { return v < INT_MIN + by ? INT_MIN : v - by; }
static int grow_up(int v, int by) { return v > INT_MAX - by ? INT_MAX : v + by; }

/* `f` in either format: the source pulled in that format over the grown window, then the library entry of that format */
static void median_render(PyObject *o, int frame_index, rgba_frame_dev *f) {
    py_median *self = (py_median *)o;
    py_rdlock(&self->n.lock);
    const cvs_median m = { self->radius, framefunc_get_f32(&self->threshold, frame_index), self->channels, 0 };
    const int reach = self->radius;
    box2i grown;
    box2i_set(&grown, grow_down(f->full_window.min.x, reach), grow_down(f->full_window.min.y, reach), grow_up(f->full_window.max.x, reach), grow_up(f->full_window.max.y, reach));
    rgba_frame_dev in = { NULL, f->format, grown, grown, f->stream };
    in.data = box2i_is_empty(&f->full_window) ? NULL : cvs_pool_malloc(frame_bytes(&grown, f->format), f->stream);
    if (!in.data) { pthread_rwlock_unlock(&self->n.lock); box2i_set_empty(&f->current_window); return; }
    video_get_frame_dev(self->n.source, frame_index, &in);
    int rc;
    if (f->format == CVS_FORMAT_F16) {
        rgba_frame_f16 fi = { in.data, in.full_window, in.current_window }, fo = { f->data, f->full_window, f->full_window };
        rc = cvs_median_f16_dev(&fo, &fi, &m, f->stream);
        f->current_window = fo.current_window;
    } else {
        rgba_frame_f32 fi = { in.data, in.full_window, in.current_window }, fo = { f->data, f->full_window, f->full_window };
        rc = cvs_median_f32_dev(&fo, &fi, &m, f->stream);
        f->current_window = fo.current_window;
    }
    pthread_rwlock_unlock(&self->n.lock);
    if (rc != 0) box2i_set_empty(&f->current_window);
    cvs_pool_free(in.data, f->stream);
}

DEFINE_NODE_VTABLE_HALF_DIRECT(median)                /* keys, network, codes back: one launch */

static int median_set_threshold(py_median *self, PyObject *v, void *closure) {
    if (!v || v == Py_None) { PyErr_SetString(PyExc_TypeError, "the attribute takes a value or a frame function"); return -1; }
    return node1_set_holder(&self->n, NODE1_HOLDER_AT(self, closure), v);
}
static PyObject *median_get_radius(py_median *self, void *closure) { return PyLong_FromLong(self->radius); }
static int median_set_radius(py_median *self, PyObject *v, void *closure) {
    const int radius = parse_radius(v);
    if (!radius) return -1;
    py_wrlock_nogil(&self->n.lock);
    self->radius = radius;
    pthread_rwlock_unlock(&self->n.lock);
    return 0;
}
PyObject *py_channels_string(int mask) {
    char s[5];
    int n = 0;
    for (int k = 0; k < 4; k++) if (mask & (1 << k)) s[n++] = "rgba"[k];
    return PyUnicode_FromStringAndSize(s, n);
}
static PyObject *median_get_channels(py_median *self, void *closure) { return py_channels_string(self->channels); }
static int median_set_channels(py_median *self, PyObject *v, void *closure) {
    const int mask = py_channels_parse(v);
    if (mask < 0) return -1;
    py_wrlock_nogil(&self->n.lock);
    self->channels = mask;
    pthread_rwlock_unlock(&self->n.lock);
    return 0;
}

static PyGetSetDef median_getset[] = {
    { VIDEO_FRAME_SOURCE_FUNCS, pyext_capsule_getter, NULL, "Video frame source C API.", &median_capsule },
    { "source", (getter)node1_get_source, (setter)node1_set_source_attr, "The upstream video source." },
    { "radius", (getter)median_get_radius, (setter)median_set_radius, "1: the median of 3 x 3 pixels, 2: of 5 x 5." },
    { "threshold", (getter)node1_get_scalar, (setter)median_set_threshold, "0: every pixel takes the median; > 0: only pixels that differ from it by more than this (number or frame function).", NODE1_HOLDER(py_median, threshold) },
    { "channels", (getter)median_get_channels, (setter)median_set_channels, "The channels filtered, letters from \"rgba\"; the others pass code for code." },
    { NULL }
};
static PyTypeObject py_type_Median = {
    PyVarObject_HEAD_INIT(NULL, 0)
    .tp_name = "fluggo.media.process.VideoMedianFilter", .tp_basicsize = sizeof(py_median), .tp_flags = Py_TPFLAGS_DEFAULT,
    .tp_base = &py_type_VideoSource, .tp_new = PyType_GenericNew, .tp_init = (initproc)median_init,
    .tp_dealloc = (destructor)median_dealloc, .tp_getset = median_getset, .tp_methods = node1_methods,
};

int init_median(PyObject *module) {
    if (pyext_make_capsule(&median_capsule, &median_funcs) < 0) return -1;
    return pyext_add_type(module, "VideoMedianFilter", &py_type_Median);
}
