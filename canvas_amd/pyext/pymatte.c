/*
 * pymatte.c -- the matte controls of fluggo.media.process that follow a keyer: clip, choke and feather of the alpha channel.
 *
 * No reference code (VideoChromaKeyFilter's notes, pykey.c, name the keyer only).  Contract: DESIGN.md "Matte refine".
 *   VideoMatteFilter(source, choke=0, feather=None, black=0.0, white=1.0, show_matte=False)
 *                                                                    cvs_matte_refine_f32_dev / _f16_dev
 * f32 is the node's own format (a workspace pulls it as f32: nothing is rounded before the over); an f16 pull over a
 * half-native source goes through the _f16_dev entry in one launch (pyblur.c, pykey.c).  The source is pulled over the requested
 * window grown by |choke| + ntaps / 2 on every side into a pooled frame, so a frame pulled in tiles equals the frame pulled whole;
 * the entry then writes the frame asked for.  choke, black and white are numbers or frame functions, the feather a fixed tap
 * list.  Locking as in pyblur.c: reader lock around the upstream pull and the parameters, writer lock where either is replaced.
 */
#include "pyext.h"
#include <limits.h>
#include <math.h>

typedef struct { node1 n; FrameFunctionHolder choke, black, white; float *taps; int ntaps; bool show_matte; } py_matte;

/* None -> no feather (*count = 0, NULL, no error); else an odd count of 1..CVS_MATTE_MAX_TAPS finite numbers -> malloc'ed floats
 * (NULL with a Python error set) */
static float *parse_feather(PyObject *obj, int *count, bool *ok) {
    *count = 0;
    *ok = true;
    if (!obj || obj == Py_None) return NULL;
    *ok = false;
    if (PyUnicode_Check(obj) || PyBytes_Check(obj)) { PyErr_SetString(PyExc_TypeError, "feather must be None or a sequence of numbers"); return NULL; }
    PyObject *seq = PySequence_Fast(obj, "feather must be None or a sequence of numbers");
    if (!seq) return NULL;
    const Py_ssize_t n = PySequence_Fast_GET_SIZE(seq);
    if (n < 1 || n > CVS_MATTE_MAX_TAPS || !(n & 1)) {
        Py_DECREF(seq);
        PyErr_Format(PyExc_ValueError, "feather takes an odd count of 1 to %d taps", CVS_MATTE_MAX_TAPS);
        return NULL;
    }
    float *taps = malloc(sizeof(float) * (size_t)n);
    if (!taps) { Py_DECREF(seq); PyErr_NoMemory(); return NULL; }
    for (Py_ssize_t k = 0; k < n; k++) {
        const double v = PyFloat_AsDouble(PySequence_Fast_GET_ITEM(seq, k));
        if (v == -1.0 && PyErr_Occurred()) { free(taps); Py_DECREF(seq); return NULL; }
        taps[k] = (float)v;
        if (!isfinite(taps[k])) { free(taps); Py_DECREF(seq); PyErr_SetString(PyExc_ValueError, "feather taps must be finite"); return NULL; }
    }
    Py_DECREF(seq);
    *count = (int)n;
    *ok = true;
    return taps;
}

static int matte_init(py_matte *self, PyObject *args, PyObject *kw) {
    static char *kwlist[] = { "source", "choke", "feather", "black", "white", "show_matte", NULL };
    PyObject *src, *choke = NULL, *feather = NULL, *black = NULL, *white = NULL;
    int show_matte = 0;
    pthread_rwlock_init(&self->n.lock, NULL);
    framefunc_init(&self->choke, 0.0, 0, 0, 0);
    framefunc_init(&self->black, 0.0, 0, 0, 0);
    framefunc_init(&self->white, 1.0, 0, 0, 0);
    if (!PyArg_ParseTupleAndKeywords(args, kw, "O|OOOOp", kwlist, &src, &choke, &feather, &black, &white, &show_matte)) return -1;
    self->show_matte = show_matte != 0;
    int n = 0;
    bool ok;
    float *taps = parse_feather(feather, &n, &ok);
    if (!ok) return -1;
    free(self->taps);
    self->taps = taps; self->ntaps = n;
    if (!py_video_take_source(src, &self->n.source)) return -1;
    if (choke && (choke == Py_None || !py_framefunc_take_source(choke, &self->choke))) { if (!PyErr_Occurred()) PyErr_SetString(PyExc_TypeError, "choke takes a number or a frame function"); return -1; }
    if (black && (black == Py_None || !py_framefunc_take_source(black, &self->black))) { if (!PyErr_Occurred()) PyErr_SetString(PyExc_TypeError, "black takes a number or a frame function"); return -1; }
    if (white && (white == Py_None || !py_framefunc_take_source(white, &self->white))) { if (!PyErr_Occurred()) PyErr_SetString(PyExc_TypeError, "white takes a number or a frame function"); return -1; }
    return 0;
}
static void matte_dealloc(py_matte *self) {
    py_video_take_source(NULL, &self->n.source);
    py_framefunc_take_source(NULL, &self->choke);
    py_framefunc_take_source(NULL, &self->black);
    py_framefunc_take_source(NULL, &self->white);
    free(self->taps);
    pthread_rwlock_destroy(&self->n.lock);
    Py_TYPE(self)->tp_free((PyObject *)self);
}

static int grow_down(int v, int by) { return v < INT_MIN + by ? INT_MIN : v - by; }
static int grow_up(int v, int by) { return v > INT_MAX - by ? INT_MAX : v + by; }

/* `f` in either format: the source pulled in that format over the grown window, then the library entry of that format */
static void matte_render(PyObject *o, int frame_index, rgba_frame_dev *f) {
    py_matte *self = (py_matte *)o;
    py_rdlock(&self->n.lock);
    const cvs_matte m = { framefunc_get_f32(&self->black, frame_index), framefunc_get_f32(&self->white, frame_index),
                          framefunc_get_i32(&self->choke, frame_index), self->ntaps, self->taps, self->show_matte ? CVS_MATTE_SHOW : 0 };
    /* a choke the entry will refuse grows nothing: the entry is still called, for its message */
    const bool legal = m.choke >= -CVS_MATTE_MAX_CHOKE && m.choke <= CVS_MATTE_MAX_CHOKE;
    const int reach = legal ? abs(m.choke) + self->ntaps / 2 : 0;
    box2i grown;
    box2i_set(&grown, grow_down(f->full_window.min.x, reach), grow_down(f->full_window.min.y, reach), grow_up(f->full_window.max.x, reach), grow_up(f->full_window.max.y, reach));
    rgba_frame_dev in = { NULL, f->format, grown, grown, f->stream };
    box2i_set_empty(&in.current_window);
    if (legal) {
        in.data = box2i_is_empty(&f->full_window) ? NULL : cvs_pool_malloc(frame_bytes(&grown, f->format), f->stream);
        if (!in.data) { pthread_rwlock_unlock(&self->n.lock); box2i_set_empty(&f->current_window); return; }
        in.current_window = grown;
        video_get_frame_dev(self->n.source, frame_index, &in);
    }
    int rc;
    if (f->format == CVS_FORMAT_F16) {
        rgba_frame_f16 fi = { in.data, in.full_window, in.current_window }, fo = { f->data, f->full_window, f->full_window };
        rc = cvs_matte_refine_f16_dev(&fo, &fi, &m, f->stream);
        f->current_window = fo.current_window;
    } else {
        rgba_frame_f32 fi = { in.data, in.full_window, in.current_window }, fo = { f->data, f->full_window, f->full_window };
        rc = cvs_matte_refine_f32_dev(&fo, &fi, &m, f->stream);
        f->current_window = fo.current_window;
    }
    pthread_rwlock_unlock(&self->n.lock);
    if (rc != 0) box2i_set_empty(&f->current_window);
    if (in.data) cvs_pool_free(in.data, f->stream);
}

DEFINE_NODE_VTABLE_HALF_DIRECT(matte)                 /* widen, every stage, truncate: one launch */

static PyObject *matte_get_choke(py_matte *self, void *closure) {       /* a count of pixels: read back as an int */
    if (self->choke.source) { Py_INCREF(self->choke.source); return self->choke.source; }
    return PyLong_FromLong(lround(self->choke.constant[0]));
}
/* closure: the holder's offset in py_matte */
static int matte_set_holder(py_matte *self, PyObject *v, void *closure) {
    if (!v || v == Py_None) { PyErr_SetString(PyExc_TypeError, "the attribute takes a value or a frame function"); return -1; }
    return node1_set_holder(&self->n, NODE1_HOLDER_AT(self, closure), v);
}
static PyObject *matte_get_feather(py_matte *self, void *closure) {
    py_rdlock(&self->n.lock);
    PyObject *t = NULL;
    if (self->ntaps == 0) { t = Py_None; Py_INCREF(t); }
    else t = PyTuple_New(self->ntaps);
    for (int k = 0; t && k < self->ntaps; k++) {
        PyObject *v = PyFloat_FromDouble(self->taps[k]);
        if (!v) { Py_CLEAR(t); break; }
        PyTuple_SET_ITEM(t, k, v);
    }
    pthread_rwlock_unlock(&self->n.lock);
    return t;
}
static int matte_set_feather(py_matte *self, PyObject *value, void *closure) {
    if (!value) { PyErr_SetString(PyExc_TypeError, "cannot delete the attribute"); return -1; }
    int n = 0;
    bool ok;
    float *taps = parse_feather(value, &n, &ok);
    if (!ok) return -1;
    py_wrlock_nogil(&self->n.lock);
    float *old = self->taps;
    self->taps = taps; self->ntaps = n;
    pthread_rwlock_unlock(&self->n.lock);
    free(old);
    return 0;
}
static PyObject *matte_get_show(py_matte *self, void *closure) { return PyBool_FromLong(self->show_matte); }
static int matte_set_show(py_matte *self, PyObject *v, void *closure) {
    if (!v || !PyBool_Check(v)) { PyErr_SetString(PyExc_TypeError, "show_matte is a bool"); return -1; }
    py_wrlock_nogil(&self->n.lock);
    self->show_matte = v == Py_True;
    pthread_rwlock_unlock(&self->n.lock);
    return 0;
}

#define MATTE_HOLDER(member) NODE1_HOLDER(py_matte, member)
static PyGetSetDef matte_getset[] = {
    { VIDEO_FRAME_SOURCE_FUNCS, pyext_capsule_getter, NULL, "Video frame source C API.", &matte_capsule },
    { "source", (getter)node1_get_source, (setter)node1_set_source_attr, "The upstream video source." },
    { "choke", (getter)matte_get_choke, (setter)matte_set_holder, "Pixels to shrink (> 0) or grow (< 0) the matte by, at most 16 (number or frame function).", MATTE_HOLDER(choke) },
    { "feather", (getter)matte_get_feather, (setter)matte_set_feather, "The tap list that blurs the matte (an odd count of up to 25 floats, centre ntaps // 2) or None." },
    { "black", (getter)node1_get_scalar, (setter)matte_set_holder, "Alpha at or below this becomes 0 (number or frame function).", MATTE_HOLDER(black) },
    { "white", (getter)node1_get_scalar, (setter)matte_set_holder, "Alpha at or above this becomes 1 (number or frame function).", MATTE_HOLDER(white) },
    { "show_matte", (getter)matte_get_show, (setter)matte_set_show, "Show (a, a, a, 1) of the refined matte instead of the picture." },
    { NULL }
};
static PyTypeObject py_type_Matte = {
    PyVarObject_HEAD_INIT(NULL, 0)
    .tp_name = "fluggo.media.process.VideoMatteFilter", .tp_basicsize = sizeof(py_matte), .tp_flags = Py_TPFLAGS_DEFAULT,
    .tp_base = &py_type_VideoSource, .tp_new = PyType_GenericNew, .tp_init = (initproc)matte_init,
    .tp_dealloc = (destructor)matte_dealloc, .tp_getset = matte_getset, .tp_methods = node1_methods,
};

int init_matte(PyObject *module) {
    if (pyext_make_capsule(&matte_capsule, &matte_funcs) < 0) return -1;
    return pyext_add_type(module, "VideoMatteFilter", &py_type_Matte);
}
