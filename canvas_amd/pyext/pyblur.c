/*
 * pyblur.c -- the two FIR effects of fluggo.media.process: soften and sharpen a clip.
 *
 * The reference's design notes name them as the filters an editor carries ("expensive blurs", "unsharp mask":
 * docs/sphinx/feature-proposal/hints.rst:51-53,68-69); it built neither.  Contracts: DESIGN.md "A11" (blur), "Unsharp mask".
 *   VideoBlurFilter(source, taps)                                    cvs_fir_blur_f32_dev / _f16_dev
 *   VideoUnsharpMaskFilter(source, taps, amount=1.0, threshold=0.0)  cvs_unsharp_mask_f32_dev / _f16_dev
 *   gaussian_taps(sigma, ntaps=None)                                 canvas_amd.synth.gaussian_taps as a tuple
 * f32 is the nodes' own format (a workspace pulls them as f32: nothing is rounded before the over); an f16 pull over a
 * half-native source goes through the _f16_dev entry in one launch (VideoMixFilter's pattern, pysources.c).  The source is
 * pulled over the requested window grown by ntaps / 2 on every side, so a frame pulled in tiles equals the frame pulled whole.
 * Locking as in pysources.c: reader lock around the upstream pull and the tap list, writer lock where either is replaced.
 */
#include "pyext.h"
#include <limits.h>
#include <math.h>

typedef struct { node1 n; float *taps; int ntaps; bool unsharp; FrameFunctionHolder amount, threshold; } py_blur;

/* a non-empty sequence of numbers -> malloc'ed floats (NULL with a Python error set) */
static float *parse_taps(PyObject *obj, int *count) {
    if (!obj || PyUnicode_Check(obj) || PyBytes_Check(obj)) { PyErr_SetString(PyExc_TypeError, "taps must be a sequence of numbers"); return NULL; }
    PyObject *seq = PySequence_Fast(obj, "taps must be a sequence of numbers");
    if (!seq) return NULL;
    const Py_ssize_t n = PySequence_Fast_GET_SIZE(seq);
    if (n < 1) { Py_DECREF(seq); PyErr_SetString(PyExc_ValueError, "taps must hold at least one tap"); return NULL; }
    if (n > INT_MAX / 4) { Py_DECREF(seq); PyErr_SetString(PyExc_ValueError, "too many taps"); return NULL; }
    float *taps = malloc(sizeof(float) * (size_t)n);
    if (!taps) { Py_DECREF(seq); PyErr_NoMemory(); return NULL; }
    for (Py_ssize_t k = 0; k < n; k++) {
        const double v = PyFloat_AsDouble(PySequence_Fast_GET_ITEM(seq, k));
        if (v == -1.0 && PyErr_Occurred()) { free(taps); Py_DECREF(seq); return NULL; }
        taps[k] = (float)v;
    }
    Py_DECREF(seq);
    *count = (int)n;
    return taps;
}

static int blur_init_common(py_blur *self, PyObject *src, PyObject *taps_obj, PyObject *amount_obj, PyObject *threshold_obj, bool unsharp) {
    self->unsharp = unsharp;
    framefunc_init(&self->amount, 1.0, 0, 0, 0);
    framefunc_init(&self->threshold, 0.0, 0, 0, 0);
    int n = 0;
    float *taps = parse_taps(taps_obj, &n);
    if (!taps) return -1;
    free(self->taps);
    self->taps = taps; self->ntaps = n;
    if (!py_video_take_source(src, &self->n.source)) return -1;
    if (amount_obj && !py_framefunc_take_source(amount_obj, &self->amount)) return -1;
    if (threshold_obj && !py_framefunc_take_source(threshold_obj, &self->threshold)) return -1;
    return 0;
}
static int blur_init(py_blur *self, PyObject *args, PyObject *kw) {
    static char *kwlist[] = { "source", "taps", NULL };
    PyObject *src, *taps;
    pthread_rwlock_init(&self->n.lock, NULL);
    if (!PyArg_ParseTupleAndKeywords(args, kw, "OO", kwlist, &src, &taps)) return -1;
    return blur_init_common(self, src, taps, NULL, NULL, false);
}
static int unsharp_init(py_blur *self, PyObject *args, PyObject *kw) {
    static char *kwlist[] = { "source", "taps", "amount", "threshold", NULL };
    PyObject *src, *taps, *amount = NULL, *threshold = NULL;
    pthread_rwlock_init(&self->n.lock, NULL);
    if (!PyArg_ParseTupleAndKeywords(args, kw, "OO|OO", kwlist, &src, &taps, &amount, &threshold)) return -1;
    return blur_init_common(self, src, taps, amount, threshold, true);
}
static void blur_dealloc(py_blur *self) {
    py_video_take_source(NULL, &self->n.source);
    py_framefunc_take_source(NULL, &self->amount);
    py_framefunc_take_source(NULL, &self->threshold);
    free(self->taps);
    pthread_rwlock_destroy(&self->n.lock);
    Py_TYPE(self)->tp_free((PyObject *)self);
}

static int grow_down(int v, int by) { return v < INT_MIN + by ? INT_MIN : v - by; }
static int grow_up(int v, int by) { return v > INT_MAX - by ? INT_MAX : v + by; }

/* `f` in either format: the source pulled in that format over the grown window, then the library entry of that format */
static void blur_render(PyObject *o, int frame_index, rgba_frame_dev *f) {
    py_blur *self = (py_blur *)o;
    py_rdlock(&self->n.lock);
    const int c = self->ntaps / 2;
    box2i grown;
    box2i_set(&grown, grow_down(f->full_window.min.x, c), grow_down(f->full_window.min.y, c), grow_up(f->full_window.max.x, c), grow_up(f->full_window.max.y, c));
    rgba_frame_dev in = { NULL, f->format, grown, grown, f->stream };
    in.data = box2i_is_empty(&f->full_window) ? NULL : cvs_pool_malloc(frame_bytes(&grown, f->format), f->stream);
    if (!in.data) { pthread_rwlock_unlock(&self->n.lock); box2i_set_empty(&f->current_window); return; }
    video_get_frame_dev(self->n.source, frame_index, &in);
    const float amount = self->unsharp ? framefunc_get_f32(&self->amount, frame_index) : 0.0f;
    const float threshold = self->unsharp ? framefunc_get_f32(&self->threshold, frame_index) : 0.0f;
    int rc;
    if (f->format == CVS_FORMAT_F16) {
        rgba_frame_f16 fi = { in.data, in.full_window, in.current_window }, fo = { f->data, f->full_window, f->full_window };
        rc = self->unsharp ? cvs_unsharp_mask_f16_dev(&fo, &fi, self->taps, self->ntaps, amount, threshold, f->stream)
                           : cvs_fir_blur_f16_dev(&fo, &fi, self->taps, self->ntaps, f->stream);
        f->current_window = fo.current_window;
    } else {
        rgba_frame_f32 fi = { in.data, in.full_window, in.current_window }, fo = { f->data, f->full_window, f->full_window };
        rc = self->unsharp ? cvs_unsharp_mask_f32_dev(&fo, &fi, self->taps, self->ntaps, amount, threshold, f->stream)
                           : cvs_fir_blur_f32_dev(&fo, &fi, self->taps, self->ntaps, f->stream);
        f->current_window = fo.current_window;
    }
    pthread_rwlock_unlock(&self->n.lock);
    if (rc != 0) box2i_set_empty(&f->current_window);
    cvs_pool_free(in.data, f->stream);
}

DEFINE_NODE_VTABLE_HALF_DIRECT(blur)                  /* widen, both passes (and the mask), truncate: one launch */

static PyObject *blur_get_taps(py_blur *self, void *c) {
    py_rdlock(&self->n.lock);
    PyObject *t = PyTuple_New(self->ntaps);
    for (int k = 0; t && k < self->ntaps; k++) {
        PyObject *v = PyFloat_FromDouble(self->taps[k]);
        if (!v) { Py_CLEAR(t); break; }
        PyTuple_SET_ITEM(t, k, v);
    }
    pthread_rwlock_unlock(&self->n.lock);
    return t;
}
static int blur_set_taps(py_blur *self, PyObject *value, void *c) {
    int n = 0;
    float *taps = parse_taps(value, &n);
    if (!taps) return -1;
    py_wrlock_nogil(&self->n.lock);
    float *old = self->taps;
    self->taps = taps; self->ntaps = n;
    pthread_rwlock_unlock(&self->n.lock);
    free(old);
    return 0;
}
static int unsharp_set_holder(py_blur *self, PyObject *v, void *offset) {
    if (!v) { PyErr_SetString(PyExc_TypeError, "cannot delete the attribute"); return -1; }
    if (v == Py_None) { PyErr_SetString(PyExc_TypeError, "the attribute takes a number or a frame function"); return -1; }
    return node1_set_holder(&self->n, NODE1_HOLDER_AT(self, offset), v);
}

static PyGetSetDef blur_getset[] = {
    { VIDEO_FRAME_SOURCE_FUNCS, pyext_capsule_getter, NULL, "Video frame source C API.", &blur_capsule },
    { "source", (getter)node1_get_source, (setter)node1_set_source_attr, "The upstream video source." },
    { "taps", (getter)blur_get_taps, (setter)blur_set_taps, "The tap list of both passes (tuple of floats; centre ntaps // 2)." },
    { NULL }
};
static PyGetSetDef unsharp_getset[] = {
    { VIDEO_FRAME_SOURCE_FUNCS, pyext_capsule_getter, NULL, "Video frame source C API.", &blur_capsule },
    { "source", (getter)node1_get_source, (setter)node1_set_source_attr, "The upstream video source." },
    { "taps", (getter)blur_get_taps, (setter)blur_set_taps, "The tap list of the blur's two passes (tuple of floats; centre ntaps // 2)." },
    { "amount", (getter)node1_get_scalar, (setter)unsharp_set_holder, "Strength of the mask (number or frame function).", NODE1_HOLDER(py_blur, amount) },
    { "threshold", (getter)node1_get_scalar, (setter)unsharp_set_holder, "Differences smaller than this are left alone (number or frame function).", NODE1_HOLDER(py_blur, threshold) },
    { NULL }
};
static PyTypeObject py_type_Blur = {
    PyVarObject_HEAD_INIT(NULL, 0)
    .tp_name = "fluggo.media.process.VideoBlurFilter", .tp_basicsize = sizeof(py_blur), .tp_flags = Py_TPFLAGS_DEFAULT,
    .tp_base = &py_type_VideoSource, .tp_new = PyType_GenericNew, .tp_init = (initproc)blur_init,
    .tp_dealloc = (destructor)blur_dealloc, .tp_getset = blur_getset, .tp_methods = node1_methods,
};
static PyTypeObject py_type_Unsharp = {
    PyVarObject_HEAD_INIT(NULL, 0)
    .tp_name = "fluggo.media.process.VideoUnsharpMaskFilter", .tp_basicsize = sizeof(py_blur), .tp_flags = Py_TPFLAGS_DEFAULT,
    .tp_base = &py_type_VideoSource, .tp_new = PyType_GenericNew, .tp_init = (initproc)unsharp_init,
    .tp_dealloc = (destructor)blur_dealloc, .tp_getset = unsharp_getset, .tp_methods = node1_methods,
};

/* gaussian_taps(sigma, ntaps=None): the arithmetic of canvas_amd.synth.gaussian_taps itself (numpy f32), as a tuple of floats */
static PyObject *mod_gaussian_taps(PyObject *module, PyObject *args, PyObject *kw) {
    static char *kwlist[] = { "sigma", "ntaps", NULL };
    double sigma;
    PyObject *ntaps_obj = Py_None;
    if (!PyArg_ParseTupleAndKeywords(args, kw, "d|O", kwlist, &sigma, &ntaps_obj)) return NULL;
    if (!(sigma > 0.0) || !isfinite(sigma)) { PyErr_SetString(PyExc_ValueError, "sigma must be positive and finite"); return NULL; }
    long ntaps;
    if (ntaps_obj == Py_None) ntaps = 2 * (long)ceil(3.0 * sigma) + 1;
    else { ntaps = PyLong_AsLong(ntaps_obj); if (ntaps == -1 && PyErr_Occurred()) return NULL; }
    if (ntaps < 1 || ntaps > 1 << 20) { PyErr_SetString(PyExc_ValueError, "ntaps must be at least 1"); return NULL; }
    PyObject *synth = PyImport_ImportModule("canvas_amd.synth");
    if (!synth) return NULL;
    PyObject *array = PyObject_CallMethod(synth, "gaussian_taps", "ld", ntaps, sigma);
    Py_DECREF(synth);
    if (!array) return NULL;
    PyObject *list = PyObject_CallMethod(array, "tolist", NULL);
    Py_DECREF(array);
    if (!list) return NULL;
    PyObject *tuple = PySequence_Tuple(list);
    Py_DECREF(list);
    return tuple;
}
static PyMethodDef blur_functions[] = {
    { "gaussian_taps", (PyCFunction)mod_gaussian_taps, METH_VARARGS | METH_KEYWORDS,
      "gaussian_taps(sigma, ntaps=None) -> tuple of taps normalised in f32 (ntaps default: 2 * ceil(3 * sigma) + 1)" },
    { NULL }
};

int init_blur(PyObject *module) {
    if (pyext_make_capsule(&blur_capsule, &blur_funcs) < 0) return -1;
    if (pyext_add_type(module, "VideoBlurFilter", &py_type_Blur) < 0 || pyext_add_type(module, "VideoUnsharpMaskFilter", &py_type_Unsharp) < 0) return -1;
    return PyModule_AddFunctions(module, blur_functions);
}
