/*
 * pysecondary.c -- the secondaries of fluggo.media.process: a qualifier that makes a matte from hue, saturation and luma, and a
 * mix of two sources through a matte held in a third.  No reference code.  Contract: DESIGN.md "Secondaries".
 *   VideoQualifierFilter(source, hue=None, saturation=None, luma=None, key_source=None, invert=False, show_matte=False)
 *                                                                    cvs_qualify_f32_dev / _f16_dev
 *   VideoMatteMixFilter(src_a, src_b, matte, channel="a", invert=False)
 *                                                                    cvs_matte_mix_f32_dev / _f16_dev
 * hue is (center, width, softness) in degrees, saturation and luma are (low, high, soft_low, soft_high); None: the axis does not
 * qualify.  Each member is a number or a frame function.  A constant the entry would refuse raises ValueError where it is given;
 * what a frame function yields is judged by the entry at the pull, whose refusal is an empty frame and a message.
 * Both nodes render in the format asked for, f16 or f32: every source is pulled over exactly the requested window in that format,
 * the first into the frame asked for, the others into pooled scratch released on the frame's stream (VideoMixFilter's pattern,
 * pysources.c), then one call of the entry in place on the first operand.
 * Locking as in pykey.c: reader lock around the upstream pulls and the parameters, writer lock where either is replaced.
 */
#include "pyext.h"
#include "canvas_secondary.h"
#include <math.h>

static rgba_frame_dev scratch_like(const rgba_frame_dev *f) {
    rgba_frame_dev t = { NULL, f->format, f->full_window, f->full_window, f->stream };
    t.data = cvs_pool_malloc(frame_bytes(&f->full_window, f->format), f->stream);
    return t;
}

/* ---------------------------------------------------------------- VideoQualifierFilter */

enum { AXIS_HUE, AXIS_SATURATION, AXIS_LUMA, AXES, PARTS = 11 };
static const int axis_first[AXES] = { 0, 3, 7 }, axis_count[AXES] = { 3, 4, 4 };
static const char *const axis_name[AXES] = { "hue", "saturation", "luma" };
static const char *const axis_form[AXES] = { "(center, width, softness)", "(low, high, soft_low, soft_high)", "(low, high, soft_low, soft_high)" };

/* given[k]: the tuple as it was handed over (what the attribute reads back), NULL where the axis does not qualify */
typedef struct { node1 n; video_source *key; FrameFunctionHolder part[PARTS]; PyObject *given[AXES]; bool invert, show_matte; } py_qual;

static bool width_ok(float v) { return isfinite(v) && v >= 0.0f; }

/* the constants among an axis's members, judged as the entry judges them */
static bool axis_constants_ok(int k, const FrameFunctionHolder *h) {
    float v[4];
    bool given[4];
    for (int j = 0; j < axis_count[k]; j++) { given[j] = h[j].source == NULL; v[j] = (float)h[j].constant[0]; }
    bool ok;
    if (k == AXIS_HUE) ok = (!given[0] || isfinite(v[0])) && (!given[1] || width_ok(v[1])) && (!given[2] || width_ok(v[2]));
    else ok = (!given[0] || isfinite(v[0])) && (!given[1] || !isnan(v[1])) && (!given[2] || width_ok(v[2])) && (!given[3] || width_ok(v[3])) &&
              (!given[0] || !given[1] || v[1] >= v[0]);
    if (!ok) PyErr_Format(PyExc_ValueError, k == AXIS_HUE ? "%s takes a finite center and a width and softness that are finite and not negative"
                                                           : "%s takes a finite low, high >= low (inf: no upper bound) and soft widths that are finite and not negative", axis_name[k]);
    return ok;
}

/* `value` into fresh[0 .. count) and *tuple (a new reference; NULL for None): 0, or -1 with a Python error set and nothing held */
static int axis_parse(int k, PyObject *value, FrameFunctionHolder *fresh, PyObject **tuple) {
    *tuple = NULL;
    for (int j = 0; j < 4; j++) framefunc_init(&fresh[j], 0, 0, 0, 0);
    if (!value || value == Py_None) return 0;
    if (PyUnicode_Check(value) || !PySequence_Check(value)) { PyErr_Format(PyExc_TypeError, "%s takes %s or None", axis_name[k], axis_form[k]); return -1; }
    PyObject *t = PySequence_Tuple(value);
    if (!t) return -1;
    if (PyTuple_GET_SIZE(t) != axis_count[k]) {
        PyErr_Format(PyExc_ValueError, "%s takes %s, not %zd members", axis_name[k], axis_form[k], PyTuple_GET_SIZE(t));
        Py_DECREF(t);
        return -1;
    }
    bool ok = true;
    for (int j = 0; ok && j < axis_count[k]; j++) {
        PyObject *m = PyTuple_GET_ITEM(t, j);
        if (PyTuple_Check(m) || PyBool_Check(m) || !(PyNumber_Check(m) || PyObject_HasAttrString(m, FRAME_FUNCTION_FUNCS))) {
            PyErr_Format(PyExc_TypeError, "member %d of %s must be a number or a frame function", j, axis_name[k]);
            ok = false;
        } else ok = py_framefunc_take_source(m, &fresh[j]);
    }
    if (ok) ok = axis_constants_ok(k, fresh);
    if (!ok) {
        for (int j = 0; j < 4; j++) py_framefunc_take_source(NULL, &fresh[j]);
        Py_DECREF(t);
        return -1;
    }
    *tuple = t;
    return 0;
}

/* a value that is refused leaves the old one; parsed with no lock held, swapped in under the writer lock (locked: the node is alive) */
static int axis_set(py_qual *self, int k, PyObject *value, bool locked) {
    FrameFunctionHolder fresh[4], old[4];
    PyObject *tuple;
    if (axis_parse(k, value, fresh, &tuple) != 0) return -1;
    if (locked) py_wrlock_nogil(&self->n.lock);
    PyObject *before = self->given[k];
    for (int j = 0; j < axis_count[k]; j++) { old[j] = self->part[axis_first[k] + j]; self->part[axis_first[k] + j] = fresh[j]; }
    self->given[k] = tuple;
    if (locked) pthread_rwlock_unlock(&self->n.lock);
    for (int j = 0; j < axis_count[k]; j++) py_framefunc_take_source(NULL, &old[j]);
    Py_XDECREF(before);
    return 0;
}

static int qual_init(py_qual *self, PyObject *args, PyObject *kw) {
    static char *kwlist[] = { "source", "hue", "saturation", "luma", "key_source", "invert", "show_matte", NULL };
    PyObject *src, *axis[AXES] = { NULL, NULL, NULL }, *key = NULL;
    int invert = 0, show_matte = 0;
    pthread_rwlock_init(&self->n.lock, NULL);
    for (int j = 0; j < PARTS; j++) framefunc_init(&self->part[j], 0, 0, 0, 0);
    if (!PyArg_ParseTupleAndKeywords(args, kw, "O|OOOOpp", kwlist, &src, &axis[0], &axis[1], &axis[2], &key, &invert, &show_matte)) return -1;
    self->invert = invert != 0;
    self->show_matte = show_matte != 0;
    if (!py_video_take_source(src, &self->n.source)) return -1;
    if (key && !py_video_take_source(key, &self->key)) return -1;
    for (int k = 0; k < AXES; k++)
        if (axis_set(self, k, axis[k], false) != 0) return -1;
    return 0;
}
static void qual_dealloc(py_qual *self) {
    py_video_take_source(NULL, &self->n.source);
    py_video_take_source(NULL, &self->key);
    for (int j = 0; j < PARTS; j++) py_framefunc_take_source(NULL, &self->part[j]);
    for (int k = 0; k < AXES; k++) Py_CLEAR(self->given[k]);
    pthread_rwlock_destroy(&self->n.lock);
    Py_TYPE(self)->tp_free((PyObject *)self);
}

/* `f` in either format: the source pulled in that format into `f` itself, the key source into scratch, then the entry in place */
static void qual_render(PyObject *o, int frame_index, rgba_frame_dev *f) {
    py_qual *self = (py_qual *)o;
    rgba_frame_dev tk = { NULL };
    py_rdlock(&self->n.lock);
    const bool keyed = self->key != NULL;
    if (keyed) tk = scratch_like(f);
    video_get_frame_dev(self->n.source, frame_index, f);
    if (tk.data) video_get_frame_dev(self->key, frame_index, &tk);
    float v[PARTS] = { 0 };
    cvs_qualifier q = { (self->invert ? CVS_QUAL_INVERT : 0) | (self->show_matte ? CVS_QUAL_SHOW_MATTE : 0) };
    for (int k = 0; k < AXES; k++)
        if (self->given[k]) {
            q.flags |= 1u << k;                         /* CVS_QUAL_HUE, _SATURATION, _LUMA */
            for (int j = axis_first[k]; j < axis_first[k] + axis_count[k]; j++) v[j] = framefunc_get_f32(&self->part[j], frame_index);
        }
    pthread_rwlock_unlock(&self->n.lock);
    q.hue = (cvs_hue_range){ v[0], v[1], v[2] };
    q.saturation = (cvs_value_range){ v[3], v[4], v[5], v[6] };
    q.luma = (cvs_value_range){ v[7], v[8], v[9], v[10] };
    if (keyed && !tk.data) { box2i_set_empty(&f->current_window); return; }
    int rc;
    if (f->format == CVS_FORMAT_F16) {
        rgba_frame_f16 fo = { f->data, f->full_window, f->current_window }, fk = { tk.data, tk.full_window, tk.current_window };
        rc = cvs_qualify_f16_dev(&fo, &fo, keyed ? &fk : NULL, &q, f->stream);
        f->current_window = fo.current_window;
    } else {
        rgba_frame_f32 fo = { f->data, f->full_window, f->current_window }, fk = { tk.data, tk.full_window, tk.current_window };
        rc = cvs_qualify_f32_dev(&fo, &fo, keyed ? &fk : NULL, &q, f->stream);
        f->current_window = fo.current_window;
    }
    if (rc != 0) box2i_set_empty(&f->current_window);
    if (tk.data) cvs_pool_free(tk.data, f->stream);
}

/* both formats are the nodes' own: each slot renders in the format it is asked for */
#define DEFINE_NODE_VTABLE_EITHER(P)                                                                           \
    static void P##_slot_dev(PyObject *self, int i, rgba_frame_dev *f) { P##_render(self, i, f); }             \
    static void P##_slot_16(PyObject *self, int i, rgba_frame_f16 *f) { node_get_frame_host16(self, i, f, CVS_FORMAT_F16, P##_render); } \
    static void P##_slot_32(PyObject *self, int i, rgba_frame_f32 *f) { node_get_frame_host32(self, i, f, CVS_FORMAT_F32, P##_render); } \
    static video_frame_source_funcs P##_funcs = {                                                             \
        .flags = VIDEO_SOURCE_FLAG_DEVICE, .get_frame = (video_get_frame_func)P##_slot_16,                    \
        .get_frame_32 = (video_get_frame_32_func)P##_slot_32, .get_frame_dev = (video_get_frame_dev_func)P##_slot_dev }; \
    static PyObject *P##_capsule;

DEFINE_NODE_VTABLE_EITHER(qual)

static PyObject *qual_get_axis(py_qual *self, void *closure) {
    py_rdlock(&self->n.lock);
    PyObject *o = self->given[(intptr_t)closure] ? self->given[(intptr_t)closure] : Py_None;
    Py_INCREF(o);
    pthread_rwlock_unlock(&self->n.lock);
    return o;
}
static int qual_set_axis(py_qual *self, PyObject *v, void *closure) {
    if (!v) { PyErr_SetString(PyExc_TypeError, "the attribute cannot be deleted; None: the axis does not qualify"); return -1; }
    return axis_set(self, (int)(intptr_t)closure, v, true);
}
static PyObject *qual_get_key(py_qual *self, void *closure) {
    py_rdlock(&self->n.lock);
    PyObject *o = self->key ? (PyObject *)self->key->obj : Py_None;
    Py_INCREF(o);
    pthread_rwlock_unlock(&self->n.lock);
    return o;
}
/* a source attribute: `v` is taken with no lock held (a value that is refused leaves the old one), swapped in under the writer
 * lock, and what the attribute held is released after unlocking */
static int source_swap(pthread_rwlock_t *lock, video_source **slot, PyObject *v) {
    video_source *fresh = NULL;
    if (!py_video_take_source(v, &fresh)) return -1;
    py_wrlock_nogil(lock);
    video_source *old = *slot;
    *slot = fresh;
    pthread_rwlock_unlock(lock);
    py_video_take_source(NULL, &old);
    return 0;
}
static int qual_set_key(py_qual *self, PyObject *v, void *closure) { return source_swap(&self->n.lock, &self->key, v); }
/* closure: the flag's offset in py_qual */
static PyObject *qual_get_flag(py_qual *self, void *closure) { return PyBool_FromLong(*((bool *)self + (size_t)closure)); }
static int qual_set_flag(py_qual *self, PyObject *v, void *closure) {
    if (!v || !PyBool_Check(v)) { PyErr_SetString(PyExc_TypeError, "the attribute is a bool"); return -1; }
    py_wrlock_nogil(&self->n.lock);
    *((bool *)self + (size_t)closure) = v == Py_True;
    pthread_rwlock_unlock(&self->n.lock);
    return 0;
}

static PyGetSetDef qual_getset[] = {
    { VIDEO_FRAME_SOURCE_FUNCS, pyext_capsule_getter, NULL, "Video frame source C API.", &qual_capsule },
    { "source", (getter)node1_get_source, (setter)node1_set_source_attr, "The upstream video source: its colours pass, its alpha is multiplied by the matte." },
    { "key_source", (getter)qual_get_key, (setter)qual_set_key, "The source whose pixels are measured, or None: the source itself." },
    { "hue", (getter)qual_get_axis, (setter)qual_set_axis, "(center, width, softness) in degrees, each a number or a frame function, or None.", (void *)(intptr_t)AXIS_HUE },
    { "saturation", (getter)qual_get_axis, (setter)qual_set_axis, "(low, high, soft_low, soft_high) of the HSV saturation, or None.", (void *)(intptr_t)AXIS_SATURATION },
    { "luma", (getter)qual_get_axis, (setter)qual_set_axis, "(low, high, soft_low, soft_high) of the Rec.709 luma, or None.", (void *)(intptr_t)AXIS_LUMA },
    { "invert", (getter)qual_get_flag, (setter)qual_set_flag, "Select what the ranges leave out.", (void *)offsetof(py_qual, invert) },
    { "show_matte", (getter)qual_get_flag, (setter)qual_set_flag, "Show (a', a', a', 1) instead of the qualified picture.", (void *)offsetof(py_qual, show_matte) },
    { NULL }
};
static PyTypeObject py_type_Qualifier = {
    PyVarObject_HEAD_INIT(NULL, 0)
    .tp_name = "fluggo.media.process.VideoQualifierFilter", .tp_basicsize = sizeof(py_qual), .tp_flags = Py_TPFLAGS_DEFAULT,
    .tp_base = &py_type_VideoSource, .tp_new = PyType_GenericNew, .tp_init = (initproc)qual_init,
    .tp_dealloc = (destructor)qual_dealloc, .tp_getset = qual_getset, .tp_methods = node1_methods,
};

/* ---------------------------------------------------------------- VideoMatteMixFilter */

enum { MMIX_SOURCES = 3 };
typedef struct { PyObject_HEAD pthread_rwlock_t lock; video_source *src[MMIX_SOURCES]; bool luma, invert; } py_mmix;
static const pyext_choice mmix_channels[] = { { "a", 0 }, { "luma", 1 }, { NULL } };

static int mmix_init(py_mmix *self, PyObject *args, PyObject *kw) {
    static char *kwlist[] = { "src_a", "src_b", "matte", "channel", "invert", NULL };
    PyObject *src[MMIX_SOURCES], *channel = NULL;
    int invert = 0, luma;
    pthread_rwlock_init(&self->lock, NULL);
    if (!PyArg_ParseTupleAndKeywords(args, kw, "OOO|Op", kwlist, &src[0], &src[1], &src[2], &channel, &invert)) return -1;
    if (!pyext_choose("VideoMatteMixFilter", "channel", channel, mmix_channels, 0, &luma)) return -1;
    self->luma = luma != 0;
    self->invert = invert != 0;
    for (int k = 0; k < MMIX_SOURCES; k++)
        if (!py_video_take_source(src[k], &self->src[k])) return -1;
    return 0;
}
static void mmix_dealloc(py_mmix *self) {
    for (int k = 0; k < MMIX_SOURCES; k++) py_video_take_source(NULL, &self->src[k]);
    pthread_rwlock_destroy(&self->lock);
    Py_TYPE(self)->tp_free((PyObject *)self);
}

static void mmix_render(PyObject *o, int frame_index, rgba_frame_dev *f) {
    py_mmix *self = (py_mmix *)o;
    rgba_frame_dev tb = scratch_like(f), tm = scratch_like(f);
    if (!tb.data || !tm.data) {
        box2i_set_empty(&f->current_window);
        cvs_pool_free(tb.data, f->stream); cvs_pool_free(tm.data, f->stream);
        return;
    }
    py_rdlock(&self->lock);
    video_get_frame_dev(self->src[0], frame_index, f);
    video_get_frame_dev(self->src[1], frame_index, &tb);
    video_get_frame_dev(self->src[2], frame_index, &tm);
    const cvs_matte_mix p = { (self->luma ? CVS_MMIX_LUMA : 0) | (self->invert ? CVS_MMIX_INVERT : 0) };
    pthread_rwlock_unlock(&self->lock);
    int rc;
    if (f->format == CVS_FORMAT_F16) {
        rgba_frame_f16 fo = { f->data, f->full_window, f->current_window }, fb = { tb.data, tb.full_window, tb.current_window }, fm = { tm.data, tm.full_window, tm.current_window };
        rc = cvs_matte_mix_f16_dev(&fo, &fo, &fb, &fm, &p, f->stream);
        f->current_window = fo.current_window;
    } else {
        rgba_frame_f32 fo = { f->data, f->full_window, f->current_window }, fb = { tb.data, tb.full_window, tb.current_window }, fm = { tm.data, tm.full_window, tm.current_window };
        rc = cvs_matte_mix_f32_dev(&fo, &fo, &fb, &fm, &p, f->stream);
        f->current_window = fo.current_window;
    }
    if (rc != 0) box2i_set_empty(&f->current_window);
    cvs_pool_free(tb.data, f->stream); cvs_pool_free(tm.data, f->stream);
}

DEFINE_NODE_VTABLE_EITHER(mmix)

/* closure: which source */
static PyObject *mmix_get_source(py_mmix *self, void *closure) {
    py_rdlock(&self->lock);
    video_source *s = self->src[(intptr_t)closure];
    PyObject *o = s ? (PyObject *)s->obj : Py_None;
    Py_INCREF(o);
    pthread_rwlock_unlock(&self->lock);
    return o;
}
static int mmix_set_source(py_mmix *self, PyObject *v, void *closure) { return source_swap(&self->lock, &self->src[(intptr_t)closure], v); }
static PyObject *mmix_get_channel(py_mmix *self, void *closure) { return PyUnicode_FromString(self->luma ? "luma" : "a"); }
static int mmix_set_channel(py_mmix *self, PyObject *v, void *closure) {
    int luma;
    if (!v) { PyErr_SetString(PyExc_TypeError, "channel cannot be deleted"); return -1; }
    if (!pyext_choose("VideoMatteMixFilter", "channel", v, mmix_channels, 0, &luma)) return -1;
    py_wrlock_nogil(&self->lock);
    self->luma = luma != 0;
    pthread_rwlock_unlock(&self->lock);
    return 0;
}
static PyObject *mmix_get_invert(py_mmix *self, void *closure) { return PyBool_FromLong(self->invert); }
static int mmix_set_invert(py_mmix *self, PyObject *v, void *closure) {
    if (!v || !PyBool_Check(v)) { PyErr_SetString(PyExc_TypeError, "invert is a bool"); return -1; }
    py_wrlock_nogil(&self->lock);
    self->invert = v == Py_True;
    pthread_rwlock_unlock(&self->lock);
    return 0;
}

static PyGetSetDef mmix_getset[] = {
    { VIDEO_FRAME_SOURCE_FUNCS, pyext_capsule_getter, NULL, "Video frame source C API.", &mmix_capsule },
    { "src_a", (getter)mmix_get_source, (setter)mmix_set_source, "What shows where the matte is 0.", (void *)(intptr_t)0 },
    { "src_b", (getter)mmix_get_source, (setter)mmix_set_source, "What shows where the matte is 1.", (void *)(intptr_t)1 },
    { "matte", (getter)mmix_get_source, (setter)mmix_set_source, "The source whose alpha (or luma) mixes src_a and src_b.", (void *)(intptr_t)2 },
    { "channel", (getter)mmix_get_channel, (setter)mmix_set_channel, "\"a\": the matte's alpha; \"luma\": its Rec.709 luma." },
    { "invert", (getter)mmix_get_invert, (setter)mmix_set_invert, "Mix by 1 - k." },
    { NULL }
};
static PyTypeObject py_type_MatteMix = {
    PyVarObject_HEAD_INIT(NULL, 0)
    .tp_name = "fluggo.media.process.VideoMatteMixFilter", .tp_basicsize = sizeof(py_mmix), .tp_flags = Py_TPFLAGS_DEFAULT,
    .tp_base = &py_type_VideoSource, .tp_new = PyType_GenericNew, .tp_init = (initproc)mmix_init,
    .tp_dealloc = (destructor)mmix_dealloc, .tp_getset = mmix_getset,
};

int init_secondary(PyObject *module) {
    if (pyext_make_capsule(&qual_capsule, &qual_funcs) < 0 || pyext_make_capsule(&mmix_capsule, &mmix_funcs) < 0) return -1;
    if (pyext_add_type(module, "VideoQualifierFilter", &py_type_Qualifier) < 0) return -1;
    return pyext_add_type(module, "VideoMatteMixFilter", &py_type_MatteMix);
}
