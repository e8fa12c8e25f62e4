/*
 * pykey.c -- the keyer of fluggo.media.process: alpha from a picture's distance to a key colour, with spill suppression.
 *
 * The reference's design notes name "Chromakey effects" next to the unsharp mask and the expensive blurs
 * (docs/sphinx/feature-proposal/hints.rst:53,69,70); it built none of them.  Contract: DESIGN.md "Chroma key".
 *   VideoChromaKeyFilter(source, key, tolerance=0.1, softness=0.1, spill=0.0, spill_range=0.0, show_matte=False)
 *                                                                    cvs_chroma_key_f32_dev / _f16_dev
 * f32 is the node's own format (a workspace pulls it as f32: nothing is rounded before the over); an f16 pull over a
 * half-native source goes through the _f16_dev entry in one launch (VideoMixFilter's pattern, pysources.c; pyblur.c).  The
 * source is pulled over exactly the requested window, into the frame asked for, and keyed there in place.
 * Locking as in pyblur.c: reader lock around the upstream pull and the parameters, writer lock where either is replaced.
 */
#include "pyext.h"

typedef struct { node1 n; FrameFunctionHolder key, tolerance, softness, spill, spill_range; bool show_matte; } py_key;

static int key_init(py_key *self, PyObject *args, PyObject *kw) {
    static char *kwlist[] = { "source", "key", "tolerance", "softness", "spill", "spill_range", "show_matte", NULL };
    PyObject *src, *key, *tolerance = NULL, *softness = NULL, *spill = NULL, *spill_range = NULL;
    int show_matte = 0;
    pthread_rwlock_init(&self->n.lock, NULL);
    framefunc_init(&self->key, 0, 0, 0, 0);
    framefunc_init(&self->tolerance, 0.1, 0, 0, 0);
    framefunc_init(&self->softness, 0.1, 0, 0, 0);
    framefunc_init(&self->spill, 0.0, 0, 0, 0);
    framefunc_init(&self->spill_range, 0.0, 0, 0, 0);
    if (!PyArg_ParseTupleAndKeywords(args, kw, "OO|OOOOp", kwlist, &src, &key, &tolerance, &softness, &spill, &spill_range, &show_matte)) return -1;
    self->show_matte = show_matte != 0;
    if (key == Py_None) { PyErr_SetString(PyExc_TypeError, "key must be an rgba tuple or a frame function"); return -1; }
    if (!py_video_take_source(src, &self->n.source)) return -1;
    if (!py_framefunc_take_source(key, &self->key)) return -1;
    if (tolerance && !py_framefunc_take_source(tolerance, &self->tolerance)) return -1;
    if (softness && !py_framefunc_take_source(softness, &self->softness)) return -1;
    if (spill && !py_framefunc_take_source(spill, &self->spill)) return -1;
    if (spill_range && !py_framefunc_take_source(spill_range, &self->spill_range)) return -1;
    return 0;
}
static void key_dealloc(py_key *self) {
    py_video_take_source(NULL, &self->n.source);
    py_framefunc_take_source(NULL, &self->key);
    py_framefunc_take_source(NULL, &self->tolerance);
    py_framefunc_take_source(NULL, &self->softness);
    py_framefunc_take_source(NULL, &self->spill);
    py_framefunc_take_source(NULL, &self->spill_range);
    pthread_rwlock_destroy(&self->n.lock);
    Py_TYPE(self)->tp_free((PyObject *)self);
}

/* `f` in either format: the source pulled in that format into `f` itself, then the library entry of that format in place */
static void key_render(PyObject *o, int frame_index, rgba_frame_dev *f) {
    py_key *self = (py_key *)o;
    py_rdlock(&self->n.lock);
    video_get_frame_dev(self->n.source, frame_index, f);
    rgba_f32 color;
    framefunc_get_rgba_f32(&color, &self->key, frame_index);        /* its alpha is ignored */
    const cvs_chroma_key key = {
        { color.r, color.g, color.b }, framefunc_get_f32(&self->tolerance, frame_index), framefunc_get_f32(&self->softness, frame_index),
        framefunc_get_f32(&self->spill, frame_index), framefunc_get_f32(&self->spill_range, frame_index), self->show_matte ? CVS_KEY_SHOW_MATTE : 0 };
    pthread_rwlock_unlock(&self->n.lock);
    if (f->format == CVS_FORMAT_F16) {
        rgba_frame_f16 fo = { f->data, f->full_window, f->current_window };
        cvs_chroma_key_f16_dev(&fo, &fo, &key, f->stream);
        f->current_window = fo.current_window;
    } else {
        rgba_frame_f32 fo = { f->data, f->full_window, f->current_window };
        cvs_chroma_key_f32_dev(&fo, &fo, &key, f->stream);
        f->current_window = fo.current_window;
    }
}

DEFINE_NODE_VTABLE_HALF_DIRECT(key)                   /* widen, key, truncate: one launch */

static PyObject *key_get_key(py_key *self, void *closure) {
    FrameFunctionHolder *h = &self->key;
    if (h->source) { Py_INCREF(h->source); return h->source; }
    rgba_f32 color = { (float)h->constant[0], (float)h->constant[1], (float)h->constant[2], (float)h->constant[3] };
    return py_make_rgba_f32(&color);
}
/* closure: the holder's offset in py_key */
static int key_set_holder(py_key *self, PyObject *v, void *closure) {
    if (!v || v == Py_None) { PyErr_SetString(PyExc_TypeError, "the attribute takes a value or a frame function"); return -1; }
    return node1_set_holder(&self->n, NODE1_HOLDER_AT(self, closure), v);
}
static PyObject *key_get_matte(py_key *self, void *closure) { return PyBool_FromLong(self->show_matte); }
static int key_set_matte(py_key *self, PyObject *v, void *closure) {
    if (!v || !PyBool_Check(v)) { PyErr_SetString(PyExc_TypeError, "show_matte is a bool"); return -1; }
    py_wrlock_nogil(&self->n.lock);
    self->show_matte = v == Py_True;
    pthread_rwlock_unlock(&self->n.lock);
    return 0;
}

#define KEY_HOLDER(member) NODE1_HOLDER(py_key, member)
static PyGetSetDef key_getset[] = {
    { VIDEO_FRAME_SOURCE_FUNCS, pyext_capsule_getter, NULL, "Video frame source C API.", &key_capsule },
    { "source", (getter)node1_get_source, (setter)node1_set_source_attr, "The upstream video source." },
    { "key", (getter)key_get_key, (setter)key_set_holder, "The colour to remove (rgba or frame function; alpha ignored).", KEY_HOLDER(key) },
    { "tolerance", (getter)node1_get_scalar, (setter)key_set_holder, "Chroma distance up to which a pixel is removed entirely (number or frame function).", KEY_HOLDER(tolerance) },
    { "softness", (getter)node1_get_scalar, (setter)key_set_holder, "Width of the ramp from removed to kept beyond tolerance; 0: a hard edge (number or frame function).", KEY_HOLDER(softness) },
    { "spill", (getter)node1_get_scalar, (setter)key_set_holder, "Strength of the spill suppression, 0..1 (number or frame function).", KEY_HOLDER(spill) },
    { "spill_range", (getter)node1_get_scalar, (setter)key_set_holder, "Distance beyond tolerance over which the suppression fades to none (number or frame function).", KEY_HOLDER(spill_range) },
    { "show_matte", (getter)key_get_matte, (setter)key_set_matte, "Show (a', a', a', 1) instead of the keyed picture." },
    { NULL }
};
static PyTypeObject py_type_ChromaKey = {
    PyVarObject_HEAD_INIT(NULL, 0)
    .tp_name = "fluggo.media.process.VideoChromaKeyFilter", .tp_basicsize = sizeof(py_key), .tp_flags = Py_TPFLAGS_DEFAULT,
    .tp_base = &py_type_VideoSource, .tp_new = PyType_GenericNew, .tp_init = (initproc)key_init,
    .tp_dealloc = (destructor)key_dealloc, .tp_getset = key_getset, .tp_methods = node1_methods,
};

int init_key(PyObject *module) {
    if (pyext_make_capsule(&key_capsule, &key_funcs) < 0) return -1;
    return pyext_add_type(module, "VideoChromaKeyFilter", &py_type_ChromaKey);
}
