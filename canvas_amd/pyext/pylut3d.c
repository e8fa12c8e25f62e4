/*
 * pylut3d.c -- the 3D colour LUT of fluggo.media.process: a lattice of N x N x N colours applied by tetrahedral interpolation.
 *
 * No reference code: the reference's only colour node is the gain/offset filter.  Contract: DESIGN.md "3D LUT".
 *   Lut3D(size, table, domain_min=(0, 0, 0), domain_max=(1, 1, 1))     an immutable value: the packed host lattice (cvs_lut3d_pack)
 *   VideoLut3DFilter(source, lut)                                      cvs_lut3d_f32_dev / _f16_dev
 * f32 is the node's own format (a workspace pulls it as f32: nothing is rounded before the over); an f16 pull over a
 * half-native source goes through the _f16_dev entry in place in one launch (pykey.c's pattern).
 *
 * The node keeps one device copy of the lattice per device context (a VideoPullQueue(devices=...) pulls one node from several).
 * A copy is made on first use in a context: cvs_malloc, the upload on the pull's stream, and one wait for that stream before
 * the pointer is published, because the context's other threads run on streams of their own.  Copies are made under `copies_lock`
 * with the node's reader lock held; the reader lock is held until the launch is enqueued, so whoever holds the writer lock finds no
 * pull between "pointer read" and "kernel queued".  Replacing the lattice (or the node's death) takes the copies away under the
 * writer lock and frees them after it: cvs_free waits for the calling thread's device before it frees, so the thread binds itself
 * to the copy's context for that call (cvs_set_context) and then back to the context it was in.
 */
#include "pyext.h"
#include "canvas_lut3d.h"
#include <math.h>

enum { LUT_CONTEXTS = 64 };             /* context ids are 0 .. 63 (canvas_hip.h) */

/* ---------------------------------------------------------------- Lut3D */

typedef struct { PyObject_HEAD cvs_lut3d p; float *nodes; size_t bytes; } py_lut;
static PyTypeObject py_type_Lut3D;

static int table_values(PyObject *table, float *rgb, size_t want) {
    Py_buffer view;
    if (PyObject_CheckBuffer(table) && PyObject_GetBuffer(table, &view, PyBUF_FORMAT | PyBUF_C_CONTIGUOUS) == 0) {
        const char *fmt = view.format ? view.format : "B";
        if (*fmt == '@' || *fmt == '=' || *fmt == '<') fmt++;
        const bool f32 = strcmp(fmt, "f") == 0, f64 = strcmp(fmt, "d") == 0;
        if (f32 || f64) {
            const size_t have = (size_t)view.len / (size_t)view.itemsize;
            if (have != want) {
                PyBuffer_Release(&view);
                PyErr_Format(PyExc_ValueError, "table holds %zu values, a lattice of that size takes %zu", have, want);
                return -1;
            }
            for (size_t k = 0; k < want; k++) rgb[k] = f32 ? ((const float *)view.buf)[k] : (float)((const double *)view.buf)[k];
            PyBuffer_Release(&view);
            return 0;
        }
        PyBuffer_Release(&view);
    }
    PyErr_Clear();
    PyObject *seq = PySequence_Fast(table, "table must be a buffer of floats or a sequence of numbers");
    if (!seq) return -1;
    const size_t have = (size_t)PySequence_Fast_GET_SIZE(seq);
    if (have != want) {
        Py_DECREF(seq);
        PyErr_Format(PyExc_ValueError, "table holds %zu values, a lattice of that size takes %zu", have, want);
        return -1;
    }
    for (size_t k = 0; k < want; k++) {
        const double v = PyFloat_AsDouble(PySequence_Fast_GET_ITEM(seq, (Py_ssize_t)k));
        if (v == -1.0 && PyErr_Occurred()) { Py_DECREF(seq); return -1; }
        rgb[k] = (float)v;
    }
    Py_DECREF(seq);
    return 0;
}

static int lut_init(py_lut *self, PyObject *args, PyObject *kw) {
    static char *kwlist[] = { "size", "table", "domain_min", "domain_max", NULL };
    int size;
    PyObject *table;
    float lo[3] = { 0.0f, 0.0f, 0.0f }, hi[3] = { 1.0f, 1.0f, 1.0f };
    if (self->nodes) { PyErr_SetString(PyExc_TypeError, "a Lut3D is immutable"); return -1; }
    if (!PyArg_ParseTupleAndKeywords(args, kw, "iO|(fff)(fff)", kwlist, &size, &table, &lo[0], &lo[1], &lo[2], &hi[0], &hi[1], &hi[2])) return -1;
    const size_t bytes = cvs_lut3d_bytes(size);
    if (bytes == 0) { PyErr_SetString(PyExc_ValueError, cvs_last_error()); return -1; }
    for (int c = 0; c < 3; c++)
        if (!isfinite(lo[c]) || !isfinite(hi[c]) || !(lo[c] < hi[c])) {
            char msg[160];
            snprintf(msg, sizeof msg, "domain %g..%g of channel %d must be finite and ascending", lo[c], hi[c], c);
            PyErr_SetString(PyExc_ValueError, msg);
            return -1;
        }
    const size_t want = bytes / 16 * 3;
    float *rgb = malloc(want * sizeof(float)), *nodes = malloc(bytes);
    if (!rgb || !nodes) { free(rgb); free(nodes); PyErr_NoMemory(); return -1; }
    if (table_values(table, rgb, want) != 0) { free(rgb); free(nodes); return -1; }
    if (cvs_lut3d_pack(nodes, rgb, size) != 0) { free(rgb); free(nodes); PyErr_SetString(PyExc_ValueError, cvs_last_error()); return -1; }
    free(rgb);
    self->p.size = size;
    memcpy(self->p.domain_min, lo, sizeof lo);
    memcpy(self->p.domain_max, hi, sizeof hi);
    self->p.flags = 0;
    self->nodes = nodes;
    self->bytes = bytes;
    return 0;
}
static void lut_dealloc(py_lut *self) {
    free(self->nodes);
    Py_TYPE(self)->tp_free((PyObject *)self);
}
static PyObject *lut_get_size(py_lut *self, void *closure) { return PyLong_FromLong(self->p.size); }
static PyObject *lut_get_domain(py_lut *self, void *closure) {
    const float *d = closure ? self->p.domain_max : self->p.domain_min;
    return Py_BuildValue("(ddd)", (double)d[0], (double)d[1], (double)d[2]);
}
/* the lattice as it was given: N^3 * 3 native floats, red fastest */
static PyObject *lut_get_table(py_lut *self, void *closure) {
    const size_t nodes = self->bytes / 16;
    PyObject *out = PyBytes_FromStringAndSize(NULL, (Py_ssize_t)(nodes * 3 * sizeof(float)));
    if (!out) return NULL;
    float *rgb = (float *)PyBytes_AS_STRING(out);
    for (size_t k = 0; k < nodes; k++) memcpy(rgb + 3 * k, self->nodes + 4 * k, 3 * sizeof(float));
    return out;
}
static PyGetSetDef lut_getset[] = {
    { "size", (getter)lut_get_size, NULL, "Nodes along each axis (2..65)." },
    { "domain_min", (getter)lut_get_domain, NULL, "The colour of lattice index 0, per channel.", NULL },
    { "domain_max", (getter)lut_get_domain, NULL, "The colour of lattice index size-1, per channel.", (void *)1 },
    { "table", (getter)lut_get_table, NULL, "The lattice as bytes: size^3 * 3 native floats, red fastest." },
    { NULL }
};
static PyTypeObject py_type_Lut3D = {
    PyVarObject_HEAD_INIT(NULL, 0)
    .tp_name = "fluggo.media.process.Lut3D", .tp_basicsize = sizeof(py_lut), .tp_flags = Py_TPFLAGS_DEFAULT,
    .tp_new = PyType_GenericNew, .tp_init = (initproc)lut_init, .tp_dealloc = (destructor)lut_dealloc, .tp_getset = lut_getset,
    .tp_doc = "Lut3D(size, table, domain_min=(0, 0, 0), domain_max=(1, 1, 1)): an immutable 3D colour lookup table; table: size^3 * 3 floats, red fastest (.cube order)",
};

/* ---------------------------------------------------------------- VideoLut3DFilter */

typedef struct { node1 n; py_lut *lut; pthread_mutex_t copies_lock; float *copies[LUT_CONTEXTS]; } py_lut_node;

/* frees copies taken out of a node (no lock needed: nobody else sees `copies`); the GIL may or may not be held */
static void free_copies(float **copies) {
    for (int ctx = 0; ctx < LUT_CONTEXTS; ctx++) {
        if (!copies[ctx]) continue;
        const int here = cvs_current_context();
        if (here != ctx && cvs_set_context(ctx) == -2) continue;          /* (a context is never closed: not reached) */
        cvs_free(copies[ctx]);
        if (here != ctx) cvs_set_context(here);
        copies[ctx] = NULL;
    }
}

/* the lattice's copy in the calling thread's context, made on first use; the node's reader lock is held.  NULL with the library's error set */
static const float *copy_here(py_lut_node *self, cvs_stream_t stream) {
    const int ctx = cvs_current_context();
    if (ctx < 0 || ctx >= LUT_CONTEXTS) return NULL;
    pthread_mutex_lock(&self->copies_lock);
    float *dev = self->copies[ctx];
    if (!dev) {
        dev = cvs_malloc(self->lut->bytes);
        if (dev && (cvs_memcpy_h2d(dev, self->lut->nodes, self->lut->bytes, stream) != 0 || cvs_stream_sync(stream) != 0)) { cvs_free(dev); dev = NULL; }
        self->copies[ctx] = dev;
    }
    pthread_mutex_unlock(&self->copies_lock);
    return dev;
}

static int lutnode_init(py_lut_node *self, PyObject *args, PyObject *kw) {
    static char *kwlist[] = { "source", "lut", NULL };
    PyObject *src, *lut;
    pthread_rwlock_init(&self->n.lock, NULL);
    pthread_mutex_init(&self->copies_lock, NULL);
    if (!PyArg_ParseTupleAndKeywords(args, kw, "OO", kwlist, &src, &lut)) return -1;
    if (!PyObject_TypeCheck(lut, &py_type_Lut3D)) { PyErr_SetString(PyExc_TypeError, "lut must be a Lut3D"); return -1; }
    if (!py_video_take_source(src, &self->n.source)) return -1;
    Py_INCREF(lut);
    self->lut = (py_lut *)lut;
    return 0;
}
static void lutnode_dealloc(py_lut_node *self) {
    py_video_take_source(NULL, &self->n.source);
    free_copies(self->copies);
    Py_XDECREF(self->lut);
    pthread_mutex_destroy(&self->copies_lock);
    pthread_rwlock_destroy(&self->n.lock);
    Py_TYPE(self)->tp_free((PyObject *)self);
}

/* `f` in either format: the source pulled in that format into `f` itself, then the library entry of that format in place */
static void lutnode_render(PyObject *o, int frame_index, rgba_frame_dev *f) {
    py_lut_node *self = (py_lut_node *)o;
    py_rdlock(&self->n.lock);
    video_get_frame_dev(self->n.source, frame_index, f);
    const float *lattice = (self->lut && !box2i_is_empty(&f->current_window)) ? copy_here(self, f->stream) : NULL;
    if (!lattice) {
        box2i_set_empty(&f->current_window);
    } else if (f->format == CVS_FORMAT_F16) {
        rgba_frame_f16 fo = { f->data, f->full_window, f->current_window };
        cvs_lut3d_f16_dev(&fo, &fo, lattice, &self->lut->p, f->stream);
        f->current_window = fo.current_window;
    } else {
        rgba_frame_f32 fo = { f->data, f->full_window, f->current_window };
        cvs_lut3d_f32_dev(&fo, &fo, lattice, &self->lut->p, f->stream);
        f->current_window = fo.current_window;
    }
    pthread_rwlock_unlock(&self->n.lock);               /* only now: the launch that reads the copy is queued */
}

DEFINE_NODE_VTABLE_HALF_DIRECT(lutnode)               /* widen, look up, truncate: one launch */

static PyObject *lutnode_get_lut(py_lut_node *self, void *closure) { Py_INCREF(self->lut); return (PyObject *)self->lut; }
static int lutnode_set_lut(py_lut_node *self, PyObject *v, void *closure) {
    if (!v || !PyObject_TypeCheck(v, &py_type_Lut3D)) { PyErr_SetString(PyExc_TypeError, "lut must be a Lut3D"); return -1; }
    float *old_copies[LUT_CONTEXTS];
    Py_INCREF(v);
    py_wrlock_nogil(&self->n.lock);
    py_lut *old = self->lut;
    self->lut = (py_lut *)v;
    memcpy(old_copies, self->copies, sizeof old_copies);
    memset(self->copies, 0, sizeof self->copies);
    pthread_rwlock_unlock(&self->n.lock);
    Py_BEGIN_ALLOW_THREADS
    free_copies(old_copies);                            /* waits for each copy's device: what was queued on it has run */
    Py_END_ALLOW_THREADS
    Py_DECREF(old);
    return 0;
}

static PyGetSetDef lutnode_getset[] = {
    { VIDEO_FRAME_SOURCE_FUNCS, pyext_capsule_getter, NULL, "Video frame source C API.", &lutnode_capsule },
    { "source", (getter)node1_get_source, (setter)node1_set_source_attr, "The upstream video source." },
    { "lut", (getter)lutnode_get_lut, (setter)lutnode_set_lut, "The Lut3D applied to the source's colours." },
    { NULL }
};
static PyTypeObject py_type_Lut3DFilter = {
    PyVarObject_HEAD_INIT(NULL, 0)
    .tp_name = "fluggo.media.process.VideoLut3DFilter", .tp_basicsize = sizeof(py_lut_node), .tp_flags = Py_TPFLAGS_DEFAULT,
    .tp_base = &py_type_VideoSource, .tp_new = PyType_GenericNew, .tp_init = (initproc)lutnode_init,
    .tp_dealloc = (destructor)lutnode_dealloc, .tp_getset = lutnode_getset, .tp_methods = node1_methods,
};

int init_lut3d(PyObject *module) {
    if (pyext_make_capsule(&lutnode_capsule, &lutnode_funcs) < 0) return -1;
    if (pyext_add_type(module, "Lut3D", &py_type_Lut3D) < 0) return -1;
    return pyext_add_type(module, "VideoLut3DFilter", &py_type_Lut3DFilter);
}
