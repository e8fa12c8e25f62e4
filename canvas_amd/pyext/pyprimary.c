/*
 * pyprimary.c -- the primary colour corrector of fluggo.media.process: per-channel curves, a 3 x 4 matrix, per-channel curves.
 *
 * No reference code: the reference's only colour node is the gain/offset filter.  Contract: DESIGN.md "Primary colour correction".
 *   ColorCurves(size, table, domain_min=(0, 0, 0), domain_max=(1, 1, 1))     an immutable value: the packed host tables (cvs_curves_pack)
 *   VideoColorCorrectFilter(source, pre=None, matrix=None, post=None)        cvs_primary_f32_dev / _f16_dev
 * f32 is the node's own format (a workspace pulls it as f32: nothing is rounded before the over); an f16 pull over a
 * half-native source goes through the _f16_dev entry in place in one launch (pylut3d.c's pattern).  With no stage set the node
 * hands its source's frame on and calls no entry.
 *
 * A ColorCurves keeps one device copy of its tables per device context (a VideoPullQueue(devices=...) pulls one node from several),
 * made on first use in a context: cvs_malloc, the upload on the pull's stream, and one wait for that stream before the pointer is
 * published, because the context's other threads run on streams of their own.  The value is immutable, so the copies live as long
 * as it does: a node holds a reference to its curves, reads the pointers under its reader lock and keeps that lock until the
 * launch is enqueued; a setter swaps the reference under the writer lock and drops the old one after it.  The copies are freed
 * with the value: cvs_free waits for the calling thread's device before it frees, so the thread binds itself to the copy's
 * context for that call (cvs_set_context) and then back to the context it was in.
 */
#include "pyext.h"
#include "canvas_primary.h"
#include <math.h>

enum { CURVE_CONTEXTS = 64 };           /* context ids are 0 .. 63 (canvas_hip.h) */

/* ---------------------------------------------------------------- ColorCurves */

typedef struct { PyObject_HEAD cvs_curves p; float *planar; size_t bytes; bool locked; pthread_mutex_t copies_lock; float *copies[CURVE_CONTEXTS]; } py_curves;
static PyTypeObject py_type_ColorCurves;

/* K rows of three numbers, or a flat sequence (or buffer of floats) of 3K -> rgb[3K], row by row */
static int curve_values(PyObject *table, float *rgb, int size) {
    const size_t want = (size_t)size * 3;
    Py_buffer view;
    if (PyObject_CheckBuffer(table) && PyObject_GetBuffer(table, &view, PyBUF_FORMAT | PyBUF_C_CONTIGUOUS) == 0) {
        const char *fmt = view.format ? view.format : "B";
        if (*fmt == '@' || *fmt == '=' || *fmt == '<') fmt++;
        const bool f32 = strcmp(fmt, "f") == 0, f64 = strcmp(fmt, "d") == 0;
        if (f32 || f64) {
            const size_t have = (size_t)view.len / (size_t)view.itemsize;
            if (have != want) {
                PyBuffer_Release(&view);
                PyErr_Format(PyExc_ValueError, "table holds %zu values, curves of that size take %zu", have, want);
                return -1;
            }
            for (size_t k = 0; k < want; k++) rgb[k] = f32 ? ((const float *)view.buf)[k] : (float)((const double *)view.buf)[k];
            PyBuffer_Release(&view);
            return 0;
        }
        PyBuffer_Release(&view);
    }
    PyErr_Clear();
    PyObject *seq = PySequence_Fast(table, "table must be a buffer of floats, a sequence of numbers or a sequence of (r, g, b) rows");
    if (!seq) return -1;
    const size_t have = (size_t)PySequence_Fast_GET_SIZE(seq);
    /* rows: `size` items that are sequences themselves (a row of a 2-D array is both a sequence and, to PyNumber_Check, a number) */
    PyObject *first = have > 0 ? PySequence_Fast_GET_ITEM(seq, 0) : NULL;
    const bool rows = have == (size_t)size && first && PySequence_Check(first) && !PyUnicode_Check(first) && !PyBytes_Check(first);
    if (!rows && have != want) {
        Py_DECREF(seq);
        PyErr_Format(PyExc_ValueError, "table holds %zu values, curves of that size take %zu (or %d rows of three)", have, want, size);
        return -1;
    }
    for (size_t k = 0; k < have; k++) {
        PyObject *item = PySequence_Fast_GET_ITEM(seq, (Py_ssize_t)k);
        if (!rows) {
            const double v = PyFloat_AsDouble(item);
            if (v == -1.0 && PyErr_Occurred()) { Py_DECREF(seq); return -1; }
            rgb[k] = (float)v;
            continue;
        }
        double r, g, b;
        PyObject *row = PySequence_Tuple(item);
        if (!row || !PyArg_ParseTuple(row, "ddd;a row of the table is three numbers", &r, &g, &b)) { Py_XDECREF(row); Py_DECREF(seq); return -1; }
        Py_DECREF(row);
        rgb[3 * k + 0] = (float)r; rgb[3 * k + 1] = (float)g; rgb[3 * k + 2] = (float)b;
    }
    Py_DECREF(seq);
    return 0;
}

static int curves_init(py_curves *self, PyObject *args, PyObject *kw) {
    static char *kwlist[] = { "size", "table", "domain_min", "domain_max", NULL };
    int size;
    PyObject *table;
    float lo[3] = { 0.0f, 0.0f, 0.0f }, hi[3] = { 1.0f, 1.0f, 1.0f };
    if (self->planar) { PyErr_SetString(PyExc_TypeError, "a ColorCurves is immutable"); return -1; }
    if (!PyArg_ParseTupleAndKeywords(args, kw, "iO|(fff)(fff)", kwlist, &size, &table, &lo[0], &lo[1], &lo[2], &hi[0], &hi[1], &hi[2])) return -1;
    const size_t bytes = cvs_curves_bytes(size);
    if (bytes == 0) { PyErr_SetString(PyExc_ValueError, cvs_last_error()); return -1; }
    for (int c = 0; c < 3; c++)
        if (!isfinite(lo[c]) || !isfinite(hi[c]) || !(lo[c] < hi[c])) {
            char msg[160];
            snprintf(msg, sizeof msg, "domain %g..%g of channel %d must be finite and ascending", lo[c], hi[c], c);
            PyErr_SetString(PyExc_ValueError, msg);
            return -1;
        }
    float *rgb = malloc(bytes), *planar = malloc(bytes);
    if (!rgb || !planar) { free(rgb); free(planar); PyErr_NoMemory(); return -1; }
    if (curve_values(table, rgb, size) != 0) { free(rgb); free(planar); return -1; }
    if (cvs_curves_pack(planar, rgb, size) != 0) { free(rgb); free(planar); PyErr_SetString(PyExc_ValueError, cvs_last_error()); return -1; }
    free(rgb);
    self->p.size = size;
    memcpy(self->p.domain_min, lo, sizeof lo);
    memcpy(self->p.domain_max, hi, sizeof hi);
    self->planar = planar;
    self->bytes = bytes;
    pthread_mutex_init(&self->copies_lock, NULL);
    self->locked = true;
    return 0;
}

/* the GIL may or may not be held; nobody else sees the value any more */
static void curves_free_copies(py_curves *self) {
    for (int ctx = 0; ctx < CURVE_CONTEXTS; ctx++) {
        if (!self->copies[ctx]) continue;
        const int here = cvs_current_context();
        if (here != ctx && cvs_set_context(ctx) == -2) continue;          /* (a context is never closed: not reached) */
        cvs_free(self->copies[ctx]);
        if (here != ctx) cvs_set_context(here);
        self->copies[ctx] = NULL;
    }
}
static void curves_dealloc(py_curves *self) {
    curves_free_copies(self);                          /* waits for each copy's device: what was queued on it has run */
    if (self->locked) pthread_mutex_destroy(&self->copies_lock);
    free(self->planar);
    Py_TYPE(self)->tp_free((PyObject *)self);
}

/* the tables' copy in the calling thread's context, made on first use.  NULL with the library's error set */
static const float *curves_copy_here(py_curves *self, cvs_stream_t stream) {
    int ctx = cvs_current_context();
    if (ctx < 0) { (void)cvs_compute_units(); ctx = cvs_current_context(); }     /* no context yet: opens the default one, or leaves the library's message why not */
    if (ctx < 0) return NULL;
    if (ctx >= CURVE_CONTEXTS) { cvs_set_context(ctx); return NULL; }            /* (ids are 0 .. 63: not reached; the call leaves "no context" as the message) */
    pthread_mutex_lock(&self->copies_lock);
    float *dev = self->copies[ctx];
    if (!dev) {
        dev = cvs_malloc(self->bytes);
        if (dev && (cvs_memcpy_h2d(dev, self->planar, self->bytes, stream) != 0 || cvs_stream_sync(stream) != 0)) { cvs_free(dev); dev = NULL; }
        self->copies[ctx] = dev;
    }
    pthread_mutex_unlock(&self->copies_lock);
    return dev;
}

static PyObject *curves_get_size(py_curves *self, void *closure) { return PyLong_FromLong(self->p.size); }
static PyObject *curves_get_domain(py_curves *self, void *closure) {
    const float *d = closure ? self->p.domain_max : self->p.domain_min;
    return Py_BuildValue("(ddd)", (double)d[0], (double)d[1], (double)d[2]);
}
/* the tables as they were given: K rows of three native floats */
static PyObject *curves_get_table(py_curves *self, void *closure) {
    const int size = self->p.size;
    PyObject *out = PyBytes_FromStringAndSize(NULL, (Py_ssize_t)self->bytes);
    if (!out) return NULL;
    float *rgb = (float *)PyBytes_AS_STRING(out);
    for (int k = 0; k < size; k++)
        for (int c = 0; c < 3; c++) rgb[3 * k + c] = self->planar[c * size + k];
    return out;
}
static PyGetSetDef curves_getset[] = {
    { "size", (getter)curves_get_size, NULL, "Nodes per channel (2..4097)." },
    { "domain_min", (getter)curves_get_domain, NULL, "The input value of node 0, per channel.", NULL },
    { "domain_max", (getter)curves_get_domain, NULL, "The input value of node size-1, per channel.", (void *)1 },
    { "table", (getter)curves_get_table, NULL, "The tables as bytes: size rows of three native floats (r g b)." },
    { NULL }
};
static PyTypeObject py_type_ColorCurves = {
    PyVarObject_HEAD_INIT(NULL, 0)
    .tp_name = "fluggo.media.process.ColorCurves", .tp_basicsize = sizeof(py_curves), .tp_flags = Py_TPFLAGS_DEFAULT,
    .tp_new = PyType_GenericNew, .tp_init = (initproc)curves_init, .tp_dealloc = (destructor)curves_dealloc, .tp_getset = curves_getset,
    .tp_doc = "ColorCurves(size, table, domain_min=(0, 0, 0), domain_max=(1, 1, 1)): three immutable 1D curves, one per colour channel; table: size rows of (r, g, b) or 3 * size numbers in that order (a 1D .cube's)",
};

/* ---------------------------------------------------------------- VideoColorCorrectFilter */

typedef struct { node1 n; py_curves *pre, *post; bool has_matrix; float matrix[12]; } py_cc;

/* None or a ColorCurves -> *out (a borrowed pointer or NULL); false with a TypeError set */
static bool curves_from(PyObject *v, const char *name, py_curves **out) {
    *out = NULL;
    if (!v || v == Py_None) return true;
    if (!PyObject_TypeCheck(v, &py_type_ColorCurves)) { PyErr_Format(PyExc_TypeError, "%s must be a ColorCurves or None", name); return false; }
    *out = (py_curves *)v;
    return true;
}
/* None, 12 numbers or 3 rows of 4 -> m[12] and *has; false with a Python error set, m and *has untouched */
static bool matrix_from(PyObject *v, float *m, bool *has) {
    if (!v || v == Py_None) { *has = false; return true; }
    PyObject *seq = PySequence_Fast(v, "matrix must be 12 numbers, 3 rows of 4 numbers, or None");
    if (!seq) return false;
    float got[12];
    const Py_ssize_t n = PySequence_Fast_GET_SIZE(seq);
    bool ok = n == 12 || n == 3;
    for (Py_ssize_t k = 0; ok && k < n; k++) {
        PyObject *item = PySequence_Fast_GET_ITEM(seq, k);
        if (n == 12) {
            const double d = PyFloat_AsDouble(item);
            if (d == -1.0 && PyErr_Occurred()) { Py_DECREF(seq); return false; }
            got[k] = (float)d;
        } else {
            double a, b, c, d;
            PyObject *row = PyNumber_Check(item) ? NULL : PySequence_Tuple(item);
            if (!row) { PyErr_Clear(); ok = false; break; }
            if (!PyArg_ParseTuple(row, "dddd;a row of the matrix is four numbers", &a, &b, &c, &d)) { Py_DECREF(row); Py_DECREF(seq); return false; }
            Py_DECREF(row);
            got[4 * k + 0] = (float)a; got[4 * k + 1] = (float)b; got[4 * k + 2] = (float)c; got[4 * k + 3] = (float)d;
        }
    }
    Py_DECREF(seq);
    if (!ok) { PyErr_SetString(PyExc_ValueError, "matrix takes 12 numbers or 3 rows of 4 numbers"); return false; }
    for (int k = 0; k < 12; k++)
        if (!isfinite(got[k])) { PyErr_Format(PyExc_ValueError, "matrix entry %d (row %d) is not finite", k, k / 4); return false; }
    memcpy(m, got, sizeof got);
    *has = true;
    return true;
}

static int cc_init(py_cc *self, PyObject *args, PyObject *kw) {
    static char *kwlist[] = { "source", "pre", "matrix", "post", NULL };
    PyObject *src, *pre = NULL, *matrix = NULL, *post = NULL;
    pthread_rwlock_init(&self->n.lock, NULL);
    if (!PyArg_ParseTupleAndKeywords(args, kw, "O|OOO", kwlist, &src, &pre, &matrix, &post)) return -1;
    py_curves *a, *b;
    if (!curves_from(pre, "pre", &a) || !curves_from(post, "post", &b) || !matrix_from(matrix, self->matrix, &self->has_matrix)) return -1;
    if (!py_video_take_source(src, &self->n.source)) return -1;
    Py_XINCREF(a); Py_XINCREF(b);
    self->pre = a; self->post = b;
    return 0;
}
static void cc_dealloc(py_cc *self) {
    py_video_take_source(NULL, &self->n.source);
    Py_XDECREF(self->pre);
    Py_XDECREF(self->post);
    pthread_rwlock_destroy(&self->n.lock);
    Py_TYPE(self)->tp_free((PyObject *)self);
}

/* `f` in either format: the source pulled in that format into `f` itself, then the library entry of that format in place */
static void cc_render(PyObject *o, int frame_index, rgba_frame_dev *f) {
    py_cc *self = (py_cc *)o;
    py_rdlock(&self->n.lock);
    video_get_frame_dev(self->n.source, frame_index, f);
    if ((!self->pre && !self->post && !self->has_matrix) || box2i_is_empty(&f->current_window)) {
        pthread_rwlock_unlock(&self->n.lock);                             /* no stage: the source's frame as it came */
        return;
    }
    cvs_primary p;
    memset(&p, 0, sizeof p);
    const float *pre = NULL, *post = NULL;
    bool ok = true;
    if (self->pre) { p.pre = self->pre->p; pre = curves_copy_here(self->pre, f->stream); ok = ok && pre; }
    if (self->post) { p.post = self->post->p; post = curves_copy_here(self->post, f->stream); ok = ok && post; }
    if (self->has_matrix) { memcpy(p.matrix, self->matrix, sizeof p.matrix); p.flags = CVS_PRIMARY_MATRIX; }
    if (!ok) {
        box2i_set_empty(&f->current_window);
    } else if (f->format == CVS_FORMAT_F16) {
        rgba_frame_f16 fo = { f->data, f->full_window, f->current_window };
        cvs_primary_f16_dev(&fo, &fo, &p, pre, post, f->stream);
        f->current_window = fo.current_window;
    } else {
        rgba_frame_f32 fo = { f->data, f->full_window, f->current_window };
        cvs_primary_f32_dev(&fo, &fo, &p, pre, post, f->stream);
        f->current_window = fo.current_window;
    }
    pthread_rwlock_unlock(&self->n.lock);               /* only now: the launch that reads the copies is queued */
}

DEFINE_NODE_VTABLE_HALF_DIRECT(cc)                    /* widen, grade, truncate: one launch */

static PyObject *cc_get_curves(py_cc *self, void *closure) {
    PyObject *v = (PyObject *)(closure ? self->post : self->pre);
    if (!v) Py_RETURN_NONE;
    Py_INCREF(v);
    return v;
}
static int cc_set_curves(py_cc *self, PyObject *v, void *closure) {
    py_curves *next;
    if (!curves_from(v, closure ? "post" : "pre", &next)) return -1;
    Py_XINCREF(next);
    py_wrlock_nogil(&self->n.lock);
    py_curves **slot = closure ? &self->post : &self->pre, *old = *slot;
    *slot = next;
    pthread_rwlock_unlock(&self->n.lock);
    Py_XDECREF(old);                                    /* (its copies, if this was the last reference: freed after the device has run what was queued) */
    return 0;
}
static PyObject *cc_get_matrix(py_cc *self, void *closure) {
    if (!self->has_matrix) Py_RETURN_NONE;
    PyObject *out = PyTuple_New(12);
    if (!out) return NULL;
    for (int k = 0; k < 12; k++) PyTuple_SET_ITEM(out, k, PyFloat_FromDouble((double)self->matrix[k]));
    return out;
}
static int cc_set_matrix(py_cc *self, PyObject *v, void *closure) {
    float m[12] = { 0 };
    bool has;
    if (!matrix_from(v, m, &has)) return -1;
    py_wrlock_nogil(&self->n.lock);
    memcpy(self->matrix, m, sizeof m);
    self->has_matrix = has;
    pthread_rwlock_unlock(&self->n.lock);
    return 0;
}

static PyGetSetDef cc_getset[] = {
    { VIDEO_FRAME_SOURCE_FUNCS, pyext_capsule_getter, NULL, "Video frame source C API.", &cc_capsule },
    { "source", (getter)node1_get_source, (setter)node1_set_source_attr, "The upstream video source." },
    { "pre", (getter)cc_get_curves, (setter)cc_set_curves, "The ColorCurves applied first, or None.", NULL },
    { "matrix", (getter)cc_get_matrix, (setter)cc_set_matrix, "The 3 x 4 matrix applied between the curves, 12 numbers row by row, or None." },
    { "post", (getter)cc_get_curves, (setter)cc_set_curves, "The ColorCurves applied last, or None.", (void *)1 },
    { NULL }
};
static PyTypeObject py_type_ColorCorrect = {
    PyVarObject_HEAD_INIT(NULL, 0)
    .tp_name = "fluggo.media.process.VideoColorCorrectFilter", .tp_basicsize = sizeof(py_cc), .tp_flags = Py_TPFLAGS_DEFAULT,
    .tp_base = &py_type_VideoSource, .tp_new = PyType_GenericNew, .tp_init = (initproc)cc_init,
    .tp_dealloc = (destructor)cc_dealloc, .tp_getset = cc_getset, .tp_methods = node1_methods,
};

int init_primary(PyObject *module) {
    if (pyext_make_capsule(&cc_capsule, &cc_funcs) < 0) return -1;
    if (pyext_add_type(module, "ColorCurves", &py_type_ColorCurves) < 0) return -1;
    return pyext_add_type(module, "VideoColorCorrectFilter", &py_type_ColorCorrect);
}
