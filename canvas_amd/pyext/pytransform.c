/*
 * pytransform.c -- the geometry node of fluggo.media.process beside VideoScaler: rotate, scale, mirror and move a layer about an
 * anchor point, interpolated alpha-weighted so that the layer's edge keeps its colour.
 *
 * No reference code.  Contract: DESIGN.md "Affine transform".
 *   VideoTransformFilter(source, source_rect, anchor=(0, 0), scale=(1, 1), rotation=0.0, position=(0, 0), filter="bilinear")
 *                                                                    cvs_transform_f32_dev / _f16_dev
 * A source point p lands on  position + R(rotation) * diag(scale) * (p - anchor), rotation in degrees, clockwise on screen.  The
 * parts are numbers, pairs or frame functions, read as f32 like every v2f of the path; cvs_transform_from_parts turns them into the
 * six target -> source coefficients, which inverse_at(frame_index) shows.  source_rect bounds what is pulled, as VideoScaler's
 * does: the source is pulled over cvs_transform_source_window(the frame asked for) clipped to it into a pooled frame, then the
 * entry of the pulled format writes the frame; the window reported is where source_rect lands in the frame asked for (fill_layer).
 * Coordinates are absolute, so a frame pulled in tiles equals the frame pulled whole, window included.  f32 is the node's own format; an f16 pull over a half-native source goes through the _f16_dev entry in one launch
 * (pymatte.c).  Locking as in pymatte.c: reader lock around the upstream pull and the parameters, writer lock where either is
 * replaced.  A pull never raises: no source, no device, a degenerate scale or a refusing entry end in an empty window.
 */
#include "pyext.h"
#include <math.h>

enum { PART_RECT, PART_ANCHOR, PART_SCALE, PART_ROTATION, PART_POSITION, PART_COUNT };
static const char *part_names[PART_COUNT] = { "source_rect", "anchor", "scale", "rotation", "position" };

/* given[k]: the constant as it was handed over (what the attribute reads back), NULL where the holder has a frame function */
typedef struct { node1 n; FrameFunctionHolder part[PART_COUNT]; PyObject *given[PART_COUNT]; int filter; } py_transform;

/* a constant of the shape the part takes, or a frame function, into a holder of its own: false with a Python error set */
static bool part_parse(int k, PyObject *v, FrameFunctionHolder *fresh) {
    framefunc_init(fresh, 0, 0, 0, 0);
    if (!v || v == Py_None) { PyErr_Format(PyExc_TypeError, "%s takes a value or a frame function", part_names[k]); return false; }
    bool shaped;
    if (k == PART_RECT) shaped = PyTuple_Check(v) && PyTuple_GET_SIZE(v) == 2 && PyTuple_Check(PyTuple_GET_ITEM(v, 0)) && PyTuple_Check(PyTuple_GET_ITEM(v, 1));
    else if (k == PART_ROTATION) shaped = PyFloat_Check(v) || (PyLong_Check(v) && !PyBool_Check(v));
    else shaped = PyTuple_Check(v) && PyTuple_GET_SIZE(v) == 2 && !PyTuple_Check(PyTuple_GET_ITEM(v, 0));
    if (!shaped && (PyTuple_Check(v) || PyNumber_Check(v) || PyUnicode_Check(v) || PyBytes_Check(v))) {
        PyErr_Format(PyExc_TypeError, "%s takes %s or a frame function", part_names[k], k == PART_RECT ? "a box2i" : k == PART_ROTATION ? "a number" : "a pair of numbers");
        return false;
    }
    if (!py_framefunc_take_source(v, fresh)) return false;
    if (!fresh->source) {
        const int count = k == PART_RECT ? 4 : k == PART_ROTATION ? 1 : 2;
        for (int i = 0; i < count; i++)
            if (!isfinite(fresh->constant[i])) { PyErr_Format(PyExc_ValueError, "%s must be finite", part_names[k]); return false; }
    }
    return true;
}

/* the node takes the parsed part over (under the writer lock once the node is alive) */
static void part_install(py_transform *self, int k, PyObject *v, FrameFunctionHolder *fresh, bool locked) {
    PyObject *keep = fresh->source ? NULL : v;
    Py_XINCREF(keep);
    if (locked) py_wrlock_nogil(&self->n.lock);
    FrameFunctionHolder old = self->part[k];
    PyObject *old_given = self->given[k];
    self->part[k] = *fresh;
    self->given[k] = keep;
    if (locked) pthread_rwlock_unlock(&self->n.lock);
    py_framefunc_take_source(NULL, &old);
    Py_XDECREF(old_given);
}

int py_transform_filter_from(PyObject *v) {
    if (v && PyUnicode_Check(v)) {
        if (PyUnicode_CompareWithASCIIString(v, "nearest") == 0) return CVS_TRANSFORM_NEAREST;
        if (PyUnicode_CompareWithASCIIString(v, "bilinear") == 0) return CVS_TRANSFORM_BILINEAR;
        PyErr_SetString(PyExc_ValueError, "filter is \"nearest\" or \"bilinear\"");
        return -1;
    }
    PyErr_SetString(PyExc_TypeError, "filter is the string \"nearest\" or \"bilinear\"");
    return -1;
}

static int transform_init(py_transform *self, PyObject *args, PyObject *kw) {
    static char *kwlist[] = { "source", "source_rect", "anchor", "scale", "rotation", "position", "filter", NULL };
    PyObject *src, *given[PART_COUNT] = { NULL }, *filter = NULL;
    pthread_rwlock_init(&self->n.lock, NULL);
    self->filter = CVS_TRANSFORM_BILINEAR;
    for (int k = 0; k < PART_COUNT; k++) framefunc_init(&self->part[k], 0, 0, 0, 0);
    if (!PyArg_ParseTupleAndKeywords(args, kw, "OO|OOOOO", kwlist, &src, &given[PART_RECT], &given[PART_ANCHOR], &given[PART_SCALE],
                                     &given[PART_ROTATION], &given[PART_POSITION], &filter)) return -1;
    if (filter && (self->filter = py_transform_filter_from(filter)) < 0) return -1;
    PyObject *defaults[PART_COUNT] = { NULL, Py_BuildValue("(dd)", 0.0, 0.0), Py_BuildValue("(dd)", 1.0, 1.0), PyFloat_FromDouble(0.0), Py_BuildValue("(dd)", 0.0, 0.0) };
    bool ok = true;
    for (int k = 0; k < PART_COUNT; k++) {
        PyObject *v = given[k] ? given[k] : defaults[k];
        FrameFunctionHolder fresh;
        if (ok && v && part_parse(k, v, &fresh)) part_install(self, k, v, &fresh, false);
        else ok = false;
    }
    for (int k = 0; k < PART_COUNT; k++) Py_XDECREF(defaults[k]);
    if (!ok) { if (!PyErr_Occurred()) PyErr_NoMemory(); return -1; }
    return py_video_take_source(src, &self->n.source) ? 0 : -1;
}
static void transform_dealloc(py_transform *self) {
    py_video_take_source(NULL, &self->n.source);
    for (int k = 0; k < PART_COUNT; k++) { py_framefunc_take_source(NULL, &self->part[k]); Py_CLEAR(self->given[k]); }
    pthread_rwlock_destroy(&self->n.lock);
    Py_TYPE(self)->tp_free((PyObject *)self);
}

/* the coefficients of one frame, under the caller's reader lock: cvs_transform_from_parts' return value */
static int coefficients(py_transform *self, int frame_index, float m[6]) {
    v2f anchor, scale, position;
    framefunc_get_v2f(&anchor, &self->part[PART_ANCHOR], frame_index);
    framefunc_get_v2f(&scale, &self->part[PART_SCALE], frame_index);
    framefunc_get_v2f(&position, &self->part[PART_POSITION], frame_index);
    const double a[2] = { anchor.x, anchor.y }, s[2] = { scale.x, scale.y }, p[2] = { position.x, position.y };
    return cvs_transform_from_parts(a, s, framefunc_get_f32(&self->part[PART_ROTATION], frame_index), p, m);
}

/* transparent black over `box` of `f` (its window is left alone): 0, or -1 */
int py_clear_box(rgba_frame_dev *f, int x0, int y0, int x1, int y1) {
    static const rgba_f32 nothing = { 0.0f, 0.0f, 0.0f, 0.0f };
    box2i box;
    box2i_set(&box, x0, y0, x1, y1);
    if (box2i_is_empty(&box)) return 0;
    if (f->format == CVS_FORMAT_F16) {
        rgba_frame_f16 t = { f->data, f->full_window, f->full_window };
        return cvs_fill_solid_f16_dev(&t, &box, &nothing, f->stream);
    }
    rgba_frame_f32 t = { f->data, f->full_window, f->full_window };
    return cvs_fill_solid_f32_dev(&t, &box, &nothing, f->stream);
}

/* The window the node reports does not depend on how much of the source this pull happened to ask for: it is where source_rect
 * lands in the frame asked for, `layer`, of which the entry has written `win` (the part the pulled source reaches); the rest is
 * transparent black.  With the entry's own window a node above would see a window that varies with the tile it is pulled in, and
 * a blur's or a matte's result would vary with it (DESIGN.md "Affine transform", Node).  0, or -1 */
static int fill_layer(rgba_frame_dev *f, const box2i *layer) {
    box2i win = f->current_window, all = *layer;
    if (box2i_is_empty(&all)) return 0;
    if (box2i_is_empty(&win)) { f->current_window = all; return py_clear_box(f, all.min.x, all.min.y, all.max.x, all.max.y); }
    if (win.min.x < all.min.x) all.min.x = win.min.x;
    if (win.min.y < all.min.y) all.min.y = win.min.y;
    if (win.max.x > all.max.x) all.max.x = win.max.x;
    if (win.max.y > all.max.y) all.max.y = win.max.y;
    f->current_window = all;
    if (py_clear_box(f, all.min.x, all.min.y, all.max.x, win.min.y - 1) != 0 || py_clear_box(f, all.min.x, win.max.y + 1, all.max.x, all.max.y) != 0) return -1;
    if (py_clear_box(f, all.min.x, win.min.y, win.min.x - 1, win.max.y) != 0 || py_clear_box(f, win.max.x + 1, win.min.y, all.max.x, win.max.y) != 0) return -1;
    return 0;
}

/* `f` in either format: the source pulled in that format over the window the taps need, then the library entry of that format */
static void transform_render(PyObject *o, int frame_index, rgba_frame_dev *f) {
    py_transform *self = (py_transform *)o;
    py_rdlock(&self->n.lock);
    cvs_transform t = { { 0 }, self->filter, 0 };
    box2i need, rect, layer = { { 0, 0 }, { -1, -1 } };
    rgba_frame_dev in = { NULL, f->format, { { 0, 0 }, { -1, -1 } }, { { 0, 0 }, { -1, -1 } }, f->stream };
    const bool sound = coefficients(self, frame_index, t.m) == 0 && cvs_transform_source_window(&t, &f->full_window, &need) == 0;
    bool draw = sound, beyond = false;            /* beyond: the frame asked for reaches nothing of source_rect */
    if (draw && self->n.source) {
        framefunc_get_box2i(&rect, &self->part[PART_RECT], frame_index);
        if (cvs_transform_target_window(&t, &rect, &f->full_window, &layer) != 0) box2i_set_empty(&layer);
        box2i_intersect(&need, &need, &rect);
        beyond = box2i_is_empty(&need);
        draw = !beyond;
    }
    if (draw && self->n.source) {
        const int lim = CVS_TRANSFORM_MAX_COORD;
        in.full_window = in.current_window = need;
        /* a window the entry will refuse is not pulled: the entry is still called, for its message */
        if (need.min.x >= -lim && need.min.y >= -lim && need.max.x <= lim && need.max.y <= lim) {
            in.data = cvs_pool_malloc(frame_bytes(&need, f->format), f->stream);
            if (!in.data) draw = false;
            else video_get_frame_dev(self->n.source, frame_index, &in);
        }
    }
    int rc = -1;
    if (draw) {
        /* without a source the entry gets none, and says so */
        if (f->format == CVS_FORMAT_F16) {
            rgba_frame_f16 fi = { in.data, in.full_window, in.current_window }, fo = { f->data, f->full_window, f->full_window };
            rc = cvs_transform_f16_dev(&fo, self->n.source ? &fi : NULL, &t, f->stream);
            f->current_window = fo.current_window;
        } else {
            rgba_frame_f32 fi = { in.data, in.full_window, in.current_window }, fo = { f->data, f->full_window, f->full_window };
            rc = cvs_transform_f32_dev(&fo, self->n.source ? &fi : NULL, &t, f->stream);
            f->current_window = fo.current_window;
        }
    } else if (beyond) {
        /* the entry has nothing to write; the layer's box is still reported */
        rc = 0;
        box2i_set_empty(&f->current_window);
    }
    if (rc == 0 && self->n.source) rc = fill_layer(f, &layer);
    pthread_rwlock_unlock(&self->n.lock);
    if (rc != 0) box2i_set_empty(&f->current_window);
    if (in.data) cvs_pool_free(in.data, f->stream);
}

static void transform_slot_dev(PyObject *o, int i, rgba_frame_dev *f) {
    py_transform *self = (py_transform *)o;
    py_rdlock(&self->n.lock);
    const bool direct = f->format == CVS_FORMAT_F16 && half_native(self->n.source);
    pthread_rwlock_unlock(&self->n.lock);
    if (direct) transform_render(o, i, f);                  /* widen, warp, truncate: one launch */
    else node_get_frame_dev(o, i, f, CVS_FORMAT_F32, transform_render);
}
static void transform_slot_32(PyObject *o, int i, rgba_frame_f32 *f) { node_get_frame_host32(o, i, f, CVS_FORMAT_F32, transform_render); }
static video_frame_source_funcs transform_funcs = {
    .flags = VIDEO_SOURCE_FLAG_DEVICE, .get_frame_32 = (video_get_frame_32_func)transform_slot_32,
    .get_frame_dev = (video_get_frame_dev_func)transform_slot_dev };
static PyObject *transform_capsule;

/* closure: the part's index */
static PyObject *transform_get_part(py_transform *self, void *closure) {
    const int k = (int)(size_t)closure;
    PyObject *v = self->part[k].source ? self->part[k].source : self->given[k];
    Py_INCREF(v);
    return v;
}
static int transform_set_part(py_transform *self, PyObject *v, void *closure) {
    const int k = (int)(size_t)closure;
    FrameFunctionHolder fresh;
    if (!part_parse(k, v, &fresh)) return -1;                /* a value that is refused leaves the old one */
    part_install(self, k, v, &fresh, true);
    return 0;
}
static PyObject *transform_get_filter(py_transform *self, void *closure) {
    return PyUnicode_FromString(self->filter == CVS_TRANSFORM_NEAREST ? "nearest" : "bilinear");
}
static int transform_set_filter(py_transform *self, PyObject *v, void *closure) {
    const int filter = py_transform_filter_from(v);
    if (filter < 0) return -1;
    py_wrlock_nogil(&self->n.lock);
    self->filter = filter;
    pthread_rwlock_unlock(&self->n.lock);
    return 0;
}

static PyObject *transform_inverse_at(py_transform *self, PyObject *args) {
    int frame_index;
    if (!PyArg_ParseTuple(args, "i", &frame_index)) return NULL;
    float m[6];
    py_rdlock(&self->n.lock);
    const int rc = coefficients(self, frame_index, m);
    pthread_rwlock_unlock(&self->n.lock);
    if (rc < 0) { PyErr_SetString(PyExc_ValueError, cvs_last_error()); return NULL; }
    if (rc > 0) Py_RETURN_NONE;
    return Py_BuildValue("(dddddd)", (double)m[0], (double)m[1], (double)m[2], (double)m[3], (double)m[4], (double)m[5]);
}

static PyMethodDef transform_methods[] = {
    { "set_source", (PyCFunction)node1_set_source, METH_VARARGS, "Sets the video source." },
    { "inverse_at", (PyCFunction)transform_inverse_at, METH_VARARGS,
      "inverse_at(frame_index): the six f32 coefficients (m0..m5, target to source) the frame is drawn with, or None where a scale is 0." },
    { NULL }
};
#define PART(k) ((void *)(size_t)(k))
static PyGetSetDef transform_getset[] = {
    { VIDEO_FRAME_SOURCE_FUNCS, pyext_capsule_getter, NULL, "Video frame source C API.", &transform_capsule },
    { "source", (getter)node1_get_source, (setter)node1_set_source_attr, "The upstream video source." },
    { "source_rect", (getter)transform_get_part, (setter)transform_set_part, "The part of the source that is drawn (box2i or frame function).", PART(PART_RECT) },
    { "anchor", (getter)transform_get_part, (setter)transform_set_part, "The source point that scale and rotation leave in place (pair or frame function).", PART(PART_ANCHOR) },
    { "scale", (getter)transform_get_part, (setter)transform_set_part, "Scale factors along x and y, negative to mirror (pair or frame function).", PART(PART_SCALE) },
    { "rotation", (getter)transform_get_part, (setter)transform_set_part, "Degrees, clockwise on screen (number or frame function).", PART(PART_ROTATION) },
    { "position", (getter)transform_get_part, (setter)transform_set_part, "Where the anchor lands in the target (pair or frame function).", PART(PART_POSITION) },
    { "filter", (getter)transform_get_filter, (setter)transform_set_filter, "\"nearest\" or \"bilinear\" (alpha-weighted)." },
    { NULL }
};
static PyTypeObject py_type_Transform = {
    PyVarObject_HEAD_INIT(NULL, 0)
    .tp_name = "fluggo.media.process.VideoTransformFilter", .tp_basicsize = sizeof(py_transform), .tp_flags = Py_TPFLAGS_DEFAULT,
    .tp_base = &py_type_VideoSource, .tp_new = PyType_GenericNew, .tp_init = (initproc)transform_init,
    .tp_dealloc = (destructor)transform_dealloc, .tp_getset = transform_getset, .tp_methods = transform_methods,
};

int init_transform(PyObject *module) {
    if (pyext_make_capsule(&transform_capsule, &transform_funcs) < 0) return -1;
    return pyext_add_type(module, "VideoTransformFilter", &py_type_Transform);
}
