/*
 * pyperspective.c -- the corner pin of fluggo.media.process: a layer put onto a surface that is not parallel to the screen, its
 * four corners pinned to four points, interpolated alpha-weighted so that the layer's edge keeps its colour.
 *
 * No reference code.  Contract: DESIGN.md "Corner pin".
 *   VideoCornerPinFilter(source, source_rect, corners, filter="bilinear")          cvs_perspective_f32_dev / _f16_dev
 * corners: where the top-left, top-right, bottom-right and bottom-left corners of source_rect's outer edges (min - 1/2 ..
 * max + 1/2) land, each a pair or a frame function, read as f32 like every v2f of the path; cvs_perspective_from_quad turns them
 * into the nine target -> source coefficients and the two origins, which coefficients_at(frame_index) shows.  source_rect bounds
 * what is pulled, as VideoTransformFilter's does: the source is pulled over cvs_perspective_source_window(the frame asked for)
 * clipped to it into a pooled frame, then the entry of the pulled format writes the frame.  The window reported is the quad's
 * bounding box [floor(min) - 1, ceil(max) + 1] cropped to the frame asked for, whatever part of the source this pull reached
 * (fill_layer), so a frame pulled in tiles equals the frame pulled whole, window included.  f32 is the node's own format; an f16
 * pull over a half-native source goes through the _f16_dev entry in one launch.  Locking as in pytransform.c: reader lock around
 * the upstream pull and the parameters, writer lock where either is replaced.  A pull never raises: no source, no device, a quad
 * that is not convex or a refusing entry end in an empty window.
 */
#include "pyext.h"
#include "canvas_perspective.h"
#include <math.h>

enum { PART_RECT, PART_CORNER0, PART_COUNT = PART_CORNER0 + 4 };
static const char *part_names[PART_COUNT] = { "source_rect", "corners[0]", "corners[1]", "corners[2]", "corners[3]" };

/* given[k]: the constant as it was handed over (what the attribute reads back), NULL where the holder has a frame function */
typedef struct { node1 n; FrameFunctionHolder part[PART_COUNT]; PyObject *given[PART_COUNT]; int filter; } py_pin;

/* a constant of the shape the part takes, or a frame function, into a holder of its own: false with a Python error set */
static bool part_parse(int k, PyObject *v, FrameFunctionHolder *fresh) {
    framefunc_init(fresh, 0, 0, 0, 0);
    if (!v || v == Py_None) { PyErr_Format(PyExc_TypeError, "%s takes a value or a frame function", part_names[k]); return false; }
    bool shaped;
    if (k == PART_RECT) shaped = PyTuple_Check(v) && PyTuple_GET_SIZE(v) == 2 && PyTuple_Check(PyTuple_GET_ITEM(v, 0)) && PyTuple_Check(PyTuple_GET_ITEM(v, 1));
    else shaped = PyTuple_Check(v) && PyTuple_GET_SIZE(v) == 2 && !PyTuple_Check(PyTuple_GET_ITEM(v, 0));
    if (!shaped && (PyTuple_Check(v) || PyNumber_Check(v) || PyUnicode_Check(v) || PyBytes_Check(v))) {
        PyErr_Format(PyExc_TypeError, "%s takes %s or a frame function", part_names[k], k == PART_RECT ? "a box2i" : "a pair of numbers");
        return false;
    }
    if (!py_framefunc_take_source(v, fresh)) return false;
    if (!fresh->source) {
        const int count = k == PART_RECT ? 4 : 2;
        for (int i = 0; i < count; i++)
            if (!isfinite(fresh->constant[i])) { PyErr_Format(PyExc_ValueError, "%s must be finite", part_names[k]); return false; }
    }
    return true;
}

/* the node takes the parsed part over (the caller holds the writer lock once the node is alive); what it held before comes
 * back through `old` and `old_given`, to be released outside the lock */
static void part_swap(py_pin *self, int k, PyObject *v, FrameFunctionHolder *fresh, FrameFunctionHolder *old, PyObject **old_given) {
    PyObject *keep = fresh->source ? NULL : v;
    Py_XINCREF(keep);
    *old = self->part[k];
    *old_given = self->given[k];
    self->part[k] = *fresh;
    self->given[k] = keep;
}

/* parts first .. first + count - 1 from values[]: all of them or, with a Python error set, none */
static int parts_set(py_pin *self, int first, int count, PyObject **values, bool locked) {
    FrameFunctionHolder fresh[PART_COUNT], old[PART_COUNT];
    PyObject *old_given[PART_COUNT];
    for (int i = 0; i < count; i++)
        if (!part_parse(first + i, values[i], &fresh[i])) {
            for (int j = 0; j < i; j++) py_framefunc_take_source(NULL, &fresh[j]);
            return -1;
        }
    if (locked) py_wrlock_nogil(&self->n.lock);
    for (int i = 0; i < count; i++) part_swap(self, first + i, values[i], &fresh[i], &old[i], &old_given[i]);
    if (locked) pthread_rwlock_unlock(&self->n.lock);
    for (int i = 0; i < count; i++) { py_framefunc_take_source(NULL, &old[i]); Py_XDECREF(old_given[i]); }
    return 0;
}

static int corners_from(PyObject *v, PyObject *items[4]) {
    if (!v || !(PyTuple_Check(v) || PyList_Check(v)) || PySequence_Size(v) != 4) {
        PyErr_SetString(PyExc_TypeError, "corners takes four points: top-left, top-right, bottom-right, bottom-left, each a pair of numbers or a frame function");
        return -1;
    }
    for (int i = 0; i < 4; i++) items[i] = PyTuple_Check(v) ? PyTuple_GET_ITEM(v, i) : PyList_GET_ITEM(v, i);     /* borrowed */
    return 0;
}

static int pin_init(py_pin *self, PyObject *args, PyObject *kw) {
    static char *kwlist[] = { "source", "source_rect", "corners", "filter", NULL };
    PyObject *src, *rect, *corners, *filter = NULL, *items[4];
    pthread_rwlock_init(&self->n.lock, NULL);
    self->filter = CVS_TRANSFORM_BILINEAR;
    for (int k = 0; k < PART_COUNT; k++) framefunc_init(&self->part[k], 0, 0, 0, 0);
    if (!PyArg_ParseTupleAndKeywords(args, kw, "OOO|O", kwlist, &src, &rect, &corners, &filter)) return -1;
    if (filter && (self->filter = py_transform_filter_from(filter)) < 0) return -1;
    if (parts_set(self, PART_RECT, 1, &rect, false) < 0) return -1;
    if (corners_from(corners, items) < 0 || parts_set(self, PART_CORNER0, 4, items, false) < 0) return -1;
    return py_video_take_source(src, &self->n.source) ? 0 : -1;
}
static void pin_dealloc(py_pin *self) {
    py_video_take_source(NULL, &self->n.source);
    for (int k = 0; k < PART_COUNT; k++) { py_framefunc_take_source(NULL, &self->part[k]); Py_CLEAR(self->given[k]); }
    pthread_rwlock_destroy(&self->n.lock);
    Py_TYPE(self)->tp_free((PyObject *)self);
}

/* the map of one frame, under the caller's reader lock: cvs_perspective_from_quad's return value, with source_rect and the
 * quad's bounding box [floor(min) - 1, ceil(max) + 1] (each bound kept inside +-2^30) */
static int coefficients(py_pin *self, int frame_index, cvs_perspective *p, box2i *rect, box2i *bbox) {
    double quad[4][2], lo[2], hi[2];
    framefunc_get_box2i(rect, &self->part[PART_RECT], frame_index);
    for (int k = 0; k < 4; k++) {
        v2f c;
        framefunc_get_v2f(&c, &self->part[PART_CORNER0 + k], frame_index);
        quad[k][0] = c.x; quad[k][1] = c.y;
    }
    const double edges[4] = { rect->min.x - 0.5, rect->min.y - 0.5, rect->max.x + 0.5, rect->max.y + 0.5 };
    const int rc = cvs_perspective_from_quad(edges, (const double (*)[2])quad, self->filter, p);
    if (rc != 0) return rc;
    for (int a = 0; a < 2; a++) {
        lo[a] = hi[a] = quad[0][a];
        for (int k = 1; k < 4; k++) { if (quad[k][a] < lo[a]) lo[a] = quad[k][a]; if (quad[k][a] > hi[a]) hi[a] = quad[k][a]; }
        lo[a] = fmax(floor(lo[a]) - 1.0, -1073741824.0);
        hi[a] = fmin(ceil(hi[a]) + 1.0, 1073741824.0);
    }
    box2i_set(bbox, (int)lo[0], (int)lo[1], (int)hi[0], (int)hi[1]);
    return 0;
}

/* The window the node reports does not depend on how much of the source this pull happened to ask for: it is `layer`, the quad's
 * bounding box in the frame asked for, of which the entry has written f->current_window (the part the pulled source reaches);
 * the rest of it is made transparent black, in at most four strips (DESIGN.md "Affine transform", Node, has the reason).  0, or -1 */
static int fill_layer(rgba_frame_dev *f, const box2i *layer) {
    box2i win;
    const box2i all = *layer;
    box2i_intersect(&win, &f->current_window, layer);
    f->current_window = all;
    if (box2i_is_empty(&all)) { box2i_set_empty(&f->current_window); return 0; }
    if (box2i_is_empty(&win)) return py_clear_box(f, all.min.x, all.min.y, all.max.x, all.max.y);
    if (py_clear_box(f, all.min.x, all.min.y, all.max.x, win.min.y - 1) != 0 || py_clear_box(f, all.min.x, win.max.y + 1, all.max.x, all.max.y) != 0) return -1;
    if (py_clear_box(f, all.min.x, win.min.y, win.min.x - 1, win.max.y) != 0 || py_clear_box(f, win.max.x + 1, win.min.y, all.max.x, win.max.y) != 0) return -1;
    return 0;
}

static bool within_span(const box2i *b, const int origin[2]) {
    const long long lim = CVS_PERSPECTIVE_MAX_SPAN;
    return (long long)b->min.x - origin[0] >= -lim && (long long)b->min.y - origin[1] >= -lim && (long long)b->max.x - origin[0] <= lim && (long long)b->max.y - origin[1] <= lim;
}

/* `f` in either format: the source pulled in that format over the window the taps need, then the library entry of that format */
static void pin_render(PyObject *o, int frame_index, rgba_frame_dev *f) {
    py_pin *self = (py_pin *)o;
    py_rdlock(&self->n.lock);
    cvs_perspective p;
    box2i need, rect, bbox, layer = { { 0, 0 }, { -1, -1 } };
    rgba_frame_dev in = { NULL, f->format, { { 0, 0 }, { -1, -1 } }, { { 0, 0 }, { -1, -1 } }, f->stream };
    const bool sound = coefficients(self, frame_index, &p, &rect, &bbox) == 0 && cvs_perspective_source_window(&p, &f->full_window, &need) == 0;
    bool draw = sound, beyond = false;            /* beyond: the frame asked for reaches nothing of source_rect */
    if (draw) box2i_intersect(&layer, &bbox, &f->full_window);
    if (draw && self->n.source) {
        box2i_intersect(&need, &need, &rect);
        beyond = box2i_is_empty(&need);
        draw = !beyond;
    }
    if (draw && self->n.source) {
        in.full_window = in.current_window = need;
        /* a window the entry will refuse is not pulled: the entry is still called, for its message */
        if (within_span(&need, p.source_origin) && within_span(&f->full_window, p.target_origin)) {
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
            rc = cvs_perspective_f16_dev(&fo, self->n.source ? &fi : NULL, &p, f->stream);
            f->current_window = fo.current_window;
        } else {
            rgba_frame_f32 fi = { in.data, in.full_window, in.current_window }, fo = { f->data, f->full_window, f->full_window };
            rc = cvs_perspective_f32_dev(&fo, self->n.source ? &fi : NULL, &p, f->stream);
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

static void pin_slot_dev(PyObject *o, int i, rgba_frame_dev *f) {
    py_pin *self = (py_pin *)o;
    py_rdlock(&self->n.lock);
    const bool direct = f->format == CVS_FORMAT_F16 && half_native(self->n.source);
    pthread_rwlock_unlock(&self->n.lock);
    if (direct) pin_render(o, i, f);                        /* widen, warp, truncate: one launch */
    else node_get_frame_dev(o, i, f, CVS_FORMAT_F32, pin_render);
}
static void pin_slot_32(PyObject *o, int i, rgba_frame_f32 *f) { node_get_frame_host32(o, i, f, CVS_FORMAT_F32, pin_render); }
static video_frame_source_funcs pin_funcs = {
    .flags = VIDEO_SOURCE_FLAG_DEVICE, .get_frame_32 = (video_get_frame_32_func)pin_slot_32,
    .get_frame_dev = (video_get_frame_dev_func)pin_slot_dev };
static PyObject *pin_capsule;

static PyObject *part_object(py_pin *self, int k) {
    PyObject *v = self->part[k].source ? self->part[k].source : self->given[k];
    Py_INCREF(v);
    return v;
}
static PyObject *pin_get_rect(py_pin *self, void *closure) { return part_object(self, PART_RECT); }
static int pin_set_rect(py_pin *self, PyObject *v, void *closure) { return parts_set(self, PART_RECT, 1, &v, true); }   /* a value that is refused leaves the old one */
static PyObject *pin_get_corners(py_pin *self, void *closure) {
    return Py_BuildValue("(NNNN)", part_object(self, PART_CORNER0), part_object(self, PART_CORNER0 + 1), part_object(self, PART_CORNER0 + 2), part_object(self, PART_CORNER0 + 3));
}
static int pin_set_corners(py_pin *self, PyObject *v, void *closure) {
    PyObject *items[4];
    if (corners_from(v, items) < 0) return -1;
    return parts_set(self, PART_CORNER0, 4, items, true);
}
static PyObject *pin_get_filter(py_pin *self, void *closure) {
    return PyUnicode_FromString(self->filter == CVS_TRANSFORM_NEAREST ? "nearest" : "bilinear");
}
static int pin_set_filter(py_pin *self, PyObject *v, void *closure) {
    const int filter = py_transform_filter_from(v);
    if (filter < 0) return -1;
    py_wrlock_nogil(&self->n.lock);
    self->filter = filter;
    pthread_rwlock_unlock(&self->n.lock);
    return 0;
}

static PyObject *pin_coefficients_at(py_pin *self, PyObject *args) {
    int frame_index;
    if (!PyArg_ParseTuple(args, "i", &frame_index)) return NULL;
    cvs_perspective p;
    box2i rect, bbox;
    py_rdlock(&self->n.lock);
    const int rc = coefficients(self, frame_index, &p, &rect, &bbox);
    pthread_rwlock_unlock(&self->n.lock);
    if (rc < 0) { PyErr_SetString(PyExc_ValueError, cvs_last_error()); return NULL; }
    if (rc > 0) Py_RETURN_NONE;
    return Py_BuildValue("((ddddddddd)(ii)(ii))", (double)p.h[0], (double)p.h[1], (double)p.h[2], (double)p.h[3], (double)p.h[4], (double)p.h[5],
                         (double)p.h[6], (double)p.h[7], (double)p.h[8], p.target_origin[0], p.target_origin[1], p.source_origin[0], p.source_origin[1]);
}

static PyMethodDef pin_methods[] = {
    { "set_source", (PyCFunction)node1_set_source, METH_VARARGS, "Sets the video source." },
    { "coefficients_at", (PyCFunction)pin_coefficients_at, METH_VARARGS,
      "coefficients_at(frame_index): (h, target_origin, source_origin) -- the nine f32 coefficients (target to source, each side counted from "
      "its origin) the frame is drawn with -- or None where the corners make no convex quad." },
    { NULL }
};
static PyGetSetDef pin_getset[] = {
    { VIDEO_FRAME_SOURCE_FUNCS, pyext_capsule_getter, NULL, "Video frame source C API.", &pin_capsule },
    { "source", (getter)node1_get_source, (setter)node1_set_source_attr, "The upstream video source." },
    { "source_rect", (getter)pin_get_rect, (setter)pin_set_rect, "The part of the source that is pinned (box2i or frame function)." },
    { "corners", (getter)pin_get_corners, (setter)pin_set_corners,
      "Where source_rect's top-left, top-right, bottom-right and bottom-left corners land (four pairs or frame functions)." },
    { "filter", (getter)pin_get_filter, (setter)pin_set_filter, "\"nearest\" or \"bilinear\" (alpha-weighted)." },
    { NULL }
};
static PyTypeObject py_type_CornerPin = {
    PyVarObject_HEAD_INIT(NULL, 0)
    .tp_name = "fluggo.media.process.VideoCornerPinFilter", .tp_basicsize = sizeof(py_pin), .tp_flags = Py_TPFLAGS_DEFAULT,
    .tp_base = &py_type_VideoSource, .tp_new = PyType_GenericNew, .tp_init = (initproc)pin_init,
    .tp_dealloc = (destructor)pin_dealloc, .tp_getset = pin_getset, .tp_methods = pin_methods,
};

int init_perspective(PyObject *module) {
    if (pyext_make_capsule(&pin_capsule, &pin_funcs) < 0) return -1;
    return pyext_add_type(module, "VideoCornerPinFilter", &py_type_CornerPin);
}
