/*
 * pytransform.c -- the geometry node of fluggo.media.process beside VideoScaler: rotate, scale, mirror and move a layer about an
 * anchor point, interpolated alpha-weighted so that the layer's edge keeps its colour.
 *
 * No reference code.  Contract: DESIGN.md "Affine transform".
 *   VideoTransformFilter(source, source_rect, anchor=(0, 0), scale=(1, 1), rotation=0.0, position=(0, 0), filter="bilinear")
 *                                                                    cvs_transform_f32_dev / _f16_dev
 * A source point p lands on  position + R(rotation) * diag(scale) * (p - anchor), rotation in degrees, clockwise on screen.  The
 * parts are numbers, pairs or frame functions, read as f32 like every v2f of the path; cvs_transform_from_parts turns them into the
 * six target -> source coefficients, which inverse_at(frame_index) shows.  The pull, the part table, the filter attribute and
 * the locking are pywarp.c's; here are the coefficients, the source window (cvs_transform_source_window of the frame asked for,
 * clipped to source_rect) and the window reported: where source_rect lands in the frame asked for (fill_layer).  Coordinates are
 * absolute, so a frame pulled in tiles equals the frame pulled whole, window included.  A degenerate scale ends in an empty
 * window.
 */
#include "pyext.h"

enum { PART_RECT, PART_ANCHOR, PART_SCALE, PART_ROTATION, PART_POSITION };
static const warp_part transform_parts[WARP_PARTS] = {
    { "source_rect", WARP_BOX2I }, { "anchor", WARP_PAIR }, { "scale", WARP_PAIR }, { "rotation", WARP_NUMBER }, { "position", WARP_PAIR } };
typedef warp_node py_transform;

static int transform_init(py_transform *self, PyObject *args, PyObject *kw) {
    static char *kwlist[] = { "source", "source_rect", "anchor", "scale", "rotation", "position", "filter", NULL };
    PyObject *src, *given[WARP_PARTS] = { NULL }, *filter = NULL;
    warp_node_init(self, transform_parts);
    if (!PyArg_ParseTupleAndKeywords(args, kw, "OO|OOOOO", kwlist, &src, &given[PART_RECT], &given[PART_ANCHOR], &given[PART_SCALE],
                                     &given[PART_ROTATION], &given[PART_POSITION], &filter)) return -1;
    if (filter && (self->filter = warp_filter_from(filter)) < 0) return -1;
    PyObject *defaults[WARP_PARTS] = { NULL, Py_BuildValue("(dd)", 0.0, 0.0), Py_BuildValue("(dd)", 1.0, 1.0), PyFloat_FromDouble(0.0), Py_BuildValue("(dd)", 0.0, 0.0) };
    bool ok = true;
    for (int k = 1; k < WARP_PARTS; k++) {
        if (!defaults[k]) ok = false;
        if (!given[k]) given[k] = defaults[k];
    }
    ok = ok && warp_parts_set(self, 0, WARP_PARTS, given, false) == 0;
    for (int k = 1; k < WARP_PARTS; k++) Py_XDECREF(defaults[k]);
    if (!ok) { if (!PyErr_Occurred()) PyErr_NoMemory(); return -1; }
    return py_video_take_source(src, &self->n.source) ? 0 : -1;
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

/* source_rect bounds what is pulled, as VideoScaler's does; the layer is where it lands in the frame asked for */
static void transform_plan(warp_node *self, int frame_index, const box2i *full, warp_plan *p) {
    cvs_transform *t = &p->c.affine;
    *t = (cvs_transform){ { 0 }, self->filter, 0 };
    p->sound = coefficients(self, frame_index, t->m) == 0 && cvs_transform_source_window(t, full, &p->need) == 0;
    if (!p->sound || !self->n.source) return;
    framefunc_get_box2i(&p->rect, &self->part[PART_RECT], frame_index);
    if (cvs_transform_target_window(t, &p->rect, full, &p->layer) != 0) box2i_set_empty(&p->layer);
    const int lim = CVS_TRANSFORM_MAX_COORD;
    box2i pulled;
    box2i_intersect(&pulled, &p->need, &p->rect);
    p->refused = pulled.min.x < -lim || pulled.min.y < -lim || pulled.max.x > lim || pulled.max.y > lim;
}
static int transform_entry(int format, void *out, const void *in, const warp_plan *p, void *stream) {
    return format == CVS_FORMAT_F16 ? cvs_transform_f16_dev(out, in, &p->c.affine, stream) : cvs_transform_f32_dev(out, in, &p->c.affine, stream);
}

/* The window the node reports does not depend on how much of the source this pull happened to ask for: it is where source_rect
 * lands in the frame asked for, `layer`, grown to `win`, what the entry has written of it (the part the pulled source reaches,
 * which the entry's own rounding may put a pixel outside `layer`: the node reports their union so that nothing written is cut
 * off); the rest is transparent black.  With the entry's own window a node above would see a window that varies with the tile
 * it is pulled in, and a blur's or a matte's result would vary with it (DESIGN.md "Affine transform", Node).  0, or -1 */
static int fill_layer(rgba_frame_dev *f, const box2i *layer) {
    box2i win = f->current_window, all = *layer;
    if (box2i_is_empty(&all)) return 0;
    if (!box2i_is_empty(&win)) {
        if (win.min.x < all.min.x) all.min.x = win.min.x;
        if (win.min.y < all.min.y) all.min.y = win.min.y;
        if (win.max.x > all.max.x) all.max.x = win.max.x;
        if (win.max.y > all.max.y) all.max.y = win.max.y;
    }
    f->current_window = all;
    return warp_clear_around(f, &all, &win);
}

static const warp_ops transform_ops = { transform_plan, transform_entry, fill_layer };
static void transform_render(PyObject *o, int frame_index, rgba_frame_dev *f) { warp_render((warp_node *)o, frame_index, f, &transform_ops); }
DEFINE_NODE_VTABLE_HALF_DIRECT(transform)             /* widen, warp, truncate: one launch */

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
    { "source_rect", (getter)warp_get_part, (setter)warp_set_part, "The part of the source that is drawn (box2i or frame function).", PART(PART_RECT) },
    { "anchor", (getter)warp_get_part, (setter)warp_set_part, "The source point that scale and rotation leave in place (pair or frame function).", PART(PART_ANCHOR) },
    { "scale", (getter)warp_get_part, (setter)warp_set_part, "Scale factors along x and y, negative to mirror (pair or frame function).", PART(PART_SCALE) },
    { "rotation", (getter)warp_get_part, (setter)warp_set_part, "Degrees, clockwise on screen (number or frame function).", PART(PART_ROTATION) },
    { "position", (getter)warp_get_part, (setter)warp_set_part, "Where the anchor lands in the target (pair or frame function).", PART(PART_POSITION) },
    { "filter", (getter)warp_get_filter, (setter)warp_set_filter, "\"nearest\", \"bilinear\" or \"catmull-rom\" (both alpha-weighted; the cubic never leaves the range of its 4 x 4 samples)." },
    { NULL }
};
static PyTypeObject py_type_Transform = {
    PyVarObject_HEAD_INIT(NULL, 0)
    .tp_name = "fluggo.media.process.VideoTransformFilter", .tp_basicsize = sizeof(py_transform), .tp_flags = Py_TPFLAGS_DEFAULT,
    .tp_base = &py_type_VideoSource, .tp_new = PyType_GenericNew, .tp_init = (initproc)transform_init,
    .tp_dealloc = (destructor)warp_node_dealloc, .tp_getset = transform_getset, .tp_methods = transform_methods,
};

int init_transform(PyObject *module) {
    if (pyext_make_capsule(&transform_capsule, &transform_funcs) < 0) return -1;
    return pyext_add_type(module, "VideoTransformFilter", &py_type_Transform);
}
