/*
 * pyperspective.c -- the corner pin of fluggo.media.process: a layer put onto a surface that is not parallel to the screen, its
 * four corners pinned to four points, interpolated alpha-weighted so that the layer's edge keeps its colour.
 *
 * No reference code.  Contract: DESIGN.md "Corner pin".
 *   VideoCornerPinFilter(source, source_rect, corners, filter="bilinear")          cvs_perspective_f32_dev / _f16_dev
 * corners: where the top-left, top-right, bottom-right and bottom-left corners of source_rect's outer edges (min - 1/2 ..
 * max + 1/2) land, each a pair or a frame function, read as f32 like every v2f of the path; cvs_perspective_from_quad turns them
 * into the nine target -> source coefficients and the two origins, which coefficients_at(frame_index) shows.  The pull, the part
 * table, the filter attribute and the locking are pywarp.c's; here are the coefficients, the source window
 * (cvs_perspective_source_window of the frame asked for, clipped to source_rect) and the window reported: the quad's bounding box
 * [floor(min) - 1, ceil(max) + 1] cropped to the frame asked for, whatever part of the source this pull reached (fill_layer), so
 * a frame pulled in tiles equals the frame pulled whole, window included.  A quad that is not convex ends in an empty window.
 */
#include "pyext.h"
#include <math.h>

enum { PART_RECT, PART_CORNER0 };
static const warp_part pin_parts[WARP_PARTS] = {
    { "source_rect", WARP_BOX2I }, { "corners[0]", WARP_PAIR }, { "corners[1]", WARP_PAIR }, { "corners[2]", WARP_PAIR }, { "corners[3]", WARP_PAIR } };
typedef warp_node py_pin;

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
    warp_node_init(self, pin_parts);
    if (!PyArg_ParseTupleAndKeywords(args, kw, "OOO|O", kwlist, &src, &rect, &corners, &filter)) return -1;
    if (filter && (self->filter = warp_filter_from(filter)) < 0) return -1;
    if (warp_parts_set(self, PART_RECT, 1, &rect, false) < 0) return -1;
    if (corners_from(corners, items) < 0 || warp_parts_set(self, PART_CORNER0, 4, items, false) < 0) return -1;
    return py_video_take_source(src, &self->n.source) ? 0 : -1;
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
 * bounding box in the frame asked for, of which the entry has written f->current_window (the part the pulled source reaches).
 * Unlike the affine node's, the entry's window is cropped to `layer` and not joined to it: it is the whole frame wherever a
 * corner of the pulled part lies beyond the vanishing line, and all of that outside the quad's box is nothing.  The rest of
 * `layer` is made transparent black (DESIGN.md "Affine transform", Node, has the reason).  0, or -1 */
static int fill_layer(rgba_frame_dev *f, const box2i *layer) {
    box2i win;
    box2i_intersect(&win, &f->current_window, layer);
    f->current_window = *layer;
    if (box2i_is_empty(layer)) { box2i_set_empty(&f->current_window); return 0; }
    return warp_clear_around(f, layer, &win);
}

static bool within_span(const box2i *b, const int origin[2]) {
    const long long lim = CVS_PERSPECTIVE_MAX_SPAN;
    return (long long)b->min.x - origin[0] >= -lim && (long long)b->min.y - origin[1] >= -lim && (long long)b->max.x - origin[0] <= lim && (long long)b->max.y - origin[1] <= lim;
}

static void pin_plan(warp_node *self, int frame_index, const box2i *full, warp_plan *p) {
    box2i bbox, pulled;
    p->sound = coefficients(self, frame_index, &p->c.pin, &p->rect, &bbox) == 0 && cvs_perspective_source_window(&p->c.pin, full, &p->need) == 0;
    if (!p->sound) return;
    box2i_intersect(&p->layer, &bbox, full);
    box2i_intersect(&pulled, &p->need, &p->rect);
    p->refused = !(within_span(&pulled, p->c.pin.source_origin) && within_span(full, p->c.pin.target_origin));
}
static int pin_entry(int format, void *out, const void *in, const warp_plan *p, void *stream) {
    return format == CVS_FORMAT_F16 ? cvs_perspective_f16_dev(out, in, &p->c.pin, stream) : cvs_perspective_f32_dev(out, in, &p->c.pin, stream);
}

static const warp_ops pin_ops = { pin_plan, pin_entry, fill_layer };
static void pin_render(PyObject *o, int frame_index, rgba_frame_dev *f) { warp_render((warp_node *)o, frame_index, f, &pin_ops); }
DEFINE_NODE_VTABLE_HALF_DIRECT(pin)                   /* widen, warp, truncate: one launch */

static PyObject *pin_get_corners(py_pin *self, void *closure) {
    return Py_BuildValue("(NNNN)", warp_get_part(self, (void *)(size_t)PART_CORNER0), warp_get_part(self, (void *)(size_t)(PART_CORNER0 + 1)),
                         warp_get_part(self, (void *)(size_t)(PART_CORNER0 + 2)), warp_get_part(self, (void *)(size_t)(PART_CORNER0 + 3)));
}
static int pin_set_corners(py_pin *self, PyObject *v, void *closure) {
    PyObject *items[4];
    if (corners_from(v, items) < 0) return -1;
    return warp_parts_set(self, PART_CORNER0, 4, items, true);
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
    { "source_rect", (getter)warp_get_part, (setter)warp_set_part, "The part of the source that is pinned (box2i or frame function)." },
    { "corners", (getter)pin_get_corners, (setter)pin_set_corners,
      "Where source_rect's top-left, top-right, bottom-right and bottom-left corners land (four pairs or frame functions)." },
    { "filter", (getter)warp_get_filter, (setter)warp_set_filter, "\"nearest\", \"bilinear\" or \"catmull-rom\" (both alpha-weighted; the cubic never leaves the range of its 4 x 4 samples)." },
    { NULL }
};
static PyTypeObject py_type_CornerPin = {
    PyVarObject_HEAD_INIT(NULL, 0)
    .tp_name = "fluggo.media.process.VideoCornerPinFilter", .tp_basicsize = sizeof(py_pin), .tp_flags = Py_TPFLAGS_DEFAULT,
    .tp_base = &py_type_VideoSource, .tp_new = PyType_GenericNew, .tp_init = (initproc)pin_init,
    .tp_dealloc = (destructor)warp_node_dealloc, .tp_getset = pin_getset, .tp_methods = pin_methods,
};

int init_perspective(PyObject *module) {
    if (pyext_make_capsule(&pin_capsule, &pin_funcs) < 0) return -1;
    return pyext_add_type(module, "VideoCornerPinFilter", &py_type_CornerPin);
}
