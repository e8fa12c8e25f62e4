/*
 * pywarp.c -- what the geometry nodes of fluggo.media.process share (pyext.h: warp_node): VideoTransformFilter (pytransform.c)
 * and VideoCornerPinFilter (pyperspective.c) differ in their coefficients, their constructors and their window rule only.
 *
 * A node's parts (source_rect, anchor, corners[0], ...) are numbers, pairs, boxes or frame functions, read as f32 like every v2f
 * of the path.  A pull: the source is pulled over the window the taps of the frame asked for can touch, clipped to source_rect,
 * into a pooled frame; the entry of the pulled format writes the frame; the node's window rule then reports the same window
 * whatever part of the source this pull reached, so that a frame pulled in tiles equals the frame pulled whole, window included.
 * f32 is the nodes' own format; an f16 pull over a half-native source goes through the _f16_dev entry in one launch.  Locking:
 * reader lock around the upstream pull and the parameters, writer lock where either is replaced.  A pull never raises: no
 * source, no device, no map or a refusing entry end in an empty window.
 */
#include "pyext.h"
#include <math.h>

/* ---------------------------------------------------------------- parts */

/* a constant of the shape the part takes, or a frame function, into a holder of its own: false with a Python error set */
static bool part_parse(const warp_part *part, PyObject *v, FrameFunctionHolder *fresh) {
    static const char *takes[] = { "a box2i", "a pair of numbers", "a number" };
    static const int counts[] = { 4, 2, 1 };
    framefunc_init(fresh, 0, 0, 0, 0);
    if (!v || v == Py_None) { PyErr_Format(PyExc_TypeError, "%s takes a value or a frame function", part->name); return false; }
    bool shaped;
    if (part->shape == WARP_BOX2I) shaped = PyTuple_Check(v) && PyTuple_GET_SIZE(v) == 2 && PyTuple_Check(PyTuple_GET_ITEM(v, 0)) && PyTuple_Check(PyTuple_GET_ITEM(v, 1));
    else if (part->shape == WARP_NUMBER) shaped = PyFloat_Check(v) || (PyLong_Check(v) && !PyBool_Check(v));
    else shaped = PyTuple_Check(v) && PyTuple_GET_SIZE(v) == 2 && !PyTuple_Check(PyTuple_GET_ITEM(v, 0));
    if (!shaped && (PyTuple_Check(v) || PyNumber_Check(v) || PyUnicode_Check(v) || PyBytes_Check(v))) {
        PyErr_Format(PyExc_TypeError, "%s takes %s or a frame function", part->name, takes[part->shape]);
        return false;
    }
    if (!py_framefunc_take_source(v, fresh)) return false;
    if (!fresh->source) {
        for (int i = 0; i < counts[part->shape]; i++)
            if (!isfinite(fresh->constant[i])) { PyErr_Format(PyExc_ValueError, "%s must be finite", part->name); return false; }
    }
    return true;
}

/* every value is parsed outside the lock, the parts are swapped under the writer lock, and what they held is released outside it */
int warp_parts_set(warp_node *self, int first, int count, PyObject **values, bool locked) {
    FrameFunctionHolder fresh[WARP_PARTS], old[WARP_PARTS];
    PyObject *old_given[WARP_PARTS];
    for (int i = 0; i < count; i++)
        if (!part_parse(&self->table[first + i], values[i], &fresh[i])) {
            for (int j = 0; j < i; j++) py_framefunc_take_source(NULL, &fresh[j]);
            return -1;
        }
    if (locked) py_wrlock_nogil(&self->n.lock);
    for (int i = 0; i < count; i++) {
        PyObject *keep = fresh[i].source ? NULL : values[i];
        Py_XINCREF(keep);
        old[i] = self->part[first + i];
        old_given[i] = self->given[first + i];
        self->part[first + i] = fresh[i];
        self->given[first + i] = keep;
    }
    if (locked) pthread_rwlock_unlock(&self->n.lock);
    for (int i = 0; i < count; i++) { py_framefunc_take_source(NULL, &old[i]); Py_XDECREF(old_given[i]); }
    return 0;
}

void warp_node_init(warp_node *self, const warp_part *table) {
    pthread_rwlock_init(&self->n.lock, NULL);
    self->table = table;
    self->filter = CVS_TRANSFORM_BILINEAR;
    for (int k = 0; k < WARP_PARTS; k++) framefunc_init(&self->part[k], 0, 0, 0, 0);
}
void warp_node_dealloc(warp_node *self) {
    py_video_take_source(NULL, &self->n.source);
    for (int k = 0; k < WARP_PARTS; k++) { py_framefunc_take_source(NULL, &self->part[k]); Py_CLEAR(self->given[k]); }
    pthread_rwlock_destroy(&self->n.lock);
    Py_TYPE(self)->tp_free((PyObject *)self);
}

PyObject *warp_get_part(warp_node *self, void *index) {
    const int k = (int)(size_t)index;
    PyObject *v = self->part[k].source ? self->part[k].source : self->given[k];
    Py_INCREF(v);
    return v;
}
int warp_set_part(warp_node *self, PyObject *value, void *index) { return warp_parts_set(self, (int)(size_t)index, 1, &value, true); }

/* ---------------------------------------------------------------- the filter */

int warp_filter_from(PyObject *v) {
    if (v && PyUnicode_Check(v)) {
        if (PyUnicode_CompareWithASCIIString(v, "nearest") == 0) return CVS_TRANSFORM_NEAREST;
        if (PyUnicode_CompareWithASCIIString(v, "bilinear") == 0) return CVS_TRANSFORM_BILINEAR;
        if (PyUnicode_CompareWithASCIIString(v, "catmull-rom") == 0) return CVS_TRANSFORM_CATMULL_ROM;
        PyErr_SetString(PyExc_ValueError, "filter is \"nearest\", \"bilinear\" or \"catmull-rom\"");
        return -1;
    }
    PyErr_SetString(PyExc_TypeError, "filter is the string \"nearest\", \"bilinear\" or \"catmull-rom\"");
    return -1;
}
PyObject *warp_get_filter(warp_node *self, void *closure) {
    return PyUnicode_FromString(self->filter == CVS_TRANSFORM_NEAREST ? "nearest" : (self->filter == CVS_TRANSFORM_CATMULL_ROM ? "catmull-rom" : "bilinear"));
}
int warp_set_filter(warp_node *self, PyObject *v, void *closure) {
    const int filter = warp_filter_from(v);
    if (filter < 0) return -1;
    py_wrlock_nogil(&self->n.lock);
    self->filter = filter;
    pthread_rwlock_unlock(&self->n.lock);
    return 0;
}

/* ---------------------------------------------------------------- the pull */

/* transparent black over `box` of `f` (its window is left alone): 0, or -1 */
static int clear_box(rgba_frame_dev *f, int x0, int y0, int x1, int y1) {
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

/* Which `all` and `win` is the node's own rule (fill_layer of pytransform.c: the layer's box grown to what the entry wrote;
 * of pyperspective.c: the quad's box, and what the entry wrote inside it); the strips are the same: above, below, left, right */
int warp_clear_around(rgba_frame_dev *f, const box2i *all, const box2i *win) {
    if (box2i_is_empty(win)) return clear_box(f, all->min.x, all->min.y, all->max.x, all->max.y);
    if (clear_box(f, all->min.x, all->min.y, all->max.x, win->min.y - 1) != 0 || clear_box(f, all->min.x, win->max.y + 1, all->max.x, all->max.y) != 0) return -1;
    if (clear_box(f, all->min.x, win->min.y, win->min.x - 1, win->max.y) != 0 || clear_box(f, win->max.x + 1, win->min.y, all->max.x, win->max.y) != 0) return -1;
    return 0;
}

/* `f` in either format: the source pulled in that format over the window the taps need, then the library entry of that format */
void warp_render(warp_node *self, int frame_index, rgba_frame_dev *f, const warp_ops *ops) {
    py_rdlock(&self->n.lock);
    warp_plan p = { .layer = { { 0, 0 }, { -1, -1 } } };
    rgba_frame_dev in = { NULL, f->format, { { 0, 0 }, { -1, -1 } }, { { 0, 0 }, { -1, -1 } }, f->stream };
    ops->plan(self, frame_index, &f->full_window, &p);
    bool draw = p.sound, beyond = false;          /* beyond: the frame asked for reaches nothing of source_rect */
    if (draw && self->n.source) {
        box2i_intersect(&p.need, &p.need, &p.rect);
        beyond = box2i_is_empty(&p.need);
        draw = !beyond;
    }
    if (draw && self->n.source) {
        in.full_window = in.current_window = p.need;
        /* a window the entry will refuse is not pulled: the entry is still called, for its message */
        if (!p.refused) {
            in.data = cvs_pool_malloc(frame_bytes(&p.need, f->format), f->stream);
            if (!in.data) draw = false;
            else video_get_frame_dev(self->n.source, frame_index, &in);
        }
    }
    int rc = -1;
    if (draw) {
        /* without a source the entry gets none, and says so */
        if (f->format == CVS_FORMAT_F16) {
            rgba_frame_f16 fi = { in.data, in.full_window, in.current_window }, fo = { f->data, f->full_window, f->full_window };
            rc = ops->entry(f->format, &fo, self->n.source ? &fi : NULL, &p, f->stream);
            f->current_window = fo.current_window;
        } else {
            rgba_frame_f32 fi = { in.data, in.full_window, in.current_window }, fo = { f->data, f->full_window, f->full_window };
            rc = ops->entry(f->format, &fo, self->n.source ? &fi : NULL, &p, f->stream);
            f->current_window = fo.current_window;
        }
    } else if (beyond) {
        /* the entry has nothing to write; the layer's box is still reported */
        rc = 0;
        box2i_set_empty(&f->current_window);
    }
    if (rc == 0 && self->n.source) rc = ops->fill_layer(f, &p.layer);
    pthread_rwlock_unlock(&self->n.lock);
    if (rc != 0) box2i_set_empty(&f->current_window);
    if (in.data) cvs_pool_free(in.data, f->stream);
}
