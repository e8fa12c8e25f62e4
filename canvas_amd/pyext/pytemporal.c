/*
 * pytemporal.c -- the temporal noise reducer of fluggo.media.process: a frame averaged with the frames around it in time where
 * nothing moved.
 *
 * No reference code (the reference has no temporal filter).  Contract: DESIGN.md "Temporal denoise".  Output frame i of
 *   VideoTemporalDenoiseFilter(source, radius=1, threshold=0.02, softness=0.04, channels="rgba")
 *                                       denoise(source[i - radius] .. source[i] .. source[i + radius])
 * radius is 1 (three frames) or 2 (five); threshold and softness are numbers or frame functions, evaluated at the OUTPUT frame;
 * channels is a string of distinct letters from "rgba" (pymedian.c's parser), read back in that order.  With channels="a" it is
 * the temporal matte smoother.  The node is f16-native on the device slot and a thin caller of cvs_temporal_denoise_f16_dev
 * (include/canvas_temporal.h).  The 2 * radius + 1 source frames are pulled into pooled device scratch over the request grown by
 * one pixel on all four sides (the entry reads a 3 x 3 neighbourhood), so the result does not depend on how a consumer tiles its
 * requests.  A neighbour whose pull comes back empty, or whose index would leave int, is absent: the start and the end of a clip
 * are denoised against the neighbours they have.  Locking as in pydeint.c and pymedian.c.
 */
#include "pyext.h"
#include "canvas_temporal.h"
#include <limits.h>

typedef struct { node1 n; int radius, channels; FrameFunctionHolder threshold, softness; } py_temporal;

/* an int 1 or 2 -> itself; 0 with a Python error set */
static int parse_radius(PyObject *obj) {
    if (!obj || !PyLong_Check(obj) || PyBool_Check(obj)) { PyErr_SetString(PyExc_TypeError, "radius is an int: 1 (three frames) or 2 (five frames)"); return 0; }
    const long v = PyLong_AsLong(obj);
    if (v == -1 && PyErr_Occurred()) return 0;
    if (v != 1 && v != 2) { PyErr_SetString(PyExc_ValueError, "radius is 1 (three frames) or 2 (five frames)"); return 0; }
    return (int)v;
}

static int temporal_init(py_temporal *self, PyObject *args, PyObject *kw) {
    static char *kwlist[] = { "source", "radius", "threshold", "softness", "channels", NULL };
    PyObject *src, *radius = NULL, *threshold = NULL, *softness = NULL, *channels = NULL;
    pthread_rwlock_init(&self->n.lock, NULL);
    framefunc_init(&self->threshold, 0.02, 0, 0, 0);
    framefunc_init(&self->softness, 0.04, 0, 0, 0);
    self->radius = 1;
    self->channels = CVS_MEDIAN_ALL;
    if (!PyArg_ParseTupleAndKeywords(args, kw, "O|OOOO", kwlist, &src, &radius, &threshold, &softness, &channels)) return -1;
    if (radius && !(self->radius = parse_radius(radius))) return -1;
    if (channels && (self->channels = py_channels_parse(channels)) < 0) return -1;
    if (!py_video_take_source(src, &self->n.source)) return -1;
    if (threshold && (threshold == Py_None || !py_framefunc_take_source(threshold, &self->threshold))) { if (!PyErr_Occurred()) PyErr_SetString(PyExc_TypeError, "threshold takes a number or a frame function"); return -1; }
    if (softness && (softness == Py_None || !py_framefunc_take_source(softness, &self->softness))) { if (!PyErr_Occurred()) PyErr_SetString(PyExc_TypeError, "softness takes a number or a frame function"); return -1; }
    return 0;
}
static void temporal_dealloc(py_temporal *self) {
    py_video_take_source(NULL, &self->n.source);
    py_framefunc_take_source(NULL, &self->threshold);
    py_framefunc_take_source(NULL, &self->softness);
    pthread_rwlock_destroy(&self->n.lock);
    Py_TYPE(self)->tp_free((PyObject *)self);
}

/* one source frame into pooled scratch over `full`; data NULL (no device, no memory) or an empty window: absent */
static rgba_frame_dev pull_scratch(py_temporal *self, int frame_index, const rgba_frame_dev *f, const box2i *full) {
    rgba_frame_dev t = { NULL, CVS_FORMAT_F16, *full, *full, f->stream };
    t.data = cvs_pool_malloc(frame_bytes(full, CVS_FORMAT_F16), f->stream);
    if (!t.data) { box2i_set_empty(&t.current_window); return t; }
    py_rdlock(&self->n.lock);
    video_get_frame_dev(self->n.source, frame_index, &t);
    pthread_rwlock_unlock(&self->n.lock);
    return t;
}

/* output frame i from source frames i - radius .. i + radius */
static void temporal_render(PyObject *o, int i, rgba_frame_dev *f) {
    py_temporal *self = (py_temporal *)o;
    if (box2i_is_empty(&f->full_window)) { box2i_set_empty(&f->current_window); return; }
    box2i grown = f->full_window;
    if (grown.min.x > -CVS_MAX_COORD) grown.min.x--;
    if (grown.min.y > -CVS_MAX_COORD) grown.min.y--;
    if (grown.max.x < CVS_MAX_COORD) grown.max.x++;
    if (grown.max.y < CVS_MAX_COORD) grown.max.y++;
    py_rdlock(&self->n.lock);
    const cvs_temporal_denoise p = { framefunc_get_f32(&self->threshold, i), framefunc_get_f32(&self->softness, i), self->channels, 0 };
    const int radius = self->radius;
    pthread_rwlock_unlock(&self->n.lock);

    /* t[0 .. 4]: frames i - 2 .. i + 2; those not pulled keep data NULL */
    rgba_frame_dev t[5] = { { NULL }, { NULL }, { NULL }, { NULL }, { NULL } };
    rgba_frame_f16 h[5], fo = { f->data, f->full_window, f->full_window };
    t[2] = pull_scratch(self, i, f, &grown);
    if (t[2].data && !box2i_is_empty(&t[2].current_window)) {
        for (int d = -radius; d <= radius; d++) {
            if (d == 0 || (d < 0 ? i < INT_MIN - d : i > INT_MAX - d)) continue;
            t[2 + d] = pull_scratch(self, i + d, f, &grown);
        }
        for (int k = 0; k < 5; k++) h[k] = (rgba_frame_f16){ t[k].data, t[k].full_window, t[k].current_window };
        if (cvs_temporal_denoise_f16_dev(&fo, t[0].data ? &h[0] : NULL, t[1].data ? &h[1] : NULL, &h[2], t[3].data ? &h[3] : NULL,
                                         t[4].data ? &h[4] : NULL, &p, f->stream) != 0) box2i_set_empty(&fo.current_window);
    } else box2i_set_empty(&fo.current_window);
    f->current_window = fo.current_window;
    for (int k = 0; k < 5; k++) cvs_pool_free(t[k].data, f->stream);
}

DEFINE_NODE_VTABLE(temporal, CVS_FORMAT_F16, 1, 0)
static void *temporal_unused[] __attribute__((unused)) = { (void *)temporal_slot_32 };

static int temporal_set_holder(py_temporal *self, PyObject *v, void *closure) {
    if (!v || v == Py_None) { PyErr_SetString(PyExc_TypeError, "the attribute takes a number or a frame function"); return -1; }
    return node1_set_holder(&self->n, NODE1_HOLDER_AT(self, closure), v);
}
static PyObject *temporal_get_radius(py_temporal *self, void *closure) { return PyLong_FromLong(self->radius); }
static int temporal_set_radius(py_temporal *self, PyObject *v, void *closure) {
    const int radius = parse_radius(v);
    if (!radius) return -1;
    py_wrlock_nogil(&self->n.lock);
    self->radius = radius;
    pthread_rwlock_unlock(&self->n.lock);
    return 0;
}
static PyObject *temporal_get_channels(py_temporal *self, void *closure) { return py_channels_string(self->channels); }
static int temporal_set_channels(py_temporal *self, PyObject *v, void *closure) {
    const int mask = py_channels_parse(v);
    if (mask < 0) return -1;
    py_wrlock_nogil(&self->n.lock);
    self->channels = mask;
    pthread_rwlock_unlock(&self->n.lock);
    return 0;
}

static PyGetSetDef temporal_getset[] = {
    { VIDEO_FRAME_SOURCE_FUNCS, pyext_capsule_getter, NULL, "Video frame source C API.", &temporal_capsule },
    { "source", (getter)node1_get_source, (setter)node1_set_source_attr, "The upstream video source." },
    { "radius", (getter)temporal_get_radius, (setter)temporal_set_radius, "1: the frame is averaged with the one before and the one after it, 2: with two on each side." },
    { "threshold", (getter)node1_get_scalar, (setter)temporal_set_holder,
      "Largest difference to a neighbouring frame that still counts as nothing moved (number or frame function).", NODE1_HOLDER(py_temporal, threshold) },
    { "softness", (getter)node1_get_scalar, (setter)temporal_set_holder,
      "Width of the ramp from averaged to untouched beyond threshold; 0: a hard switch (number or frame function).", NODE1_HOLDER(py_temporal, softness) },
    { "channels", (getter)temporal_get_channels, (setter)temporal_set_channels, "The channels compared and averaged, letters from \"rgba\"; the others pass code for code." },
    { NULL }
};
static PyTypeObject py_type_Temporal = {
    PyVarObject_HEAD_INIT(NULL, 0)
    .tp_name = "fluggo.media.process.VideoTemporalDenoiseFilter", .tp_basicsize = sizeof(py_temporal), .tp_flags = Py_TPFLAGS_DEFAULT,
    .tp_base = &py_type_VideoSource, .tp_new = PyType_GenericNew, .tp_init = (initproc)temporal_init,
    .tp_dealloc = (destructor)temporal_dealloc, .tp_getset = temporal_getset, .tp_methods = node1_methods,
};

int init_temporal(PyObject *module) {
    if (pyext_make_capsule(&temporal_capsule, &temporal_funcs) < 0) return -1;
    return pyext_add_type(module, "VideoTemporalDenoiseFilter", &py_type_Temporal);
}
