/*
 * pyycc422.c -- the two 4:2:2 Y'CbCr nodes of fluggo.media.process (include/canvas_ycc422.h, DESIGN.md "4:2:2 Y'CbCr edges").
 *
 *   YCbCr422ReconstructionFilter(source, size, layout="v210", matrix="709")   coded images -> VideoSource
 *   YCbCr422SubsampleFilter(source, size, layout="v210", matrix="709")        VideoSource -> coded images
 *
 * No reference node: the reference's decoder hands 4:2:2 images out (src/libav/AVVideoDecoder.c:72-91) and nothing reads them.
 * layout: "planar8" (yuv422p), "planar10" (yuv422p10le), "uyvy" (2vuy) or "v210"; matrix: "601" or "709".  The planes cross PCIe
 * exactly as the DV and MPEG-2 nodes' do: both nodes go through pydv.c's py_planes_render and py_planes_from_source.
 */
#include "pyext.h"
#include "canvas_ycc422.h"

typedef struct { int width, height, layout, flags, planes; } ycc422_args;

static const pyext_choice layouts[] = { { "planar8", CVS_422_PLANAR8 }, { "planar10", CVS_422_PLANAR10 }, { "uyvy", CVS_422_UYVY }, { "v210", CVS_422_V210 }, { NULL, 0 } };
static const pyext_choice matrices[] = { { "601", 0 }, { "709", CVS_YCC_REC709 }, { NULL, 0 } };

/* size and the two keywords as both nodes take them; false with a ValueError (or the parser's error) set */
static bool args_parse(const char *node, PyObject *args, PyObject *kw, PyObject **src, ycc422_args *a) {
    static char *kwlist[] = { "source", "size", "layout", "matrix", NULL };
    PyObject *size, *layout = NULL, *matrix = NULL;
    if (!PyArg_ParseTupleAndKeywords(args, kw, "OO|OO", kwlist, src, &size, &layout, &matrix)) return false;
    v2i sz;
    if (!py_parse_v2i(size, &sz)) return false;
    if (!pyext_choose(node, "layout", layout, layouts, CVS_422_V210, &a->layout) || !pyext_choose(node, "matrix", matrix, matrices, CVS_YCC_REC709, &a->flags))
        return false;
    int strides[3], lines[3];
    a->planes = cvs_ycc422_layout(a->layout, sz.x, sz.y, strides, lines);
    if (a->planes < 0) {
        PyErr_Format(PyExc_ValueError, "%s: size (%d, %d): the width must be even and at least 2, the height at least 1", node, sz.x, sz.y);
        return false;
    }
    a->width = sz.x;
    a->height = sz.y;
    return true;
}

/* ---------------------------------------------------------------- YCbCr422ReconstructionFilter */

typedef struct { PyObject_HEAD CodedImageSourceHolder source; ycc422_args a; } py_ycc422recon;

static int recon_init(py_ycc422recon *self, PyObject *args, PyObject *kw) {
    PyObject *src;
    ycc422_args a;
    if (!args_parse("YCbCr422ReconstructionFilter", args, kw, &src, &a)) return -1;
    if (!py_coded_image_take_source(src, &self->source)) return -1;
    self->a = a;
    return 0;
}
static void recon_dealloc(py_ycc422recon *self) {
    py_coded_image_take_source(NULL, &self->source);
    Py_TYPE(self)->tp_free((PyObject *)self);
}

static int recon_entry(rgba_frame_f16 *out, const coded_image *dev, const void *node, cvs_stream_t s) {
    const ycc422_args *a = &((const py_ycc422recon *)node)->a;
    return cvs_reconstruct_422_dev(out, dev, a->width, a->height, a->layout, a->flags, s);
}
static void recon_render(PyObject *o, int frame_index, rgba_frame_dev *f) {
    py_planes_render(&((py_ycc422recon *)o)->source, ((py_ycc422recon *)o)->a.planes, recon_entry, o, frame_index, f);
}
DEFINE_NODE_VTABLE(recon, CVS_FORMAT_F16, 1, 0)
static void *recon_unused[] __attribute__((unused)) = { (void *)recon_slot_32 };
static PyGetSetDef recon_getset[] = { { VIDEO_FRAME_SOURCE_FUNCS, pyext_capsule_getter, NULL, "Video frame source C API.", &recon_capsule }, { NULL } };
static PyTypeObject py_type_YCbCr422ReconstructionFilter = {
    PyVarObject_HEAD_INIT(NULL, 0)
    .tp_name = "fluggo.media.process.YCbCr422ReconstructionFilter", .tp_basicsize = sizeof(py_ycc422recon), .tp_flags = Py_TPFLAGS_DEFAULT,
    .tp_base = &py_type_VideoSource, .tp_new = PyType_GenericNew, .tp_init = (initproc)recon_init,
    .tp_dealloc = (destructor)recon_dealloc, .tp_getset = recon_getset,
};

/* ---------------------------------------------------------------- YCbCr422SubsampleFilter */

typedef struct { PyObject_HEAD video_source *source; ycc422_args a; } py_ycc422sub;

static int sub_init(py_ycc422sub *self, PyObject *args, PyObject *kw) {
    PyObject *src;
    ycc422_args a;
    if (!args_parse("YCbCr422SubsampleFilter", args, kw, &src, &a)) return -1;
    if (!py_video_take_source(src, &self->source)) return -1;
    self->a = a;
    return 0;
}
static void sub_dealloc(py_ycc422sub *self) {
    py_video_take_source(NULL, &self->source);
    Py_TYPE(self)->tp_free((PyObject *)self);
}

static int sub_entry(coded_image *dev, const rgba_frame_f16 *in, const void *node, cvs_stream_t s) {
    const ycc422_args *a = node;
    return cvs_subsample_422_dev(dev, in, a->width, a->height, a->layout, a->flags, s);
}

/* a CodedImage with the least strides of cvs_ycc422_layout */
static coded_image *sub_get_frame(py_ycc422sub *self, int frame, int quality) {
    int strides[3], lines[3];
    const int planes = cvs_ycc422_layout(self->a.layout, self->a.width, self->a.height, strides, lines);
    if (planes < 0) return NULL;
    box2i window;
    box2i_set(&window, 0, 0, self->a.width - 1, self->a.height - 1);
    return py_planes_from_source(self->source, frame, &window, strides, lines, planes, sub_entry, &self->a);
}

static coded_image_source_funcs sub_funcs = { 0, (coded_image_getFrameFunc)sub_get_frame };
static PyObject *sub_capsule;
static PyGetSetDef sub_getset[] = { { CODED_IMAGE_SOURCE_FUNCS, pyext_capsule_getter, NULL, "Coded image source C API.", &sub_capsule }, { NULL } };
static PyTypeObject py_type_YCbCr422SubsampleFilter = {
    PyVarObject_HEAD_INIT(NULL, 0)
    .tp_name = "fluggo.media.process.YCbCr422SubsampleFilter", .tp_basicsize = sizeof(py_ycc422sub), .tp_flags = Py_TPFLAGS_DEFAULT,
    .tp_base = &py_type_CodedImageSource, .tp_new = PyType_GenericNew, .tp_init = (initproc)sub_init,
    .tp_dealloc = (destructor)sub_dealloc, .tp_getset = sub_getset,
};

int init_ycc422(PyObject *module) {
    sub_capsule = PyCapsule_New(&sub_funcs, CODED_IMAGE_SOURCE_FUNCS, NULL);
    if (!sub_capsule || pyext_make_capsule(&recon_capsule, &recon_funcs) < 0) return -1;
    if (pyext_add_type(module, "YCbCr422ReconstructionFilter", &py_type_YCbCr422ReconstructionFilter) < 0) return -1;
    return pyext_add_type(module, "YCbCr422SubsampleFilter", &py_type_YCbCr422SubsampleFilter);
}
