/*
 * pyycc420.c -- the two 4:2:0 Y'CbCr nodes of fluggo.media.process (include/canvas_ycc420.h, DESIGN.md "4:2:0 Y'CbCr edges").
 *
 *   YCbCr420ReconstructionFilter(source, size, layout="nv12", matrix="709", range="studio", siting="left", transfer="709")
 *                                                                                       coded images -> VideoSource
 *   YCbCr420SubsampleFilter(source, size, layout="nv12", matrix="709", range="studio", siting="left", transfer="709")
 *                                                                                       VideoSource -> coded images
 *
 * No reference node.  layout: "planar8" (yuv420p), "planar10" (yuv420p10le), "nv12" or "p010"; matrix: "601", "709" or "2020";
 * range: "studio" or "full"; siting: "left", "center" or "topleft"; transfer: "709" or "none" (the frame holds the non-linear
 * R'G'B' codes: a VideoColorCorrectFilter applies PQ, HLG or a camera curve).  The planes cross PCIe exactly as the DV, MPEG-2 and
 * 4:2:2 nodes' do: both nodes go through pydv.c's py_planes_render and py_planes_from_source.
 */
#include "pyext.h"
#include "canvas_ycc420.h"

typedef struct { int width, height, layout, flags, planes; } ycc420_args;
static const pyext_choice layouts[] = { { "planar8", CVS_420_PLANAR8 }, { "planar10", CVS_420_PLANAR10 }, { "nv12", CVS_420_NV12 }, { "p010", CVS_420_P010 }, { NULL, 0 } };
static const pyext_choice matrices[] = { { "601", 0 }, { "709", CVS_YCC_REC709 }, { "2020", CVS_YCC_REC2020 }, { NULL, 0 } };
static const pyext_choice ranges[] = { { "studio", 0 }, { "full", CVS_YCC_FULL_RANGE }, { NULL, 0 } };
static const pyext_choice sitings[] = { { "left", 0 }, { "center", CVS_YCC_SITING_CENTER }, { "topleft", CVS_YCC_SITING_TOPLEFT }, { NULL, 0 } };
static const pyext_choice transfers[] = { { "709", 0 }, { "none", CVS_YCC_NO_TRANSFER }, { NULL, 0 } };

/* size and the five keywords as both nodes take them; false with a ValueError (or the parser's error) set */
static bool args_parse(const char *node, PyObject *args, PyObject *kw, PyObject **src, ycc420_args *a) {
    static char *kwlist[] = { "source", "size", "layout", "matrix", "range", "siting", "transfer", NULL };
    PyObject *size, *layout = NULL, *matrix = NULL, *range = NULL, *siting = NULL, *transfer = NULL;
    if (!PyArg_ParseTupleAndKeywords(args, kw, "OO|OOOOO", kwlist, src, &size, &layout, &matrix, &range, &siting, &transfer)) return false;
    v2i sz;
    if (!py_parse_v2i(size, &sz)) return false;
    int m, r, s, t;
    if (!pyext_choose(node, "layout", layout, layouts, CVS_420_NV12, &a->layout) || !pyext_choose(node, "matrix", matrix, matrices, CVS_YCC_REC709, &m) ||
        !pyext_choose(node, "range", range, ranges, 0, &r) || !pyext_choose(node, "siting", siting, sitings, 0, &s) ||
        !pyext_choose(node, "transfer", transfer, transfers, 0, &t))
        return false;
    a->flags = m | r | s | t;
    int strides[3], lines[3];
    a->planes = cvs_ycc420_layout(a->layout, sz.x, sz.y, strides, lines);
    if (a->planes < 0) {
        PyErr_Format(PyExc_ValueError, "%s: size (%d, %d): the width and the height must be even and at least 2", node, sz.x, sz.y);
        return false;
    }
    a->width = sz.x;
    a->height = sz.y;
    return true;
}

/* ---------------------------------------------------------------- YCbCr420ReconstructionFilter */

typedef struct { PyObject_HEAD CodedImageSourceHolder source; ycc420_args a; } py_ycc420recon;

static int recon_init(py_ycc420recon *self, PyObject *args, PyObject *kw) {
    PyObject *src;
    ycc420_args a;
    if (!args_parse("YCbCr420ReconstructionFilter", args, kw, &src, &a)) return -1;
    if (!py_coded_image_take_source(src, &self->source)) return -1;
    self->a = a;
    return 0;
}
static void recon_dealloc(py_ycc420recon *self) {
    py_coded_image_take_source(NULL, &self->source);
    Py_TYPE(self)->tp_free((PyObject *)self);
}

static int recon_entry(rgba_frame_f16 *out, const coded_image *dev, const void *node, cvs_stream_t s) {
    const ycc420_args *a = &((const py_ycc420recon *)node)->a;
    return cvs_reconstruct_420_dev(out, dev, a->width, a->height, a->layout, a->flags, s);
}
static void recon_render(PyObject *o, int frame_index, rgba_frame_dev *f) {
    py_planes_render(&((py_ycc420recon *)o)->source, ((py_ycc420recon *)o)->a.planes, recon_entry, o, frame_index, f);
}
DEFINE_NODE_VTABLE(recon, CVS_FORMAT_F16, 1, 0)
static void *recon_unused[] __attribute__((unused)) = { (void *)recon_slot_32 };
static PyGetSetDef recon_getset[] = { { VIDEO_FRAME_SOURCE_FUNCS, pyext_capsule_getter, NULL, "Video frame source C API.", &recon_capsule }, { NULL } };
static PyTypeObject py_type_YCbCr420ReconstructionFilter = {
    PyVarObject_HEAD_INIT(NULL, 0)
    .tp_name = "fluggo.media.process.YCbCr420ReconstructionFilter", .tp_basicsize = sizeof(py_ycc420recon), .tp_flags = Py_TPFLAGS_DEFAULT,
    .tp_base = &py_type_VideoSource, .tp_new = PyType_GenericNew, .tp_init = (initproc)recon_init,
    .tp_dealloc = (destructor)recon_dealloc, .tp_getset = recon_getset,
};

/* ---------------------------------------------------------------- YCbCr420SubsampleFilter */

typedef struct { PyObject_HEAD video_source *source; ycc420_args a; } py_ycc420sub;

static int sub_init(py_ycc420sub *self, PyObject *args, PyObject *kw) {
    PyObject *src;
    ycc420_args a;
    if (!args_parse("YCbCr420SubsampleFilter", args, kw, &src, &a)) return -1;
    if (!py_video_take_source(src, &self->source)) return -1;
    self->a = a;
    return 0;
}
static void sub_dealloc(py_ycc420sub *self) {
    py_video_take_source(NULL, &self->source);
    Py_TYPE(self)->tp_free((PyObject *)self);
}

static int sub_entry(coded_image *dev, const rgba_frame_f16 *in, const void *node, cvs_stream_t s) {
    const ycc420_args *a = node;
    return cvs_subsample_420_dev(dev, in, a->width, a->height, a->layout, a->flags, s);
}

/* a CodedImage with the least strides of cvs_ycc420_layout */
static coded_image *sub_get_frame(py_ycc420sub *self, int frame, int quality) {
    int strides[3], lines[3];
    const int planes = cvs_ycc420_layout(self->a.layout, self->a.width, self->a.height, strides, lines);
    if (planes < 0) return NULL;
    box2i window;
    box2i_set(&window, 0, 0, self->a.width - 1, self->a.height - 1);
    return py_planes_from_source(self->source, frame, &window, strides, lines, planes, sub_entry, &self->a);
}

static coded_image_source_funcs sub_funcs = { 0, (coded_image_getFrameFunc)sub_get_frame };
static PyObject *sub_capsule;
static PyGetSetDef sub_getset[] = { { CODED_IMAGE_SOURCE_FUNCS, pyext_capsule_getter, NULL, "Coded image source C API.", &sub_capsule }, { NULL } };
static PyTypeObject py_type_YCbCr420SubsampleFilter = {
    PyVarObject_HEAD_INIT(NULL, 0)
    .tp_name = "fluggo.media.process.YCbCr420SubsampleFilter", .tp_basicsize = sizeof(py_ycc420sub), .tp_flags = Py_TPFLAGS_DEFAULT,
    .tp_base = &py_type_CodedImageSource, .tp_new = PyType_GenericNew, .tp_init = (initproc)sub_init,
    .tp_dealloc = (destructor)sub_dealloc, .tp_getset = sub_getset,
};

int init_ycc420(PyObject *module) {
    sub_capsule = PyCapsule_New(&sub_funcs, CODED_IMAGE_SOURCE_FUNCS, NULL);
    if (!sub_capsule || pyext_make_capsule(&recon_capsule, &recon_funcs) < 0) return -1;
    if (pyext_add_type(module, "YCbCr420ReconstructionFilter", &py_type_YCbCr420ReconstructionFilter) < 0) return -1;
    return pyext_add_type(module, "YCbCr420SubsampleFilter", &py_type_YCbCr420SubsampleFilter);
}
