/*
 * pydv.c -- coded-image sources, the two DV 4:1:1 nodes and the MPEG-2 4:2:0 node.
 *
 *   CodedImageSource, CodedImage, py_coded_image_take_source ... src/process/CodedImageSource.c:28-272,
 *                                                                include/pyframework.h:121-132
 *   DVReconstructionFilter(source)  coded images -> VideoSource   src/process/DVReconstructionFilter.c:31-110
 *   DVSubsampleFilter(source)       VideoSource -> coded images   src/process/DVSubsampleFilter.c:31-110
 *   MPEG2SubsampleFilter(source, size=(720, 480))   VideoSource -> Y'CbCr 4:2:0   src/process/MPEG2SubsampleFilter.c (GL there)
 *   MPEG2ReconstructionFilter(source, size=(720, 480), interlaced=True, matrix="601")   Y'CbCr 4:2:0 -> VideoSource
 *                                   (no reference node: the inverse of the one above, for the 4:2:0 images decoders hand out)
 *
 * A coded image is a handful of byte planes in host memory (it is what a decoder hands over or an encoder
 * takes), so these nodes are where bytes cross PCIe: a reconstruction node uploads three planes
 * (DV: 518 400 bytes) and renders straight into the device frame it was given; a subsample node pulls its
 * source into a device frame, converts there and downloads the three planes.  On the device the planes of
 * either kind live in one pooled block (planes_block below); the reconstruction nodes share one render, the
 * subsample nodes one get_frame (py_planes_render, py_planes_from_source: pyycc422.c's nodes go through them too).
 */
#include "pyext.h"

static PyObject *coded_image_tuple;          /* collections.namedtuple("CodedImage", "data stride line_count") */

CVS_EXPORT bool py_coded_image_take_source(PyObject *source, CodedImageSourceHolder *holder) {
    PyObject *old = holder->source.obj;
    holder->source.obj = NULL;
    holder->source.funcs = NULL;
    Py_XDECREF(old);
    Py_CLEAR(holder->csource);
    if (source == NULL || source == Py_None) return true;
    PyObject *capsule = PyObject_GetAttrString(source, CODED_IMAGE_SOURCE_FUNCS);
    if (!capsule || !PyCapsule_IsValid(capsule, CODED_IMAGE_SOURCE_FUNCS)) {
        Py_XDECREF(capsule);
        PyErr_SetString(PyExc_Exception, "The source didn't have an acceptable " CODED_IMAGE_SOURCE_FUNCS " attribute.");
        return false;
    }
    Py_INCREF(source);
    holder->source.obj = source;
    holder->source.funcs = PyCapsule_GetPointer(capsule, CODED_IMAGE_SOURCE_FUNCS);
    holder->csource = capsule;
    return true;
}

/* ---------------------------------------------------------------- CodedImageSource (base, subclassable in Python) */

static PyObject *cis_get_frame(PyObject *self, PyObject *args) {
    int frame;
    if (!PyArg_ParseTuple(args, "i", &frame)) return NULL;
    CodedImageSourceHolder holder = { { 0 } };
    if (!py_coded_image_take_source(self, &holder)) return NULL;
    coded_image *image = NULL;
    if (holder.source.funcs && holder.source.funcs->getFrame) {
        Py_BEGIN_ALLOW_THREADS
        image = holder.source.funcs->getFrame(holder.source.obj, frame, 0);
        Py_END_ALLOW_THREADS
    }
    py_coded_image_take_source(NULL, &holder);
    if (!image) Py_RETURN_NONE;
    int count = 0;
    while (count < CODED_IMAGE_MAX_PLANES && image->data[count]) count++;
    PyObject *result = count ? PyList_New(count) : NULL;
    for (int i = 0; result && i < count; i++) {
        PyObject *bytes = PyByteArray_FromStringAndSize(image->data[i], (Py_ssize_t)image->stride[i] * image->line_count[i]);
        PyObject *member = bytes ? PyObject_CallFunction(coded_image_tuple, "Oii", bytes, image->stride[i], image->line_count[i]) : NULL;
        Py_XDECREF(bytes);
        if (!member) { Py_CLEAR(result); break; }
        PyList_SET_ITEM(result, i, member);
    }
    if (image->free_func) image->free_func(image);
    if (!result && !PyErr_Occurred()) Py_RETURN_NONE;
    return result;
}

/* vtable entry of the base type: ask the Python object (a subclass that overrides get_frame) */
static coded_image *cis_from_python(PyObject *self, int frame, int quality) {
    PyGILState_STATE g = PyGILState_Ensure();
    coded_image *image = NULL;
    PyObject *own = PyObject_GetAttrString((PyObject *)Py_TYPE(self), "get_frame");
    PyObject *base = PyObject_GetAttrString((PyObject *)&py_type_CodedImageSource, "get_frame");
    const bool overridden = own && base && own != base;
    Py_XDECREF(own); Py_XDECREF(base);
    PyObject *planes = overridden ? PyObject_CallMethod(self, "get_frame", "i", frame) : NULL;
    if (planes && planes != Py_None) {
        Py_ssize_t n = PySequence_Length(planes);
        int strides[CODED_IMAGE_MAX_PLANES] = { 0 }, lines[CODED_IMAGE_MAX_PLANES] = { 0 };
        Py_buffer views[CODED_IMAGE_MAX_PLANES];
        bool have[CODED_IMAGE_MAX_PLANES] = { false }, ok = n >= 0;
        if (n > CODED_IMAGE_MAX_PLANES) n = CODED_IMAGE_MAX_PLANES;
        for (Py_ssize_t p = 0; ok && p < n; p++) {
            PyObject *plane = PySequence_GetItem(planes, p);
            PyObject *data = plane ? PyObject_GetAttrString(plane, "data") : NULL;
            PyObject *stride = plane ? PyObject_GetAttrString(plane, "stride") : NULL;
            PyObject *count = plane ? PyObject_GetAttrString(plane, "line_count") : NULL;
            ok = data && stride && count;
            if (ok && data != Py_None) {
                strides[p] = (int)PyLong_AsLong(stride);
                lines[p] = (int)PyLong_AsLong(count);
                ok = !PyErr_Occurred() && strides[p] >= 0 && lines[p] >= 0 && PyObject_GetBuffer(data, &views[p], PyBUF_SIMPLE) == 0;
                if (ok) {
                    have[p] = true;
                    if (views[p].len != (Py_ssize_t)strides[p] * lines[p]) {
                        fprintf(stderr, "fluggo.media.process.CodedImageSource: plane %zd: expected %zd bytes, got %zd bytes.\n",
                                p, (Py_ssize_t)strides[p] * lines[p], views[p].len);
                        ok = false;
                    }
                }
            }
            Py_XDECREF(data); Py_XDECREF(stride); Py_XDECREF(count); Py_XDECREF(plane);
        }
        if (ok) image = coded_image_alloc(strides, lines, (int)n);
        for (Py_ssize_t p = 0; p < n; p++) {
            if (image && have[p] && image->data[p]) memcpy(image->data[p], views[p].buf, (size_t)views[p].len);
            if (have[p]) PyBuffer_Release(&views[p]);
        }
        if (!ok && image) { image->free_func(image); image = NULL; }
    }
    if (PyErr_Occurred()) PyErr_Print();
    Py_XDECREF(planes);
    PyGILState_Release(g);
    return image;
}

static coded_image_source_funcs cis_funcs = { 0, (coded_image_getFrameFunc)cis_from_python };
static PyObject *cis_capsule, *sub_capsule;
static PyMethodDef cis_methods[] = {
    { "get_frame", cis_get_frame, METH_VARARGS, "[CodedImage(data, stride, line_count), ...] or None = source.get_frame(frame)" },
    { NULL }
};
static PyGetSetDef cis_getset[] = { { CODED_IMAGE_SOURCE_FUNCS, pyext_capsule_getter, NULL, "Coded image source C API.", &cis_capsule }, { NULL } };

CVS_EXPORT PyTypeObject py_type_CodedImageSource = {
    PyVarObject_HEAD_INIT(NULL, 0)
    .tp_name = "fluggo.media.process.CodedImageSource", .tp_basicsize = sizeof(PyObject), .tp_new = PyType_GenericNew,
    .tp_flags = Py_TPFLAGS_DEFAULT | Py_TPFLAGS_BASETYPE, .tp_methods = cis_methods, .tp_getset = cis_getset,
};

/* ---------------------------------------------------------------- coded planes on the device */

static size_t plane_bytes(const coded_image *image, int p) { return (size_t)image->stride[p] * (size_t)image->line_count[p]; }

/* *dev = *host with its three planes in one pooled block, each on a 256-byte boundary; NULL when there is no memory */
static char *planes_block(coded_image *dev, const coded_image *host, cvs_stream_t s) {
    size_t off[3], total = 0;
    for (int p = 0; p < 3; p++) { off[p] = total; total += (plane_bytes(host, p) + 255) & ~(size_t)255; }
    char *block = cvs_pool_malloc(total ? total : 1, s);
    *dev = *host;
    for (int p = 0; p < 3; p++) dev->data[p] = block ? block + off[p] : NULL;
    return block;
}

static int planes_copy(const coded_image *dev, const coded_image *host, bool up, cvs_stream_t s) {
    int rc = 0;
    for (int p = 0; rc == 0 && p < 3; p++)
        if (plane_bytes(host, p))          /* (a one-plane layout has two planes of no bytes) */
            rc = up ? cvs_memcpy_h2d(dev->data[p], host->data[p], plane_bytes(host, p), s) : cvs_memcpy_d2h(host->data[p], dev->data[p], plane_bytes(host, p), s);
    return rc;
}

/* The render of every reconstruction node (native: f16): the planes up, the node's device entry straight into the device slot.
 * `planes`: how many planes the node's layout takes (the first `planes` must be there); `entry(out, dev, node, stream)`: the
 * node's call.  Planes missing give an empty window here, planes too small for the raster at the entry (it refuses them before
 * any read). */
typedef struct { PyObject_HEAD CodedImageSourceHolder source; int width, height, flags; } py_mpeg2recon;

void py_planes_render(CodedImageSourceHolder *source, int planes, py_planes_recon entry, const void *node, int frame_index, rgba_frame_dev *f) {
    box2i_set_empty(&f->current_window);
    if (!source->source.obj || !source->source.funcs || !source->source.funcs->getFrame) return;
    coded_image *image = source->source.funcs->getFrame(source->source.obj, frame_index, 0);
    if (!image) return;
    coded_image dev;
    bool have = true;
    for (int p = 0; p < planes; p++) have = have && image->data[p];
    char *block = have ? planes_block(&dev, image, f->stream) : NULL;
    if (block) {
        rgba_frame_f16 out = { f->data, f->full_window, f->full_window };
        int rc = planes_copy(&dev, image, true, f->stream);
        if (rc == 0) rc = entry(&out, &dev, node, f->stream);
        if (rc == 0) f->current_window = out.current_window;
        /* the host planes may be freed below: the uploads must have left them */
        cvs_stream_sync(f->stream);
        cvs_pool_free(block, f->stream);
    }
    if (image->free_func) image->free_func(image);
}

static int dv_recon_entry(rgba_frame_f16 *out, const coded_image *dev, const void *node, cvs_stream_t s) { return cvs_reconstruct_dv_dev(out, dev, s); }
static int mpeg2_recon_entry(rgba_frame_f16 *out, const coded_image *dev, const void *node, cvs_stream_t s) {
    const py_mpeg2recon *m = node;
    return cvs_reconstruct_mpeg2_dev(out, dev, m->width, m->height, m->flags, s);
}

/* The get_frame of every subsample node: pull `window` into a device frame, subsample there through the node's device entry
 * `entry(dev, in, node, stream)`, download the planes (`count` of them, of these strides and line counts). */
coded_image *py_planes_from_source(video_source *source, int frame, const box2i *window, const int strides[3], const int lines[3], int count,
                                   py_planes_sub entry, const void *node) {
    coded_image *out = coded_image_alloc(strides, lines, count), dev;
    if (!out) return NULL;
    rgba_frame_dev d = { cvs_pool_malloc(frame_bytes(window, CVS_FORMAT_F16), NULL), CVS_FORMAT_F16, *window, *window, NULL };
    char *block = planes_block(&dev, out, NULL);
    int rc = (d.data && block) ? 0 : -1;
    if (rc == 0) {
        video_get_frame_dev(source, frame, &d);
        rgba_frame_f16 in = { d.data, d.full_window, d.current_window };
        rc = entry(&dev, &in, node, NULL);
        if (rc == 0) rc = planes_copy(&dev, out, false, NULL);
    }
    cvs_pool_free(block, NULL);
    cvs_pool_free(d.data, NULL);
    if (rc != 0) { out->free_func(out); return NULL; }
    return out;
}

/* DV: the pulled frame is scratch, no need to leave it encoded */
static int dv_sub_entry(coded_image *dev, const rgba_frame_f16 *in, const void *node, cvs_stream_t s) { return cvs_subsample_dv_dev(dev, (rgba_frame_f16 *)in, 0, s); }
static int mpeg2_sub_entry(coded_image *dev, const rgba_frame_f16 *in, const void *node, cvs_stream_t s) {
    const int *size = node;
    return cvs_subsample_mpeg2_dev(dev, in, size[0], size[1], s);
}

/* DV: 720x480 at y = -1 (DVSubsampleFilter.c:55-56), chroma w/4 x h; MPEG-2: (0,0)-(w-1,h-1), chroma w/2 x h/2. */
static coded_image *planes_from_source(video_source *source, int frame, int w, int h, bool dv) {
    const int cw = dv ? w / 4 : w / 2, ch = dv ? h : h / 2, y0 = dv ? -1 : 0;
    const int strides[3] = { w, cw, cw }, lines[3] = { h, ch, ch }, size[2] = { w, h };
    box2i window;
    box2i_set(&window, 0, y0, w - 1, y0 + h - 1);
    return py_planes_from_source(source, frame, &window, strides, lines, 3, dv ? dv_sub_entry : mpeg2_sub_entry, size);
}

/* ---------------------------------------------------------------- DVReconstructionFilter */

typedef struct { PyObject_HEAD CodedImageSourceHolder source; } py_dvrecon;

static int recon_init(py_dvrecon *self, PyObject *args, PyObject *kw) {
    static char *kwlist[] = { "source", NULL };
    PyObject *src;
    if (!PyArg_ParseTupleAndKeywords(args, kw, "O", kwlist, &src)) return -1;
    return py_coded_image_take_source(src, &self->source) ? 0 : -1;
}
static void recon_dealloc(py_dvrecon *self) {
    py_coded_image_take_source(NULL, &self->source);
    Py_TYPE(self)->tp_free((PyObject *)self);
}

static void recon_render(PyObject *o, int frame_index, rgba_frame_dev *f) { py_planes_render(&((py_dvrecon *)o)->source, 3, dv_recon_entry, NULL, frame_index, f); }
DEFINE_NODE_VTABLE(recon, CVS_FORMAT_F16, 1, 0)
static void *recon_unused[] __attribute__((unused)) = { (void *)recon_slot_32 };
static PyGetSetDef recon_getset[] = { { VIDEO_FRAME_SOURCE_FUNCS, pyext_capsule_getter, NULL, "Video frame source C API.", &recon_capsule }, { NULL } };
static PyTypeObject py_type_DVReconstructionFilter = {
    PyVarObject_HEAD_INIT(NULL, 0)
    .tp_name = "fluggo.media.process.DVReconstructionFilter", .tp_basicsize = sizeof(py_dvrecon), .tp_flags = Py_TPFLAGS_DEFAULT,
    .tp_base = &py_type_VideoSource, .tp_new = PyType_GenericNew, .tp_init = (initproc)recon_init,
    .tp_dealloc = (destructor)recon_dealloc, .tp_getset = recon_getset,
};

/* ---------------------------------------------------------------- DVSubsampleFilter */

typedef struct { PyObject_HEAD video_source *source; } py_dvsub;

static int sub_init(py_dvsub *self, PyObject *args, PyObject *kw) {
    static char *kwlist[] = { "source", NULL };
    PyObject *src;
    if (!PyArg_ParseTupleAndKeywords(args, kw, "O", kwlist, &src)) return -1;
    return py_video_take_source(src, &self->source) ? 0 : -1;
}
static void sub_dealloc(py_dvsub *self) {
    py_video_take_source(NULL, &self->source);
    Py_TYPE(self)->tp_free((PyObject *)self);
}

static coded_image *sub_get_frame(py_dvsub *self, int frame, int quality) { return planes_from_source(self->source, frame, 720, 480, true); }

static coded_image_source_funcs sub_funcs = { 0, (coded_image_getFrameFunc)sub_get_frame };
static PyGetSetDef sub_getset[] = { { CODED_IMAGE_SOURCE_FUNCS, pyext_capsule_getter, NULL, "Coded image source C API.", &sub_capsule }, { NULL } };
static PyTypeObject py_type_DVSubsampleFilter = {
    PyVarObject_HEAD_INIT(NULL, 0)
    .tp_name = "fluggo.media.process.DVSubsampleFilter", .tp_basicsize = sizeof(py_dvsub), .tp_flags = Py_TPFLAGS_DEFAULT,
    .tp_base = &py_type_CodedImageSource, .tp_new = PyType_GenericNew, .tp_init = (initproc)sub_init,
    .tp_dealloc = (destructor)sub_dealloc, .tp_getset = sub_getset,
};

/* ---------------------------------------------------------------- MPEG2SubsampleFilter */

/* src/process/MPEG2SubsampleFilter.c (GL-only in the reference, video_subsample_mpeg2_gl): the same node on the device
 * entry, with the raster as a keyword (the reference's 720x480 by default). */
typedef struct { PyObject_HEAD video_source *source; int width, height; } py_mpeg2sub;

static int mpeg2_init(py_mpeg2sub *self, PyObject *args, PyObject *kw) {
    static char *kwlist[] = { "source", "size", NULL };
    PyObject *src, *size = NULL;
    if (!PyArg_ParseTupleAndKeywords(args, kw, "O|O", kwlist, &src, &size)) return -1;
    v2i sz = { 720, 480 };
    if (size && !py_parse_v2i(size, &sz)) return -1;
    if (sz.x < 2 || (sz.x & 1) || sz.y < 4 || (sz.y & 3)) {
        PyErr_Format(PyExc_ValueError, "MPEG2SubsampleFilter: size (%d, %d): the width must be even and at least 2, the height a multiple of 4", sz.x, sz.y);
        return -1;
    }
    if (!py_video_take_source(src, &self->source)) return -1;
    self->width = sz.x;
    self->height = sz.y;
    return 0;
}
static void mpeg2_dealloc(py_mpeg2sub *self) {
    py_video_take_source(NULL, &self->source);
    Py_TYPE(self)->tp_free((PyObject *)self);
}

static coded_image *mpeg2_get_frame(py_mpeg2sub *self, int frame, int quality) { return planes_from_source(self->source, frame, self->width, self->height, false); }

static coded_image_source_funcs mpeg2_funcs = { 0, (coded_image_getFrameFunc)mpeg2_get_frame };
static PyObject *mpeg2_capsule;
static PyGetSetDef mpeg2_getset[] = { { CODED_IMAGE_SOURCE_FUNCS, pyext_capsule_getter, NULL, "Coded image source C API.", &mpeg2_capsule }, { NULL } };
static PyTypeObject py_type_MPEG2SubsampleFilter = {
    PyVarObject_HEAD_INIT(NULL, 0)
    .tp_name = "fluggo.media.process.MPEG2SubsampleFilter", .tp_basicsize = sizeof(py_mpeg2sub), .tp_flags = Py_TPFLAGS_DEFAULT,
    .tp_base = &py_type_CodedImageSource, .tp_new = PyType_GenericNew, .tp_init = (initproc)mpeg2_init,
    .tp_dealloc = (destructor)mpeg2_dealloc, .tp_getset = mpeg2_getset,
};

/* ---------------------------------------------------------------- MPEG2ReconstructionFilter */

/* coded planes -> half RGBA on the device entry (DESIGN.md "MPEG-2 4:2:0 reconstruction"): the raster, the siting and the matrix
 * as keywords.  Renders like DVReconstructionFilter (py_planes_render above, where py_mpeg2recon is declared). */

static int mpeg2r_init(py_mpeg2recon *self, PyObject *args, PyObject *kw) {
    static char *kwlist[] = { "source", "size", "interlaced", "matrix", NULL };
    PyObject *src, *size = NULL, *matrix = NULL;
    int interlaced = 1;
    if (!PyArg_ParseTupleAndKeywords(args, kw, "O|OpO", kwlist, &src, &size, &interlaced, &matrix)) return -1;
    v2i sz = { 720, 480 };
    if (size && !py_parse_v2i(size, &sz)) return -1;
    if (sz.x < 2 || (sz.x & 1) || sz.y < 2 || (sz.y & 1) || (interlaced && (sz.y < 4 || (sz.y & 3)))) {
        PyErr_Format(PyExc_ValueError, "MPEG2ReconstructionFilter: size (%d, %d): the width must be even and at least 2, the height %s", sz.x, sz.y,
                     interlaced ? "a multiple of 4 (interlaced)" : "even and at least 2");
        return -1;
    }
    int flags = interlaced ? 0 : CVS_YCC_PROGRESSIVE;
    if (matrix) {
        const char *m = PyUnicode_Check(matrix) ? PyUnicode_AsUTF8(matrix) : NULL;
        if (m && !strcmp(m, "709")) flags |= CVS_YCC_REC709;
        else if (!m || strcmp(m, "601")) {
            PyErr_Clear();
            PyErr_Format(PyExc_ValueError, "MPEG2ReconstructionFilter: matrix must be \"601\" or \"709\", not %R", matrix);
            return -1;
        }
    }
    if (!py_coded_image_take_source(src, &self->source)) return -1;
    self->width = sz.x;
    self->height = sz.y;
    self->flags = flags;
    return 0;
}
static void mpeg2r_dealloc(py_mpeg2recon *self) {
    py_coded_image_take_source(NULL, &self->source);
    Py_TYPE(self)->tp_free((PyObject *)self);
}

static void mpeg2r_render(PyObject *o, int frame_index, rgba_frame_dev *f) { py_planes_render(&((py_mpeg2recon *)o)->source, 3, mpeg2_recon_entry, o, frame_index, f); }
DEFINE_NODE_VTABLE(mpeg2r, CVS_FORMAT_F16, 1, 0)
static void *mpeg2r_unused[] __attribute__((unused)) = { (void *)mpeg2r_slot_32 };
static PyGetSetDef mpeg2r_getset[] = { { VIDEO_FRAME_SOURCE_FUNCS, pyext_capsule_getter, NULL, "Video frame source C API.", &mpeg2r_capsule }, { NULL } };
static PyTypeObject py_type_MPEG2ReconstructionFilter = {
    PyVarObject_HEAD_INIT(NULL, 0)
    .tp_name = "fluggo.media.process.MPEG2ReconstructionFilter", .tp_basicsize = sizeof(py_mpeg2recon), .tp_flags = Py_TPFLAGS_DEFAULT,
    .tp_base = &py_type_VideoSource, .tp_new = PyType_GenericNew, .tp_init = (initproc)mpeg2r_init,
    .tp_dealloc = (destructor)mpeg2r_dealloc, .tp_getset = mpeg2r_getset,
};

int init_dv(PyObject *module) {
    PyObject *collections = PyImport_ImportModule("collections");
    if (!collections) return -1;
    coded_image_tuple = PyObject_CallMethod(collections, "namedtuple", "ss", "CodedImage", "data stride line_count");
    Py_DECREF(collections);
    if (!coded_image_tuple) return -1;
    PyObject_SetAttrString(coded_image_tuple, "__module__", PyUnicode_FromString("fluggo.media.process"));
    cis_capsule = PyCapsule_New(&cis_funcs, CODED_IMAGE_SOURCE_FUNCS, NULL);
    sub_capsule = PyCapsule_New(&sub_funcs, CODED_IMAGE_SOURCE_FUNCS, NULL);
    mpeg2_capsule = PyCapsule_New(&mpeg2_funcs, CODED_IMAGE_SOURCE_FUNCS, NULL);
    if (!cis_capsule || !sub_capsule || !mpeg2_capsule || pyext_make_capsule(&recon_capsule, &recon_funcs) < 0 ||
        pyext_make_capsule(&mpeg2r_capsule, &mpeg2r_funcs) < 0)
        return -1;
    Py_INCREF(coded_image_tuple);
    if (PyModule_AddObject(module, "CodedImage", coded_image_tuple) < 0) return -1;
    if (pyext_add_type(module, "CodedImageSource", &py_type_CodedImageSource) < 0) return -1;
    if (pyext_add_type(module, "DVReconstructionFilter", &py_type_DVReconstructionFilter) < 0) return -1;
    if (pyext_add_type(module, "DVSubsampleFilter", &py_type_DVSubsampleFilter) < 0) return -1;
    if (pyext_add_type(module, "MPEG2SubsampleFilter", &py_type_MPEG2SubsampleFilter) < 0) return -1;
    return pyext_add_type(module, "MPEG2ReconstructionFilter", &py_type_MPEG2ReconstructionFilter);
}
