/*
 * ycc422.c -- the 4:2:2 Y'CbCr edges (include/canvas_ycc422.h): planar 8/10-bit, UYVY and v210 <-> half RGBA frame.
 *
 * No reference code: its decoder hands 4:2:2 images out untouched (src/libav/AVVideoDecoder.c:72-91 leaves chroma_height at the
 * full height for everything that is not 4:2:0 or 4:1:0) and neither of its reconstruction filters reads them.  The shape is the
 * MPEG-2 edges' (mpeg2.c) without the vertical part; what the kernels compute, rounding included, is DESIGN.md "4:2:2 Y'CbCr
 * edges" and kernels/ycc422_recon_ops.hip, kernels/ycc422_ops.hip.  Device entries only: the reference names no video_* twin.
 */
#include "internal.h"
#include "canvas_ycc422.h"

/* R'G'B' -> Y'CbCr row by row: Rec.601 as kernels/mpeg2_ops.hip has it (video_subsample.c:189-526), Rec.709 (Poynton p. 316) */
static const float rgb_601[9] = { 0.299f, 0.587f, 0.114f, -0.168736f, -0.331264f, 0.5f, 0.5f, -0.418688f, -0.081312f };
static const float rgb_709[9] = { 0.2126f, 0.7152f, 0.0722f, -0.114572f, -0.385428f, 0.5f, 0.5f, -0.454153f, -0.045847f };

static const char *const layout_names[4] = { "planar 8-bit", "planar 10-bit", "UYVY", "v210" };

/* planes, least strides and the alignment of bases and strides; 0 where the size or the layout is refused (error set) */
static int layout_of(const char *what, int layout, int width, int height, int strides[3], int lines[3], int *align) {
    if (layout < CVS_422_PLANAR8 || layout > CVS_422_V210) { cvs_set_error("%s: unknown layout %d", what, layout); return 0; }
    /* (the bound keeps every stride, and 2 * width, inside an int) */
    if (width < 2 || (width & 1) || height < 1 || width > (1 << 29)) {
        cvs_set_error("%s: %dx%d: the width must be even and at least 2, the height at least 1", what, width, height);
        return 0;
    }
    const int planes = layout == CVS_422_PLANAR8 || layout == CVS_422_PLANAR10 ? 3 : 1;
    strides[0] = strides[1] = strides[2] = 0;
    switch (layout) {
    case CVS_422_PLANAR8: strides[0] = width; strides[1] = strides[2] = width / 2; *align = 1; break;
    case CVS_422_PLANAR10: strides[0] = 2 * width; strides[1] = strides[2] = width; *align = 2; break;
    case CVS_422_UYVY: strides[0] = 2 * width; *align = 1; break;
    default: strides[0] = 16 * ((width + 5) / 6); *align = 4; break;
    }
    for (int p = 0; p < 3; p++) lines[p] = p < planes ? height : 0;
    return planes;
}

CVS_EXPORT int cvs_ycc422_layout(int layout, int width, int height, int strides[3], int line_counts[3]) {
    int s[3], l[3], align;
    const int planes = layout_of("cvs_ycc422_layout", layout, width, height, s, l, &align);
    if (!planes) return -1;
    for (int p = 0; p < 3; p++) {
        if (strides) strides[p] = s[p];
        if (line_counts) line_counts[p] = l[p];
    }
    return planes;
}

/* everything an entry asks of the image; 0 and *view filled, or -1 with the error set */
static int image_check(const char *what, const coded_image *image, int layout, int width, int height, cvk_ycc422_image *view) {
    int strides[3], lines[3], align;
    const int planes = layout_of(what, layout, width, height, strides, lines, &align);
    if (!planes) return -1;
    if (!image) { cvs_set_error("%s: need an image", what); return -1; }
    memset(view, 0, sizeof *view);
    for (int p = 0; p < planes; p++) {
        if (!image->data[p]) { cvs_set_error("%s: %s takes %d plane%s, plane %d is missing", what, layout_names[layout], planes, planes > 1 ? "s" : "", p); return -1; }
        if (image->stride[p] < strides[p] || image->line_count[p] < lines[p]) {
            cvs_set_error("%s: plane %d of %s %dx%d is too short: need %d lines of %d bytes, got %d of %d", what, p, layout_names[layout], width, height,
                          lines[p], strides[p], image->line_count[p], image->stride[p]);
            return -1;
        }
        if (((uintptr_t)image->data[p] | (uintptr_t)(unsigned)image->stride[p]) & (uintptr_t)(align - 1)) {
            cvs_set_error("%s: plane %d of %s is misaligned: base %p and stride %d must be multiples of %d", what, p, layout_names[layout],
                          image->data[p], image->stride[p], align);
            return -1;
        }
        view->p[p] = image->data[p];
        view->stride[p] = image->stride[p];
    }
    return 0;
}

static bool flags_refused(const char *what, int flags) {
    if (!(flags & ~CVS_YCC_REC709)) return false;
    cvs_set_error("%s: unknown flags 0x%x (CVS_YCC_REC709 or 0: 4:2:2 has no siting to choose)", what, (unsigned)flags);
    return true;
}

CVS_EXPORT int cvs_reconstruct_422_dev(rgba_frame_f16 *frame, const coded_image *image, int width, int height, int layout, int flags, cvs_stream_t stream) {
    static const char what[] = "4:2:2 reconstruct";
    if (!frame) { cvs_set_error("%s: need a frame", what); return -1; }
    box2i_set_empty(&frame->current_window);
    if (cvs_enter() != 0) return -1;
    if (cvs_coords_refused("cvs_reconstruct_422_dev", "frame", &frame->full_window, NULL, CVS_MAX_COORD)) return -1;
    if (flags_refused(what, flags)) return -1;
    cvk_ycc422_image view;
    if (image_check(what, image, layout, width, height, &view) != 0) return -1;
    box2i w;
    box2i_set(&w, max(0, frame->full_window.min.x), max(0, frame->full_window.min.y), min(width - 1, frame->full_window.max.x),
              min(height - 1, frame->full_window.max.y));
    if (box2i_is_empty(&frame->full_window) || box2i_is_empty(&w)) return 0;
    /* the separate flavour's table in both flavours, as at the MPEG-2 edge: the pixels must not depend on the flavour */
    const half *lut = cvs_lut_device_separate(CVS_LUT_REC709_TO_LINEAR_SCENE);
    if (!lut) return -1;
    const int rc = cvk_ycc422_reconstruct(cvs_view(frame->data, &frame->full_window), cvs_rect(&w), &view, width, height, layout,
                                          (flags & CVS_YCC_REC709) ? cvs_ycc_709 : cvs_ycc_601, lut, cvs_cus(), cvs_pick_stream(stream));
    if (rc != 0) { cvs_set_error("%s: %s", what, hipGetErrorString((hipError_t)rc)); return rc; }
    frame->current_window = w;
    return 0;
}

CVS_EXPORT int cvs_subsample_422_dev(coded_image *image, const rgba_frame_f16 *frame, int width, int height, int layout, int flags, cvs_stream_t stream) {
    static const char what[] = "4:2:2 subsample";
    if (cvs_enter() != 0) return -1;
    if (!frame) { cvs_set_error("%s: need a frame", what); return -1; }
    if (!cvs_box_contains(&frame->full_window, &frame->current_window)) { cvs_set_error("%s: current window outside the buffer", what); return -1; }
    if (cvs_coords_refused("cvs_subsample_422_dev", "frame", &frame->full_window, &frame->current_window, CVS_MAX_COORD)) return -1;
    if (flags_refused(what, flags)) return -1;
    cvk_ycc422_image view;
    if (image_check(what, image, layout, width, height, &view) != 0) return -1;
    /* pixels outside the current window (and outside the raster) count as black: the kernel reads inside w only */
    box2i w;
    box2i_set(&w, max(0, frame->current_window.min.x), max(0, frame->current_window.min.y), min(width - 1, frame->current_window.max.x),
              min(height - 1, frame->current_window.max.y));
    const cvk_rect none = { 0, 0, -1, -1 };
    const cvk_rect r = box2i_is_empty(&frame->current_window) || box2i_is_empty(&w) ? none : cvs_rect(&w);
    /* the separate flavour's table in both flavours (mpeg2.c: the contracted build of linear -> Rec.709 differs at one code) */
    const half *lut = cvs_lut_device_separate(CVS_LUT_LINEAR_TO_REC709);
    if (!lut) return -1;
    CVS_KERNEL(cvk_ycc422_subsample(&view, cvs_view(frame->data, &frame->full_window), r, width, height, layout,
                                    (flags & CVS_YCC_REC709) ? rgb_709 : rgb_601, lut, cvs_cus(), cvs_pick_stream(stream)));
    return 0;
}
