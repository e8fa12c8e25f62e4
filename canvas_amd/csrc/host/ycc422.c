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
    return cvs_ycc_layout_out(layout_of("cvs_ycc422_layout", layout, width, height, s, l, &align), s, l, strides, line_counts);
}

/* what both entries refuse about flags, layout, size and image, before the device is touched; 0 and *view filled, or -1 (error set) */
static int args_check(const char *what, const coded_image *image, int width, int height, int layout, int flags, cvk_ycc_image *view) {
    if (flags & ~CVS_YCC_REC709) {
        cvs_set_error("%s: unknown flags 0x%x (CVS_YCC_REC709 or 0: 4:2:2 has no siting to choose)", what, (unsigned)flags);
        return -1;
    }
    int strides[3], lines[3], align;
    const int planes = layout_of(what, layout, width, height, strides, lines, &align);
    if (!planes) return -1;
    return cvs_ycc_image_check(what, image, planes, strides, lines, align, layout_names[layout], width, height, view);
}

/* Both entries refuse before they touch the device, as the 4:2:0 edges do (ycc420.c): a refusal needs no GPU. */
CVS_EXPORT int cvs_reconstruct_422_dev(rgba_frame_f16 *frame, const coded_image *image, int width, int height, int layout, int flags, cvs_stream_t stream) {
    static const char what[] = "4:2:2 reconstruct";
    if (!frame) { cvs_set_error("%s: need a frame", what); return -1; }
    box2i_set_empty(&frame->current_window);
    if (cvs_coords_refused("cvs_reconstruct_422_dev", "frame", &frame->full_window, NULL, CVS_MAX_COORD)) return -1;
    cvk_ycc_image view;
    if (args_check(what, image, width, height, layout, flags, &view) != 0) return -1;
    if (cvs_enter() != 0) return -1;
    box2i w;
    if (cvs_raster_window(&frame->full_window, width, height, &w)) return 0;
    const half *lut = cvs_ycc_import_lut();
    if (!lut) return -1;
    const int rc = cvk_ycc422_reconstruct(cvs_view(frame->data, &frame->full_window), cvs_rect(&w), &view, width, height, layout, cvs_ycc_to_rgb(flags), lut,
                                          cvs_cus(), cvs_pick_stream(stream));
    if (rc != 0) { cvs_set_error("%s: %s", what, hipGetErrorString((hipError_t)rc)); return rc; }
    frame->current_window = w;
    return 0;
}

CVS_EXPORT int cvs_subsample_422_dev(coded_image *image, const rgba_frame_f16 *frame, int width, int height, int layout, int flags, cvs_stream_t stream) {
    static const char what[] = "4:2:2 subsample";
    if (!frame) { cvs_set_error("%s: need a frame", what); return -1; }
    if (!cvs_box_contains(&frame->full_window, &frame->current_window)) { cvs_set_error("%s: current window outside the buffer", what); return -1; }
    if (cvs_coords_refused("cvs_subsample_422_dev", "frame", &frame->full_window, &frame->current_window, CVS_MAX_COORD)) return -1;
    cvk_ycc_image view;
    if (args_check(what, image, width, height, layout, flags, &view) != 0) return -1;
    if (cvs_enter() != 0) return -1;
    const half *lut = cvs_ycc_export_lut();
    if (!lut) return -1;
    CVS_KERNEL(cvk_ycc422_subsample(&view, cvs_view(frame->data, &frame->full_window), cvs_raster_rect(&frame->current_window, width, height), width, height,
                                    layout, cvs_rgb_to_ycc(flags), lut, cvs_cus(), cvs_pick_stream(stream)));
    return 0;
}

