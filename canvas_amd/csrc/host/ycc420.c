/*
 * ycc420.c -- the 4:2:0 Y'CbCr edges (include/canvas_ycc420.h): planar 8/10-bit, NV12 and P010 <-> half RGBA frame, progressive.
 *
 * No reference code: its decoder hands 4:2:0 images out (src/libav/AVVideoDecoder.c:75-97) and its one 4:2:0 filter is the
 * interlaced Rec.601 MPEG-2 subsample (mpeg2.c).  The shape is the 4:2:2 edges' (ycc422.c) with a height rule and more flags; what
 * the kernels compute, rounding included, is DESIGN.md "4:2:0 Y'CbCr edges" and kernels/ycc420_recon_ops.hip,
 * kernels/ycc420_ops.hip.  Range, matrix and siting reach the kernels as constants and weights.  Device entries only.
 */
#include "internal.h"
#include "canvas_ycc420.h"

static const char *const layout_names[4] = { "planar 8-bit", "planar 10-bit", "NV12", "P010" };
enum { KNOWN_FLAGS = CVS_YCC_REC709 | CVS_YCC_REC2020 | CVS_YCC_FULL_RANGE | CVS_YCC_SITING_CENTER | CVS_YCC_SITING_TOPLEFT | CVS_YCC_NO_TRANSFER };

/* planes, least strides, line counts and the alignment of bases and strides; 0 where the size or the layout is refused (error set) */
static int layout_of(const char *what, int layout, int width, int height, int strides[3], int lines[3], int *align) {
    if (layout < CVS_420_PLANAR8 || layout > CVS_420_P010) { cvs_set_error("%s: unknown layout %d", what, layout); return 0; }
    /* (the bound keeps every stride, and 2 * width, inside an int) */
    if (width < 2 || (width & 1) || height < 2 || (height & 1) || width > (1 << 29)) {
        cvs_set_error("%s: %dx%d: the width and the height must be even and at least 2", what, width, height);
        return 0;
    }
    const int bytes = layout == CVS_420_PLANAR10 || layout == CVS_420_P010 ? 2 : 1;
    const int planes = layout == CVS_420_PLANAR8 || layout == CVS_420_PLANAR10 ? 3 : 2;
    *align = bytes;
    strides[0] = bytes * width;
    strides[1] = planes == 3 ? bytes * (width / 2) : bytes * width;
    strides[2] = planes == 3 ? bytes * (width / 2) : 0;
    lines[0] = height;
    lines[1] = height / 2;
    lines[2] = planes == 3 ? height / 2 : 0;
    return planes;
}

CVS_EXPORT int cvs_ycc420_layout(int layout, int width, int height, int strides[3], int line_counts[3]) {
    int s[3], l[3], align;
    return cvs_ycc_layout_out(layout_of("cvs_ycc420_layout", layout, width, height, s, l, &align), s, l, strides, line_counts);
}

/* what both entries refuse about flags, layout, size and image, before the device is touched; 0 and *view filled, or -1 (error set) */
static int args_check(const char *what, const coded_image *image, int width, int height, int layout, int flags, cvk_ycc_image *view) {
    if (flags & ~KNOWN_FLAGS) {
        cvs_set_error("%s: unknown flags 0x%x (these edges are progressive: CVS_YCC_PROGRESSIVE is not taken)", what, (unsigned)flags);
        return -1;
    }
    if ((flags & CVS_YCC_REC709) && (flags & CVS_YCC_REC2020)) { cvs_set_error("%s: flags 0x%x name two matrices, Rec.709 and Rec.2020", what, (unsigned)flags); return -1; }
    if ((flags & CVS_YCC_SITING_CENTER) && (flags & CVS_YCC_SITING_TOPLEFT)) {
        cvs_set_error("%s: flags 0x%x name two sitings, centre and top-left", what, (unsigned)flags);
        return -1;
    }
    int strides[3], lines[3], align;
    const int planes = layout_of(what, layout, width, height, strides, lines, &align);
    if (!planes) return -1;
    return cvs_ycc_image_check(what, image, planes, strides, lines, align, layout_names[layout], width, height, view);
}

static int siting_of(int flags) { return (flags & CVS_YCC_SITING_CENTER) ? CVK_420_CENTER : ((flags & CVS_YCC_SITING_TOPLEFT) ? CVK_420_TOPLEFT : CVK_420_LEFT); }

CVS_EXPORT int cvs_reconstruct_420_dev(rgba_frame_f16 *frame, const coded_image *image, int width, int height, int layout, int flags, cvs_stream_t stream) {
    static const char what[] = "4:2:0 reconstruct";
    if (!frame) { cvs_set_error("%s: need a frame", what); return -1; }
    box2i_set_empty(&frame->current_window);
    /* every refusal comes before the device is touched */
    if (cvs_coords_refused("cvs_reconstruct_420_dev", "frame", &frame->full_window, NULL, CVS_MAX_COORD)) return -1;
    cvk_ycc_image view;
    if (args_check(what, image, width, height, layout, flags, &view) != 0) return -1;
    if (cvs_enter() != 0) return -1;
    box2i w;
    if (cvs_raster_window(&frame->full_window, width, height, &w)) return 0;
    const half *lut = NULL;
    if (!(flags & CVS_YCC_NO_TRANSFER) && !(lut = cvs_ycc_import_lut())) return -1;
    const bool ten = layout == CVS_420_PLANAR10 || layout == CVS_420_P010, full = (flags & CVS_YCC_FULL_RANGE) != 0;
    const float s = ten ? 4.0f : 1.0f, top = ten ? 1023.0f : 255.0f;
    const int siting = siting_of(flags);
    cvk_ycc420_decode d;
    memcpy(d.mat, cvs_ycc_to_rgb(flags), sizeof d.mat);
    d.y_off = full ? 0.0f : 16.0f * s;
    d.y_div = full ? top : 219.0f * s;
    d.c_off = 128.0f * s;
    d.c_div = full ? top : 224.0f * s;
    /* near and far weight of every step (kernels.h): 1, 0 is the near value itself; 0.5, 0.5 the mean */
    d.ve[0] = siting == CVK_420_TOPLEFT ? 1.0f : 0.75f;  d.ve[1] = siting == CVK_420_TOPLEFT ? 0.0f : 0.25f;
    d.vo[0] = siting == CVK_420_TOPLEFT ? 0.5f : 0.75f;  d.vo[1] = siting == CVK_420_TOPLEFT ? 0.5f : 0.25f;
    d.he[0] = siting == CVK_420_CENTER ? 0.75f : 1.0f;   d.he[1] = siting == CVK_420_CENTER ? 0.25f : 0.0f;
    d.ho[0] = siting == CVK_420_CENTER ? 0.75f : 0.5f;   d.ho[1] = siting == CVK_420_CENTER ? 0.25f : 0.5f;
    d.left_column = siting == CVK_420_CENTER;
    const int rc = cvk_ycc420_reconstruct(cvs_view(frame->data, &frame->full_window), cvs_rect(&w), &view, width, height, layout, &d, lut, cvs_cus(),
                                          cvs_pick_stream(stream));
    if (rc != 0) { cvs_set_error("%s: %s", what, hipGetErrorString((hipError_t)rc)); return rc; }
    frame->current_window = w;
    return 0;
}

CVS_EXPORT int cvs_subsample_420_dev(coded_image *image, const rgba_frame_f16 *frame, int width, int height, int layout, int flags, cvs_stream_t stream) {
    static const char what[] = "4:2:0 subsample";
    /* every refusal comes before the device is touched */
    if (!frame) { cvs_set_error("%s: need a frame", what); return -1; }
    if (!cvs_box_contains(&frame->full_window, &frame->current_window)) { cvs_set_error("%s: current window outside the buffer", what); return -1; }
    if (cvs_coords_refused("cvs_subsample_420_dev", "frame", &frame->full_window, &frame->current_window, CVS_MAX_COORD)) return -1;
    cvk_ycc_image view;
    if (args_check(what, image, width, height, layout, flags, &view) != 0) return -1;
    if (cvs_enter() != 0) return -1;
    const half *lut = NULL;
    if (!(flags & CVS_YCC_NO_TRANSFER) && !(lut = cvs_ycc_export_lut())) return -1;
    const bool ten = layout == CVS_420_PLANAR10 || layout == CVS_420_P010, full = (flags & CVS_YCC_FULL_RANGE) != 0;
    const float s = ten ? 4.0f : 1.0f, top = ten ? 1023.0f : 255.0f;
    cvk_ycc420_encode e;
    memcpy(e.mat, cvs_rgb_to_ycc(flags), sizeof e.mat);
    e.y_scale = full ? 1.0f : (219.0f * s) / top;
    e.y_offset = full ? 0.0f : (16.0f * s) / top;
    e.c_scale = full ? 1.0f : (224.0f * s) / top;
    e.c_offset = (128.0f * s) / top;
    e.top = top;
    /* 0-3 and 1020-1023 are reserved on SDI; full range knows no reserved codes */
    e.lo = ten && !full ? 4u : 0u;
    e.hi = ten ? (full ? 1023u : 1019u) : 255u;
    e.siting = siting_of(flags);
    CVS_KERNEL(cvk_ycc420_subsample(&view, cvs_view(frame->data, &frame->full_window), cvs_raster_rect(&frame->current_window, width, height), width, height,
                                    layout, &e, lut, cvs_cus(), cvs_pick_stream(stream)));
    return 0;
}

