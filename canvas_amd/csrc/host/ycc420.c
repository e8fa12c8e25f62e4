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

/* Y'CbCr -> R'G'B' of Rec.2020, non-constant luminance (Kr 0.2627, Kb 0.0593); Rec.601 and Rec.709 are mpeg2.c's */
static const float ycc_2020[9] = { 1.0f, 0.0f, 1.4746f, 1.0f, -0.164553f, -0.571353f, 1.0f, 1.8814f, 0.0f };
/* R'G'B' -> Y'CbCr row by row: Rec.601 and Rec.709 as ycc422.c has them, Rec.2020 */
static const float rgb_601[9] = { 0.299f, 0.587f, 0.114f, -0.168736f, -0.331264f, 0.5f, 0.5f, -0.418688f, -0.081312f };
static const float rgb_709[9] = { 0.2126f, 0.7152f, 0.0722f, -0.114572f, -0.385428f, 0.5f, 0.5f, -0.454153f, -0.045847f };
static const float rgb_2020[9] = { 0.2627f, 0.6780f, 0.0593f, -0.139630f, -0.360370f, 0.5f, 0.5f, -0.459786f, -0.040214f };

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
    const int planes = layout_of("cvs_ycc420_layout", layout, width, height, s, l, &align);
    if (!planes) return -1;
    for (int p = 0; p < 3; p++) {
        if (strides) strides[p] = s[p];
        if (line_counts) line_counts[p] = l[p];
    }
    return planes;
}

/* everything an entry asks of the image; 0 and *view filled, or -1 with the error set */
static int image_check(const char *what, const coded_image *image, int layout, int width, int height, cvk_ycc420_image *view) {
    int strides[3], lines[3], align;
    const int planes = layout_of(what, layout, width, height, strides, lines, &align);
    if (!planes) return -1;
    if (!image) { cvs_set_error("%s: need an image", what); return -1; }
    memset(view, 0, sizeof *view);
    for (int p = 0; p < planes; p++) {
        if (!image->data[p]) { cvs_set_error("%s: %s takes %d planes, plane %d is missing", what, layout_names[layout], planes, p); return -1; }
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
    if (flags & ~KNOWN_FLAGS) {
        cvs_set_error("%s: unknown flags 0x%x (these edges are progressive: CVS_YCC_PROGRESSIVE is not taken)", what, (unsigned)flags);
        return true;
    }
    if ((flags & CVS_YCC_REC709) && (flags & CVS_YCC_REC2020)) { cvs_set_error("%s: flags 0x%x name two matrices, Rec.709 and Rec.2020", what, (unsigned)flags); return true; }
    if ((flags & CVS_YCC_SITING_CENTER) && (flags & CVS_YCC_SITING_TOPLEFT)) {
        cvs_set_error("%s: flags 0x%x name two sitings, centre and top-left", what, (unsigned)flags);
        return true;
    }
    return false;
}

static int siting_of(int flags) { return (flags & CVS_YCC_SITING_CENTER) ? CVK_420_CENTER : ((flags & CVS_YCC_SITING_TOPLEFT) ? CVK_420_TOPLEFT : CVK_420_LEFT); }

CVS_EXPORT int cvs_reconstruct_420_dev(rgba_frame_f16 *frame, const coded_image *image, int width, int height, int layout, int flags, cvs_stream_t stream) {
    static const char what[] = "4:2:0 reconstruct";
    if (!frame) { cvs_set_error("%s: need a frame", what); return -1; }
    box2i_set_empty(&frame->current_window);
    /* every refusal comes before the device is touched */
    if (cvs_coords_refused("cvs_reconstruct_420_dev", "frame", &frame->full_window, NULL, CVS_MAX_COORD)) return -1;
    if (flags_refused(what, flags)) return -1;
    cvk_ycc420_image view;
    if (image_check(what, image, layout, width, height, &view) != 0) return -1;
    if (cvs_enter() != 0) return -1;
    box2i w;
    box2i_set(&w, max(0, frame->full_window.min.x), max(0, frame->full_window.min.y), min(width - 1, frame->full_window.max.x),
              min(height - 1, frame->full_window.max.y));
    if (box2i_is_empty(&frame->full_window) || box2i_is_empty(&w)) return 0;
    /* the separate flavour's table in both flavours, as at the MPEG-2 edge: the pixels must not depend on the flavour */
    const half *lut = NULL;
    if (!(flags & CVS_YCC_NO_TRANSFER) && !(lut = cvs_lut_device_separate(CVS_LUT_REC709_TO_LINEAR_SCENE))) return -1;
    const bool ten = layout == CVS_420_PLANAR10 || layout == CVS_420_P010, full = (flags & CVS_YCC_FULL_RANGE) != 0;
    const float s = ten ? 4.0f : 1.0f, top = ten ? 1023.0f : 255.0f;
    const int siting = siting_of(flags);
    cvk_ycc420_decode d;
    memcpy(d.mat, (flags & CVS_YCC_REC2020) ? ycc_2020 : ((flags & CVS_YCC_REC709) ? cvs_ycc_709 : cvs_ycc_601), sizeof d.mat);
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
    if (flags_refused(what, flags)) return -1;
    cvk_ycc420_image view;
    if (image_check(what, image, layout, width, height, &view) != 0) return -1;
    if (cvs_enter() != 0) return -1;
    /* pixels outside the current window (and outside the raster) count as black: the kernel reads inside w only */
    box2i w;
    box2i_set(&w, max(0, frame->current_window.min.x), max(0, frame->current_window.min.y), min(width - 1, frame->current_window.max.x),
              min(height - 1, frame->current_window.max.y));
    const cvk_rect none = { 0, 0, -1, -1 };
    const cvk_rect r = box2i_is_empty(&frame->current_window) || box2i_is_empty(&w) ? none : cvs_rect(&w);
    /* the separate flavour's table in both flavours (mpeg2.c: the contracted build of linear -> Rec.709 differs at one code) */
    const half *lut = NULL;
    if (!(flags & CVS_YCC_NO_TRANSFER) && !(lut = cvs_lut_device_separate(CVS_LUT_LINEAR_TO_REC709))) return -1;
    const bool ten = layout == CVS_420_PLANAR10 || layout == CVS_420_P010, full = (flags & CVS_YCC_FULL_RANGE) != 0;
    const float s = ten ? 4.0f : 1.0f, top = ten ? 1023.0f : 255.0f;
    cvk_ycc420_encode e;
    memcpy(e.mat, (flags & CVS_YCC_REC2020) ? rgb_2020 : ((flags & CVS_YCC_REC709) ? rgb_709 : rgb_601), sizeof e.mat);
    e.y_scale = full ? 1.0f : (219.0f * s) / top;
    e.y_offset = full ? 0.0f : (16.0f * s) / top;
    e.c_scale = full ? 1.0f : (224.0f * s) / top;
    e.c_offset = (128.0f * s) / top;
    e.top = top;
    /* 0-3 and 1020-1023 are reserved on SDI; full range knows no reserved codes */
    e.lo = ten && !full ? 4u : 0u;
    e.hi = ten ? (full ? 1023u : 1019u) : 255u;
    e.siting = siting_of(flags);
    CVS_KERNEL(cvk_ycc420_subsample(&view, cvs_view(frame->data, &frame->full_window), r, width, height, layout, &e, lut, cvs_cus(), cvs_pick_stream(stream)));
    return 0;
}
