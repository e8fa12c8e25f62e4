/*
 * ycc_common.c -- what the Y'CbCr edges share on the host (mpeg2.c, ycc422.c, ycc420.c): the matrices, the checks on a coded image
 * against a layout's planes, the window an entry works on, and the half table both arithmetic flavours use.  What is particular to
 * an edge -- its layouts, flags, constants and weights -- stays in its file.
 */
#include "internal.h"
#include "canvas_ycc420.h"

/* Y'CbCr -> R'G'B' row by row, as video_reconstruct.c:55-59 (Rec.601, Poynton p. 305) and :62-66 (Rec.709, p. 316) state them;
 * Rec.2020 non-constant luminance (Kr 0.2627, Kb 0.0593) */
static const float ycc_601[9] = { 1.0f, 0.0f, 1.402f, 1.0f, -0.344136f, -0.714136f, 1.0f, 1.772f, 0.0f };
static const float ycc_709[9] = { 1.0f, 0.0f, 1.5748f, 1.0f, -0.187324f, -0.468124f, 1.0f, 1.8556f, 0.0f };
static const float ycc_2020[9] = { 1.0f, 0.0f, 1.4746f, 1.0f, -0.164553f, -0.571353f, 1.0f, 1.8814f, 0.0f };
/* R'G'B' -> Y'CbCr row by row: Rec.601 as kernels/mpeg2_ops.hip has it (video_subsample.c:189-526), Rec.709 (Poynton p. 316), Rec.2020 */
static const float rgb_601[9] = { 0.299f, 0.587f, 0.114f, -0.168736f, -0.331264f, 0.5f, 0.5f, -0.418688f, -0.081312f };
static const float rgb_709[9] = { 0.2126f, 0.7152f, 0.0722f, -0.114572f, -0.385428f, 0.5f, 0.5f, -0.454153f, -0.045847f };
static const float rgb_2020[9] = { 0.2627f, 0.6780f, 0.0593f, -0.139630f, -0.360370f, 0.5f, 0.5f, -0.459786f, -0.040214f };

const float *cvs_ycc_to_rgb(int flags) { return (flags & CVS_YCC_REC2020) ? ycc_2020 : ((flags & CVS_YCC_REC709) ? ycc_709 : ycc_601); }
const float *cvs_rgb_to_ycc(int flags) { return (flags & CVS_YCC_REC2020) ? rgb_2020 : ((flags & CVS_YCC_REC709) ? rgb_709 : rgb_601); }

int cvs_ycc_layout_out(int planes, const int s[3], const int l[3], int strides[3], int line_counts[3]) {
    if (!planes) return -1;
    for (int p = 0; p < 3; p++) {
        if (strides) strides[p] = s[p];
        if (line_counts) line_counts[p] = l[p];
    }
    return planes;
}

int cvs_ycc_image_check(const char *what, const coded_image *image, int planes, const int strides[3], const int lines[3], int align, const char *layout_name,
                        int width, int height, cvk_ycc_image *view) {
    if (!image) { cvs_set_error("%s: need an image", what); return -1; }
    memset(view, 0, sizeof *view);
    for (int p = 0; p < planes; p++) {
        if (!image->data[p]) { cvs_set_error("%s: %s takes %d plane%s, plane %d is missing", what, layout_name, planes, planes > 1 ? "s" : "", p); return -1; }
        if (image->stride[p] < strides[p] || image->line_count[p] < lines[p]) {
            cvs_set_error("%s: plane %d of %s %dx%d is too short: need %d lines of %d bytes, got %d of %d", what, p, layout_name, width, height,
                          lines[p], strides[p], image->line_count[p], image->stride[p]);
            return -1;
        }
        if (((uintptr_t)image->data[p] | (uintptr_t)(unsigned)image->stride[p]) & (uintptr_t)(align - 1)) {
            cvs_set_error("%s: plane %d of %s is misaligned: base %p and stride %d must be multiples of %d", what, p, layout_name,
                          image->data[p], image->stride[p], align);
            return -1;
        }
        view->p[p] = image->data[p];
        view->stride[p] = image->stride[p];
    }
    return 0;
}

bool cvs_raster_window(const box2i *window, int width, int height, box2i *w) {
    box2i_set(w, max(0, window->min.x), max(0, window->min.y), min(width - 1, window->max.x), min(height - 1, window->max.y));
    return box2i_is_empty(window) || box2i_is_empty(w);
}

cvk_rect cvs_raster_rect(const box2i *window, int width, int height) {
    const cvk_rect none = { 0, 0, -1, -1 };
    box2i w;
    return cvs_raster_window(window, width, height, &w) ? none : cvs_rect(&w);
}

const half *cvs_ycc_export_lut(void) { return cvs_lut_device_separate(CVS_LUT_LINEAR_TO_REC709); }
const half *cvs_ycc_import_lut(void) { return cvs_lut_device_separate(CVS_LUT_REC709_TO_LINEAR_SCENE); }
