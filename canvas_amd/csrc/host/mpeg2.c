/*
 * mpeg2.c -- MPEG-2 4:2:0 edges of the path: half RGBA frame <-> planar 8-bit Y'CbCr.
 *
 *   video_subsample_mpeg2 ..... src/cprocess/video_subsample.c:189-526 (video_subsample_mpeg2_gl: GLSL only there)
 *   video_reconstruct_mpeg2 ... no reference code (src/cprocess/video_reconstruct.c knows DV only); the inverse edge, for the
 *                               4:2:0 images the reference's decoder hands out (src/libav/AVVideoDecoder.c:75-97)
 * The reference fixes the raster at 720x480 with its origin at frame coordinate (0, 0); the device entry takes any
 * width x height with width even and height a multiple of 4 (both fields of every chroma row pair inside the raster).
 * What the kernel computes, rounding included, is stated in DESIGN.md "MPEG-2 4:2:0 subsample" and in
 * kernels/mpeg2_ops.hip.  The caller's frame is only read.  The reference-named entries take the frame and the planes (one
 * pooled block) through the bridge (bridge.c).
 * The reconstruction takes interlaced or progressive siting and the Rec.601 or Rec.709 matrix (DESIGN.md "MPEG-2 4:2:0
 * reconstruction", kernels/mpeg2_recon_ops.hip); it writes the frame's pixels inside the raster and nothing else.
 */
#include "internal.h"

enum { MPEG2_W = 720, MPEG2_H = 480 };

static bool mpeg2_size_ok(int width, int height) { return width >= 2 && !(width & 1) && height >= 4 && !(height & 3); }

CVS_EXPORT int cvs_subsample_mpeg2_dev(coded_image *planar, const rgba_frame_f16 *frame, int width, int height, cvs_stream_t stream) {
    if (cvs_enter() != 0) return -1;
    if (!mpeg2_size_ok(width, height)) { cvs_set_error("MPEG-2 subsample: %dx%d: the width must be even and the height a multiple of 4", width, height); return -1; }
    const int planes = cvs_planes_check(planar, width, height, width / 2, height / 2);
    if (!frame || planes == CVS_PLANES_MISSING) { cvs_set_error("MPEG-2 subsample: need a frame and three planes"); return -1; }
    if (planes != CVS_PLANES_OK) {
        cvs_set_error("MPEG-2 subsample: need planes of %dx%d, %dx%d, %dx%d", width, height, width / 2, height / 2, width / 2, height / 2);
        return -1;
    }
    if (!cvs_box_contains(&frame->full_window, &frame->current_window)) { cvs_set_error("MPEG-2 subsample: current window outside the buffer"); return -1; }
    if (cvs_coords_refused("cvs_subsample_mpeg2_dev", "frame", &frame->full_window, &frame->current_window, CVS_MAX_COORD)) return -1;
    const half *lut = cvs_ycc_export_lut();
    if (!lut) return -1;
    cvk_dv_planes pl = cvs_planes_view(planar);
    CVS_KERNEL(cvk_mpeg2_subsample(&pl, cvs_view(frame->data, &frame->full_window), cvs_raster_rect(&frame->current_window, width, height), width, height, lut,
                                   cvs_cus(), cvs_pick_stream(stream)));
    return 0;
}

/* ---- reference-named entry point on host memory: 720x480, planes allocated like video_subsample_dv's ---- */

CVS_EXPORT coded_image *video_subsample_mpeg2(rgba_frame_f16 *frame) {
    const int strides[3] = { MPEG2_W, MPEG2_W / 2, MPEG2_W / 2 }, lines[3] = { MPEG2_H, MPEG2_H / 2, MPEG2_H / 2 };
    cvs_bridge br;
    rgba_frame_f16 dframe;
    coded_image dev;
    if (cvs_bridge_open(&br) != 0 || !frame) return NULL;
    if (!cvs_box_contains(&frame->full_window, &frame->current_window)) { cvs_set_error("MPEG-2 subsample: current window outside the buffer"); return NULL; }
    if (cvs_coords_refused("video_subsample_mpeg2", "frame", &frame->full_window, &frame->current_window, CVS_MAX_COORD)) return NULL;
    coded_image *out = coded_image_alloc(strides, lines, 3);
    if (!out) return NULL;
    /* a frame without pixels is not read: one byte stands in for its buffer */
    const bool have_pixels = !box2i_is_empty(&frame->current_window);
    dframe = *frame;
    dframe.data = cvs_bridge_frame(&br, frame->data, have_pixels ? cvs_frame_bytes(&frame->full_window, sizeof(rgba_f16)) : 1, have_pixels ? CVS_BRIDGE_UPLOAD : 0);
    cvs_bridge_planes(&br, &dev, out, lines, false);
    CVS_BRIDGE_CALL(&br, cvs_subsample_mpeg2_dev, &dev, &dframe, MPEG2_W, MPEG2_H);
    cvs_bridge_planes_back(&br, out, &dev);
    if (cvs_bridge_close(&br, NULL) != 0) { out->free_func(out); return NULL; }
    return out;
}

/* ---- the import edge: planar Y'CbCr 4:2:0 -> half RGBA ---- */

static bool recon_size_ok(int width, int height, bool progressive) {
    return width >= 2 && !(width & 1) && height >= 2 && !(height & 1) && (progressive || (height >= 4 && !(height & 3)));
}

CVS_EXPORT int cvs_reconstruct_mpeg2_dev(rgba_frame_f16 *frame, const coded_image *planar, int width, int height, int flags, cvs_stream_t stream) {
    if (!frame) { cvs_set_error("MPEG-2 reconstruct: need a frame"); return -1; }
    box2i_set_empty(&frame->current_window);
    if (cvs_enter() != 0) return -1;
    if (cvs_coords_refused("cvs_reconstruct_mpeg2_dev", "frame", &frame->full_window, NULL, CVS_MAX_COORD)) return -1;
    const bool progressive = (flags & CVS_YCC_PROGRESSIVE) != 0;
    if (flags & ~(CVS_YCC_PROGRESSIVE | CVS_YCC_REC709)) { cvs_set_error("MPEG-2 reconstruct: unknown flags 0x%x", (unsigned)flags); return -1; }
    if (!recon_size_ok(width, height, progressive)) {
        cvs_set_error("MPEG-2 reconstruct: %dx%d: the width must be even and at least 2, the height %s", width, height,
                      progressive ? "even and at least 2" : "a multiple of 4 and at least 4");
        return -1;
    }
    const int planes = cvs_planes_check(planar, width, height, width / 2, height / 2);
    if (planes == CVS_PLANES_MISSING) { cvs_set_error("MPEG-2 reconstruct: need three planes"); return -1; }
    if (planes != CVS_PLANES_OK) {
        cvs_set_error("MPEG-2 reconstruct: need planes of %dx%d, %dx%d, %dx%d", width, height, width / 2, height / 2, width / 2, height / 2);
        return -1;
    }
    box2i w;
    if (cvs_raster_window(&frame->full_window, width, height, &w)) return 0;
    const half *lut = cvs_ycc_import_lut();
    if (!lut) return -1;
    cvk_dv_planes pl = cvs_planes_view(planar);
    const int rc = cvk_mpeg2_reconstruct(cvs_view(frame->data, &frame->full_window), cvs_rect(&w), &pl, width, height, progressive, cvs_ycc_to_rgb(flags), lut,
                                         cvs_cus(), cvs_pick_stream(stream));
    if (rc != 0) { cvs_set_error("MPEG-2 reconstruct: %s", hipGetErrorString((hipError_t)rc)); return rc; }
    frame->current_window = w;
    return 0;
}

/* reference-named entry point on host memory: the reference's 720x480, interlaced, Rec.601; planes staged in one pooled block */
CVS_EXPORT void video_reconstruct_mpeg2(rgba_frame_f16 *frame, coded_image *planar) {
    cvs_bridge br;
    rgba_frame_f16 dframe;
    coded_image dev;
    if (!frame) return;
    box2i_set_empty(&frame->current_window);
    if (cvs_bridge_open(&br) != 0) return;
    if (cvs_planes_check(planar, 0, 0, 0, 0) == CVS_PLANES_MISSING) { cvs_set_error("MPEG-2 reconstruct: need three planes"); return; }
    CVS_BRIDGE_FRAME(&br, dframe, frame, 0);
    cvs_bridge_planes(&br, &dev, planar, planar->line_count, true);
    CVS_BRIDGE_CALL(&br, cvs_reconstruct_mpeg2_dev, &dframe, &dev, MPEG2_W, MPEG2_H, 0);
    /* pixels outside the current window keep what the caller's buffer held: only the written rows come back */
    if (br.rc == 0 && !box2i_is_empty(&dframe.current_window) &&
        cvs_bridge_pull_window(&br, frame->data, &frame->full_window, &dframe.current_window, sizeof(rgba_f16)) != 0)
        cvs_set_error("MPEG-2 reconstruct: download failed");
    if (cvs_bridge_close(&br, NULL) == 0) frame->current_window = dframe.current_window;
}
