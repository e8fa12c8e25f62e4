/*
 * oracle.h -- CPU restatement of the Canvas src/cprocess per-pixel video path.
 *
 * TEST INFRASTRUCTURE ONLY.  Nothing under canvas_amd/ may include, link or
 * call this.  Only tests/, __graft_entry__.smoke() and bench.py's
 * cpu_baseline leg use it, and only as the checker / reported CPU baseline.
 *
 * Pinning status ("how do we know this restatement is right?"):
 *   - Where the reference tree is present, oracle/ref_build.py compiles its own
 *     src/cprocess in place into oracle/_ref/ (gcc and clang flavours), and
 *     tests/test_oracle_against_reference.py holds every function below that
 *     has a CPU implementation there to it, bit for bit.
 *   - Pinned by the reference's own known-answer tests: crossfade KAT
 *     (tests/canvas/sequence.py:58-100), solid/window KATs
 *     (tests/process/video/RgbaFrameF16.py:6-23,
 *      tests/process/video/SolidColorVideoSource.py:13-55).
 *   - h2f is additionally checked against IEEE-754 (numpy) for all 65536
 *     codes and f2h against an independent integer round-toward-zero model.
 *   - over / scale / named colour functions / LUT / tap values: the reference
 *     holds no test or fixture for them; they are pinned by that build.
 *     Gaussian blur, gain/offset rounding, the general matrix and everything
 *     else without a CPU implementation in the reference are defined by this
 *     project alone (Part II A).
 *
 * All file:line citations are relative to /root/reference.
 * Struct layouts follow include/framework.h:46-75,155-213,618-627 so the same
 * ctypes structures drive the oracle and the product library.
 */
#ifndef CANVAS_ORACLE_H
#define CANVAS_ORACLE_H

#include <stdint.h>
#include <stddef.h>

typedef uint16_t orc_half;

typedef struct { int32_t x, y; } orc_v2i;
typedef struct { orc_v2i min, max; } orc_box2i;
typedef struct { float x, y; } orc_v2f;
typedef struct { orc_half r, g, b, a; } orc_px16;
typedef struct { float r, g, b, a; } orc_px32;

typedef struct { orc_px16 *data; orc_box2i full_window, current_window; } orc_frame16;
typedef struct { orc_px32 *data; orc_box2i full_window, current_window; } orc_frame32;

typedef void (*orc_get16_fn)(void *self, int frame_index, orc_frame16 *frame);
typedef void (*orc_get32_fn)(void *self, int frame_index, orc_frame32 *frame);
typedef struct { int flags; orc_get16_fn get_frame; orc_get32_fn get_frame_32; void *reserved; } orc_source_funcs;
typedef struct { void *obj; orc_source_funcs *funcs; } orc_source;

typedef struct { float *coeff; int width; int center; } orc_fir;

/* half.c / genhalf.py */
void orc_half_to_float(float *out, const orc_half *in, int count);
void orc_float_to_half(orc_half *out, const float *in, int count);
void orc_half_to_float_fast(float *out, const orc_half *in, int count);
void orc_float_to_half_fast(orc_half *out, const float *in, int count);
void orc_half_lookup(const orc_half *table, orc_half *out, const orc_half *in, int count);

/* gammatab.c */
enum { ORC_LUT_REC709_TO_LINEAR_SCENE = 0, ORC_LUT_REC709_TO_LINEAR_DISPLAY = 1,
       ORC_LUT_LINEAR_TO_REC709 = 2, ORC_LUT_LINEAR_TO_SRGB = 3 };
const orc_half *orc_transfer_table(int which);
void orc_transfer(int which, orc_half *out, const orc_half *in, size_t count);
const uint8_t *orc_gamma45_ramp(void);

/* filter.c */
void orc_fir_triangle(float sub, float offset, orc_fir *f);
void orc_fir_lanczos(float sub, int kernel_size, float offset, orc_fir *f);
void orc_fir_free(orc_fir *f);

/* main.c */
void orc_get_frame_f16(orc_source *src, int frame_index, orc_frame16 *frame);
void orc_get_frame_f32(orc_source *src, int frame_index, orc_frame32 *frame);

/* video_mix.c */
void orc_copy_frame_f16(orc_frame16 *out, orc_frame16 *in);
void orc_copy_frame_alpha_f32(orc_frame32 *out, orc_frame32 *in, float alpha);
void orc_mix_cross_f32(orc_frame32 *out, orc_frame32 *a, orc_frame32 *b, float mix_b);
void orc_mix_cross_f32_pull(orc_frame32 *out, orc_source *a, int frame_a, orc_source *b, int frame_b, float mix_b);
void orc_mix_over_f32(orc_frame32 *out, orc_frame32 *b, float mix_b);

/* video_scale.c */
void orc_scale_bilinear_f32(orc_frame32 *target, orc_v2f target_point, orc_frame32 *source,
                            orc_v2f source_point, orc_v2f factors);
void orc_scale_bilinear_f32_pull(orc_frame32 *target, orc_v2f target_point, orc_source *source, int frame,
                                 orc_box2i *source_rect, orc_v2f source_point, orc_v2f factors);

/* color.c -- generic form + the two named instances.  m is COLUMN-major as the
 * reference passes it: m[0..2] = "r" column (a.x a.y a.z), m[3..5] = "g", m[6..8] = "b". */
void orc_color_matrix_f16(orc_frame16 *frame, const float m[9], const orc_half *pre_lut, const orc_half *post_lut);
void orc_color_rgb_to_xyz_sdtv(orc_frame16 *frame);
void orc_color_xyz_to_srgb(orc_frame16 *frame);

/* semantics the reference only has in GLSL / Python-layer C */
void orc_gain_offset_f16(orc_frame16 *out, orc_frame16 *in, float gain, float offset);
void orc_solid_f16(orc_frame16 *frame, const orc_box2i *window, const float color[4]);
void orc_solid_f32(orc_frame32 *frame, const orc_box2i *window, const float color[4]);

/* the repo's definition of separable FIR blur (absent from the reference) */
void orc_fir_blur_f32(orc_frame32 *target, orc_frame32 *source, const float *taps, int ntaps);
/* gather resample with caller-supplied per-output tap generator (Lanczos path; no reference caller) */
void orc_resample_lanczos_f32(orc_frame32 *target, orc_frame32 *source, float factor_x, float factor_y, int kernel_size);

/* 2:3 pulldown removal (src/process/Pulldown23RemovalFilter.c:43-107) */
int orc_pulldown23_frames(int offset, int frame_index, int *first, int *second);
void orc_weave_fields_f16(orc_frame16 *frame, const orc_frame16 *other);
void orc_pulldown23_get_frame_f16(orc_source *source, int offset, int frame_index, orc_frame16 *frame);

/* workspace.c video stack, as a pure function of the item list */
typedef struct { int64_t x, length, z, offset; orc_source *source; } orc_ws_item;
void orc_workspace_get_frame_f32(const orc_ws_item *items, int n, int frame_index, orc_frame32 *frame);

/* DV 4:1:1 edge (dv.c): planes = Y 720x480, Cb 180x480, Cr 180x480, 8 bits */
void orc_reconstruct_dv(orc_frame16 *frame, const uint8_t *const planes[3], const int strides[3]);   /* video_reconstruct.c:50-137 */
void orc_subsample_dv(uint8_t *const planes[3], const int strides[3], orc_frame16 *frame);           /* video_subsample.c:99-187 */

/* display / export edge: widget_gl.c:291-307, writeVideo.c:328-340 (mode 0), RgbaFrameF16.c:114-149 (mode 1) */
void orc_frame_to_bytes(uint32_t *dst, const orc_frame16 *frame, const orc_half *pre, int mode);
void orc_widget_ramp(uint8_t *ramp, float rendering_intent);                                         /* widget_gl.c:955-968 */
void orc_frame_to_rgba8_intent(uint32_t *dst, const orc_frame16 *frame, const orc_half *pre, float rendering_intent);

/* fused chain of BASELINE config 2, composed from the pieces above (bench cpu_baseline + parity) */
void orc_chain_color_over_f16(orc_frame16 *out, orc_frame16 *const *layers, int nlayers,
                              const float m[9], const orc_half *pre_lut, const orc_half *post_lut);

#endif
