"""ctypes binding of libcanvas_hip.so (the C-ABI declared in include/canvas_hip.h and, for the scopes, the 3D LUT, the corner pin
the adaptive deinterlacer, the median and the temporal denoise, include/canvas_scope.h, include/canvas_lut3d.h,
include/canvas_perspective.h, include/canvas_deinterlace.h, include/canvas_median.h, include/canvas_temporal.h,
include/canvas_ycc422.h, include/canvas_ycc420.h, include/canvas_primary.h and include/canvas_secondary.h).

There is no fallback: if the shared library is missing or cannot be loaded, importing symbols
from here raises, and every pixel entry point needs a HIP device at run time.
"""
import ctypes as C
import os

from .abi import (box2i, fir_filter, rational, rgba_frame_f16, rgba_frame_f32, v2f, v2i, video_frame_source_funcs,
                  video_source)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libcanvas_hip.so")

CHAIN_MAX_LAYERS = 8
DISPLAY_RGBA8, DISPLAY_ARGB32_PREMUL = 0, 1
FIR_PATH_AUTO, FIR_PATH_PASSES, FIR_PATH_TILED, FIR_PATH_TABLES, FIR_PATH_HV, FIR_PATH_ONE_COLUMN, FIR_PATH_TWO_COLUMNS, FIR_PATH_STRIPS, FIR_PATH_TILES = 0, 1, 2, 4, 16, 32, 64, 128, 256
FIR_KERNEL_NONE, FIR_KERNEL_WINDOW, FIR_KERNEL_HALVE, _FIR_KERNEL_RETIRED_3, FIR_KERNEL_VH, FIR_KERNEL_TILED, _FIR_KERNEL_RETIRED_6, FIR_KERNEL_TWO_PASS, FIR_KERNEL_PASS, FIR_KERNEL_HV, FIR_KERNEL_WINDOW_PAIR, FIR_KERNEL_HALVE_PAIR, FIR_KERNEL_TILE_VH, FIR_KERNEL_UNSHARP = range(14)
ARITH_SEPARATE, ARITH_CONTRACTED = 0, 1          # cvs_set_arithmetic: the reference's gcc build / its clang (contracting) build
LUT_NONE, LUT_REC709_TO_LINEAR_SCENE, LUT_REC709_TO_LINEAR_DISPLAY, LUT_LINEAR_TO_REC709, LUT_LINEAR_TO_SRGB = -1, 0, 1, 2, 3
KEY_SHOW_MATTE = 1                                  # cvs_chroma_key.flags
MATTE_SHOW, MATTE_MAX_CHOKE, MATTE_MAX_TAPS = 1, 16, 25    # cvs_matte.flags and its limits
TRANSFORM_NEAREST, TRANSFORM_BILINEAR, TRANSFORM_MAX_COORD = 0, 1, 1 << 23    # cvs_transform.filter and the coordinate limit
TRANSFORM_CATMULL_ROM = 4                                                   # (the filter's support in samples per axis)
MAX_COORD, RESAMPLE_MAX_COORD = 1 << 30, 1 << 23        # the coordinate contract of canvas_hip.h: every entry's bound, the resamplers'
SCOPE_HISTOGRAM, SCOPE_WAVEFORM, SCOPE_PARADE, SCOPE_VECTORSCOPE = range(4)      # cvs_scope.kind
SCOPE_SKIP_TRANSPARENT, SCOPE_MAX_COLUMNS = 1, 4096                             # cvs_scope.flags and the limit of its columns
LUT3D_MIN_SIZE, LUT3D_MAX_SIZE = 2, 65                                           # cvs_lut3d.size
CURVES_MIN_SIZE, CURVES_MAX_SIZE, PRIMARY_MATRIX = 2, 4097, 1                    # cvs_curves.size, cvs_primary.flags
QUAL_HUE, QUAL_SATURATION, QUAL_LUMA, QUAL_INVERT, QUAL_SHOW_MATTE = 1, 2, 4, 8, 16                   # cvs_qualifier.flags
MMIX_LUMA, MMIX_INVERT = 1, 2                                                    # cvs_matte_mix.flags
PERSPECTIVE_MAX_SPAN = 1 << 23                                                   # cvs_perspective: how far a window may lie from its origin
YCC_PROGRESSIVE, YCC_REC709 = 1, 2                  # cvs_reconstruct_mpeg2_dev flags (0: interlaced siting, Rec.601)


class rgba_f32(C.Structure):
    _fields_ = [("r", C.c_float), ("g", C.c_float), ("b", C.c_float), ("a", C.c_float)]


class rgba_frame_dev(C.Structure):
    _fields_ = [("data", C.c_void_p), ("format", C.c_int), ("full_window", box2i), ("current_window", box2i),
                ("stream", C.c_void_p)]


class chain_job(C.Structure):
    _fields_ = [("out", C.POINTER(rgba_frame_f16)), ("layers", C.POINTER(rgba_frame_f16) * CHAIN_MAX_LAYERS),
                ("nlayers", C.c_int)]


class chroma_key(C.Structure):
    _fields_ = [("key", C.c_float * 3), ("tolerance", C.c_float), ("softness", C.c_float), ("spill", C.c_float),
                ("spill_range", C.c_float), ("flags", C.c_int)]


class matte_params(C.Structure):
    _fields_ = [("black", C.c_float), ("white", C.c_float), ("choke", C.c_int), ("ntaps", C.c_int), ("taps", C.POINTER(C.c_float)),
                ("flags", C.c_int)]


def matte(choke=0, feather=None, black=0.0, white=1.0, show_matte=False):
    """A cvs_matte for the two cvs_matte_refine entries; the tap array lives as long as the struct returned."""
    taps = [float(t) for t in feather] if feather is not None else []
    array = (C.c_float * len(taps))(*taps) if taps else None
    m = matte_params(black, white, int(choke), len(taps), C.cast(array, C.POINTER(C.c_float)) if taps else None, MATTE_SHOW if show_matte else 0)
    m._taps = array
    return m


class transform_params(C.Structure):
    _fields_ = [("m", C.c_float * 6), ("filter", C.c_int), ("flags", C.c_int)]


def transform(m=(1.0, 0.0, 0.0, 0.0, 1.0, 0.0), filter=TRANSFORM_BILINEAR):
    """A cvs_transform for the two cvs_transform entries and the window helpers: m maps target to source coordinates."""
    return transform_params((C.c_float * 6)(*[float(v) for v in m]), int(filter), 0)


class scope_params(C.Structure):
    _fields_ = [("kind", C.c_int), ("pre_lut", C.c_int), ("rendering_intent", C.c_float), ("columns", C.c_int), ("flags", C.c_int),
                ("region", box2i)]


def scope(kind, region, columns=256, pre_lut=LUT_NONE, rendering_intent=0.0, flags=0):
    """A cvs_scope for the scope entries; region: a box2i (copied) or (x0, y0, x1, y1)."""
    r = region if isinstance(region, box2i) else box2i.of(*region)
    return scope_params(int(kind), int(pre_lut), float(rendering_intent), int(columns), int(flags), box2i.of(*r.tuple()))


class lut3d_params(C.Structure):
    _fields_ = [("size", C.c_int), ("domain_min", C.c_float * 3), ("domain_max", C.c_float * 3), ("flags", C.c_int)]


def lut3d(size, domain_min=(0.0, 0.0, 0.0), domain_max=(1.0, 1.0, 1.0), flags=0):
    """A cvs_lut3d for the two cvs_lut3d entries: a lattice of size^3 nodes whose ends sit on domain_min and domain_max."""
    return lut3d_params(int(size), (C.c_float * 3)(*[float(v) for v in domain_min]), (C.c_float * 3)(*[float(v) for v in domain_max]), int(flags))


class curves_params(C.Structure):
    _fields_ = [("size", C.c_int), ("domain_min", C.c_float * 3), ("domain_max", C.c_float * 3)]


class primary_params(C.Structure):
    _fields_ = [("pre", curves_params), ("matrix", C.c_float * 12), ("post", curves_params), ("flags", C.c_int)]


def curves(size=0, domain_min=(0.0, 0.0, 0.0), domain_max=(1.0, 1.0, 1.0)):
    """A cvs_curves: three tables of `size` nodes whose ends sit on domain_min and domain_max; size 0: the stage is absent."""
    return curves_params(int(size), (C.c_float * 3)(*[float(v) for v in domain_min]), (C.c_float * 3)(*[float(v) for v in domain_max]))


def primary(pre=None, matrix=None, post=None, flags=None):
    """A cvs_primary for the two cvs_primary entries.  pre / post: None (absent), a size, or (size, domain_min, domain_max);
    matrix: None (absent) or 12 numbers, three rows of four.  flags: PRIMARY_MATRIX exactly when a matrix is given, unless stated."""
    def stage(v):
        if v is None:
            return curves()
        return curves(v) if isinstance(v, int) else curves(*v)
    m = [0.0] * 12 if matrix is None else [float(v) for row in matrix for v in (row if hasattr(row, "__len__") else [row])]
    if len(m) != 12:
        raise ValueError("matrix takes 12 numbers, three rows of four")
    return primary_params(stage(pre), (C.c_float * 12)(*m), stage(post), int((PRIMARY_MATRIX if matrix is not None else 0) if flags is None else flags))


class hue_range(C.Structure):
    _fields_ = [("center", C.c_float), ("width", C.c_float), ("softness", C.c_float)]


class value_range(C.Structure):
    _fields_ = [("low", C.c_float), ("high", C.c_float), ("soft_low", C.c_float), ("soft_high", C.c_float)]


class qualifier_params(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("hue", hue_range), ("saturation", value_range), ("luma", value_range)]


class matte_mix_params(C.Structure):
    _fields_ = [("flags", C.c_uint32)]


def qualifier(hue=None, saturation=None, luma=None, invert=False, show_matte=False, flags=None):
    """A cvs_qualifier for the two cvs_qualify entries.  hue: None (the axis does not qualify) or (center, width, softness) in
    degrees; saturation / luma: None or (low, high, soft_low, soft_high).  flags: the axes given, invert and show_matte, unless
    stated."""
    f = (QUAL_HUE if hue is not None else 0) | (QUAL_SATURATION if saturation is not None else 0) | (QUAL_LUMA if luma is not None else 0)
    f |= (QUAL_INVERT if invert else 0) | (QUAL_SHOW_MATTE if show_matte else 0)
    h = hue_range(*[float(v) for v in hue]) if hue is not None else hue_range()
    s = value_range(*[float(v) for v in saturation]) if saturation is not None else value_range()
    y = value_range(*[float(v) for v in luma]) if luma is not None else value_range()
    return qualifier_params(int(f if flags is None else flags) & 0xFFFFFFFF, h, s, y)


def matte_mix(luma=False, invert=False, flags=None):
    """A cvs_matte_mix for the two cvs_matte_mix entries: k from the matte's alpha, or from its Rec.709 luma; inverted or not."""
    return matte_mix_params(int(((MMIX_LUMA if luma else 0) | (MMIX_INVERT if invert else 0)) if flags is None else flags) & 0xFFFFFFFF)


class perspective_params(C.Structure):
    _fields_ = [("h", C.c_float * 9), ("target_origin", C.c_int * 2), ("source_origin", C.c_int * 2), ("filter", C.c_int), ("flags", C.c_int)]


def perspective(h=(1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0), target_origin=(0, 0), source_origin=(0, 0), filter=TRANSFORM_BILINEAR, flags=0):
    """A cvs_perspective for the two cvs_perspective entries and the window helpers: h maps target to source coordinates, each
    side counted from its origin."""
    return perspective_params((C.c_float * 9)(*[float(v) for v in h]), (C.c_int * 2)(*[int(v) for v in target_origin]),
                              (C.c_int * 2)(*[int(v) for v in source_origin]), int(filter), int(flags))


class deinterlace_params(C.Structure):
    _fields_ = [("field", C.c_int), ("threshold", C.c_float), ("softness", C.c_float), ("flags", C.c_int)]


def deinterlace_adaptive(field=0, threshold=0.02, softness=0.04, flags=0):
    """A cvs_deinterlace_adaptive for cvs_deinterlace_adaptive_f16_dev."""
    return deinterlace_params(int(field), float(threshold), float(softness), int(flags))


MEDIAN_R, MEDIAN_G, MEDIAN_B, MEDIAN_A, MEDIAN_COLOUR, MEDIAN_ALL = 1, 2, 4, 8, 7, 15


class median_params(C.Structure):
    _fields_ = [("radius", C.c_int), ("threshold", C.c_float), ("channels", C.c_int), ("flags", C.c_int)]


def median(radius=1, threshold=0.0, channels=MEDIAN_ALL, flags=0):
    """A cvs_median for cvs_median_f16_dev / _f32_dev."""
    return median_params(int(radius), float(threshold), int(channels), int(flags))


class temporal_params(C.Structure):
    _fields_ = [("threshold", C.c_float), ("softness", C.c_float), ("channels", C.c_int), ("flags", C.c_int)]


def temporal_denoise(threshold=0.02, softness=0.04, channels=MEDIAN_ALL, flags=0):
    """A cvs_temporal_denoise for cvs_temporal_denoise_f16_dev; channels: a MEDIAN_* mask."""
    return temporal_params(float(threshold), float(softness), int(channels), int(flags))


class coded_image(C.Structure):
    _fields_ = [("data", C.c_void_p * 4), ("stride", C.c_int * 4), ("line_count", C.c_int * 4), ("free_func", C.c_void_p)]


P = C.POINTER
rgba_frame_f16_t = rgba_frame_f16
rgba_frame_f32_t = rgba_frame_f32
_u16p, _f32p, _vp = P(C.c_uint16), P(C.c_float), C.c_void_p
_F16, _F32 = P(rgba_frame_f16), P(rgba_frame_f32)

# name -> (restype, argtypes); this table is also what tests use to check that every symbol the
# header declares is exported.
SIGNATURES = {
    # (1) reference symbol set, host frames
    "init_half": (None, []),
    "get_frame_time": (C.c_int64, [P(rational), C.c_int]),
    "get_time_frame": (C.c_int, [P(rational), C.c_int64]),
    "gettime": (C.c_int64, []),
    "video_get_frame_f16": (None, [P(video_source), C.c_int, _F16]),
    "video_get_frame_f32": (None, [P(video_source), C.c_int, _F32]),
    "video_get_frame_f16_gl": (None, [P(video_source), C.c_int, _F16]),
    "video_get_frame_f32_gl": (None, [P(video_source), C.c_int, _F32]),
    "video_get_frame_dev": (None, [P(video_source), C.c_int, P(rgba_frame_dev)]),
    "video_copy_frame_f16": (None, [_F16, _F16]),
    "video_copy_frame_alpha_f32": (None, [_F32, _F32, C.c_float]),
    "video_attenuate_f32": (None, [_F32, C.c_float]),
    "cvs_pulldown23_frames": (C.c_int, [C.c_int, C.c_int, P(C.c_int), P(C.c_int)]),
    "cvs_weave_fields_f16_dev": (C.c_int, [_F16, _F16, _vp]),
    "cvs_field_to_frame_f16_dev": (C.c_int, [_F16, _F16, C.c_int, _vp]),
    "cvs_soften_fields_f16_dev": (C.c_int, [_F16, _F16, _vp]),
    "cvs_interlace_fields_f16_dev": (C.c_int, [_F16, _F16, _F16, _vp]),
    "cvs_pulldown23_add_frames": (C.c_int, [C.c_int, C.c_int, P(C.c_int), P(C.c_int)]),
    "video_mix_cross_f32": (None, [_F32, _F32, _F32, C.c_float]),
    "video_mix_cross_f32_pull": (None, [_F32, P(video_source), C.c_int, P(video_source), C.c_int, C.c_float]),
    "video_mix_over_f32": (None, [_F32, _F32, C.c_float]),
    "video_scale_bilinear_f32": (None, [_F32, v2f, _F32, v2f, v2f]),
    "video_scale_bilinear_f32_pull": (None, [_F32, v2f, P(video_source), C.c_int, P(box2i), v2f, v2f]),
    "video_transfer_rec709_to_linear_scene": (None, [_u16p, _u16p, C.c_size_t]),
    "video_transfer_rec709_to_linear_display": (None, [_u16p, _u16p, C.c_size_t]),
    "video_transfer_linear_to_rec709": (None, [_u16p, _u16p, C.c_size_t]),
    "video_transfer_linear_to_sRGB": (None, [_u16p, _u16p, C.c_size_t]),
    "video_get_gamma45_ramp": (P(C.c_uint8), []),
    "video_color_rgb_to_xyz_sdtv": (None, [_F16]),
    "video_color_xyz_to_srgb": (None, [_F16]),
    "filter_createTriangle": (None, [C.c_float, C.c_float, P(fir_filter)]),
    "filter_createLanczos": (None, [C.c_float, C.c_int, C.c_float, P(fir_filter)]),
    "filter_free": (None, [P(fir_filter)]),
    "video_filter_gain_offset_f16": (None, [_F16, _F16, C.c_float, C.c_float]),
    "video_fill_solid_f16": (None, [_F16, P(box2i), P(rgba_f32)]),
    "video_fill_solid_f32": (None, [_F32, P(box2i), P(rgba_f32)]),
    "workspace_create": (_vp, []),
    "workspace_get_length": (C.c_int, [_vp]),
    "workspace_add_item": (_vp, [_vp, _vp, C.c_int64, C.c_int64, C.c_int64, C.c_int64, _vp]),
    "workspace_get_item": (_vp, [_vp, C.c_int]),
    "workspace_remove_item": (None, [_vp]),
    "workspace_as_video_source": (None, [_vp, P(video_source)]),
    "workspace_free": (None, [_vp]),
    "workspace_get_item_pos": (None, [_vp, P(C.c_int64), P(C.c_int64), P(C.c_int64)]),
    "workspace_get_item_offset": (C.c_int64, [_vp]),
    "workspace_set_item_offset": (None, [_vp, C.c_int64]),
    "workspace_get_item_source": (_vp, [_vp]),
    "workspace_set_item_source": (None, [_vp, _vp]),
    "workspace_get_item_tag": (_vp, [_vp]),
    "workspace_set_item_tag": (None, [_vp, _vp]),
    "workspace_update_item": (None, [_vp, P(C.c_int64), P(C.c_int64), P(C.c_int64), P(C.c_int64), P(_vp), P(_vp)]),
    # (2) runtime + device twins
    "cvs_set_arithmetic": (C.c_int, [C.c_int]),
    "cvs_get_arithmetic": (C.c_int, []),
    "cvs_init": (C.c_int, [C.c_int]),
    "cvs_device_count": (C.c_int, []),
    "cvs_current_device": (C.c_int, []),
    "cvs_context_open": (C.c_int, [C.c_int]),
    "cvs_context_count": (C.c_int, []),
    "cvs_context_device": (C.c_int, [C.c_int]),
    "cvs_set_context": (C.c_int, [C.c_int]),
    "cvs_current_context": (C.c_int, []),
    "cvs_frame_owner": (C.c_int, [C.c_int64, C.c_int]),
    "cvs_last_error": (C.c_char_p, []),
    "cvs_clear_last_error": (None, []),
    "cvs_set_log_handler": (None, [C.c_void_p, C.c_void_p]),
    "cvs_device_name": (C.c_char_p, []),
    "cvs_compute_units": (C.c_int, []),
    "cvs_malloc": (_vp, [C.c_size_t]),
    "cvs_free": (None, [_vp]),
    "cvs_graph_begin": (C.c_int, [_vp]),
    "cvs_graph_end": (_vp, [_vp]),
    "cvs_graph_launch": (C.c_int, [_vp, _vp]),
    "cvs_graph_destroy": (None, [_vp]),
    "cvs_mem_info": (C.c_int, [P(C.c_size_t), P(C.c_size_t)]),
    "cvs_pool_malloc": (_vp, [C.c_size_t, _vp]),
    "cvs_pool_free": (None, [_vp, _vp]),
    "cvs_pool_trim": (None, []),
    "cvs_thread_release": (None, []),
    "cvs_memcpy_h2d": (C.c_int, [_vp, _vp, C.c_size_t, _vp]),
    "cvs_memcpy_d2h": (C.c_int, [_vp, _vp, C.c_size_t, _vp]),
    "cvs_memcpy_d2d": (C.c_int, [_vp, _vp, C.c_size_t, _vp]),
    "cvs_memset": (C.c_int, [_vp, C.c_int, C.c_size_t, _vp]),
    "cvs_stream_create": (_vp, []),
    "cvs_stream_destroy": (None, [_vp]),
    "cvs_stream_sync": (C.c_int, [_vp]),
    "cvs_event_create": (_vp, []),
    "cvs_event_destroy": (None, [_vp]),
    "cvs_event_record": (C.c_int, [_vp, _vp]),
    "cvs_event_sync": (C.c_int, [_vp]),
    "cvs_event_elapsed_ms": (C.c_float, [_vp, _vp]),
    "cvs_lut_device": (_vp, [C.c_int]),
    "cvs_lut_host": (_u16p, [C.c_int]),
    "cvs_lut_install": (C.c_int, [C.c_int, _u16p]),
    "cvs_half_to_float_dev": (C.c_int, [_vp, _vp, C.c_size_t, _vp]),
    "cvs_float_to_half_dev": (C.c_int, [_vp, _vp, C.c_size_t, _vp]),
    "cvs_half_to_float_fast_dev": (C.c_int, [_vp, _vp, C.c_size_t, _vp]),
    "cvs_float_to_half_fast_dev": (C.c_int, [_vp, _vp, C.c_size_t, _vp]),
    "cvs_half_lookup_dev": (C.c_int, [_vp, _vp, _vp, C.c_size_t, _vp]),
    "cvs_frame_f16_to_f32_dev": (C.c_int, [_F32, _F16, _vp]),
    "cvs_frame_f32_to_f16_dev": (C.c_int, [_F16, _F32, _vp]),
    "cvs_copy_frame_f16_dev": (C.c_int, [_F16, _F16, _vp]),
    "cvs_copy_frame_alpha_f32_dev": (C.c_int, [_F32, _F32, C.c_float, _vp]),
    "cvs_mix_cross_f32_dev": (C.c_int, [_F32, _F32, _F32, C.c_float, _vp]),
    "cvs_mix_over_f32_dev": (C.c_int, [_F32, _F32, C.c_float, _vp]),
    "cvs_color_matrix_f16_dev": (C.c_int, [_F16, _f32p, C.c_int, C.c_int, _vp]),
    "cvs_color_matrix_f16_to_dev": (C.c_int, [_F16, _F16, _f32p, C.c_int, C.c_int, _vp]),
    "cvs_gain_offset_f16_dev": (C.c_int, [_F16, _F16, C.c_float, C.c_float, _vp]),
    "cvs_fill_solid_f16_dev": (C.c_int, [_F16, P(box2i), P(rgba_f32), _vp]),
    "cvs_fill_solid_f32_dev": (C.c_int, [_F32, P(box2i), P(rgba_f32), _vp]),
    "cvs_scale_bilinear_f16_dev": (C.c_int, [_F16, v2f, _F16, v2f, v2f, _vp]),
    "cvs_scale_bilinear_f32_dev": (C.c_int, [_F32, v2f, _F32, v2f, v2f, _vp]),
    "cvs_fir_blur_f32_dev": (C.c_int, [_F32, _F32, _f32p, C.c_int, _vp]),
    "coded_image_alloc": (P(coded_image), [P(C.c_int), P(C.c_int), C.c_int]),
    "coded_image_alloc0": (P(coded_image), [P(C.c_int), P(C.c_int), C.c_int]),
    "video_reconstruct_dv": (None, [_F16, P(coded_image)]),
    "video_subsample_dv": (P(coded_image), [_F16]),
    "cvs_reconstruct_dv_dev": (C.c_int, [_F16, P(coded_image), _vp]),
    "cvs_subsample_dv_dev": (C.c_int, [P(coded_image), _F16, C.c_int, _vp]),
    "video_subsample_mpeg2": (P(coded_image), [_F16]),
    "cvs_subsample_mpeg2_dev": (C.c_int, [P(coded_image), _F16, C.c_int, C.c_int, _vp]),
    "video_reconstruct_mpeg2": (None, [_F16, P(coded_image)]),
    "cvs_reconstruct_mpeg2_dev": (C.c_int, [_F16, P(coded_image), C.c_int, C.c_int, C.c_int, _vp]),
    "cvs_frame_to_bytes_dev": (C.c_int, [_vp, _F16, C.c_int, C.c_int, _vp]),
    "video_frame_to_bytes": (C.c_int, [_vp, _F16, C.c_int, C.c_int]),
    "cvs_frame_to_rgba8_intent_dev": (C.c_int, [_vp, _F16, C.c_int, C.c_float, _vp]),
    "video_frame_to_rgba8_intent": (C.c_int, [_vp, _F16, C.c_int, C.c_float]),
    "cvs_fir_blur_f16_dev": (C.c_int, [_F16, _F16, _f32p, C.c_int, _vp]),
    "cvs_unsharp_mask_f32_dev": (C.c_int, [_F32, _F32, _f32p, C.c_int, C.c_float, C.c_float, _vp]),
    "cvs_unsharp_mask_f16_dev": (C.c_int, [_F16, _F16, _f32p, C.c_int, C.c_float, C.c_float, _vp]),
    "cvs_chroma_key_f32_dev": (C.c_int, [_F32, _F32, P(chroma_key), _vp]),
    "cvs_chroma_key_f16_dev": (C.c_int, [_F16, _F16, P(chroma_key), _vp]),
    "cvs_matte_refine_f32_dev": (C.c_int, [_F32, _F32, P(matte_params), _vp]),
    "cvs_matte_refine_f16_dev": (C.c_int, [_F16, _F16, P(matte_params), _vp]),
    "cvs_transform_f32_dev": (C.c_int, [_F32, _F32, P(transform_params), _vp]),
    "cvs_transform_f16_dev": (C.c_int, [_F16, _F16, P(transform_params), _vp]),
    "cvs_transform_from_parts": (C.c_int, [P(C.c_double), P(C.c_double), C.c_double, P(C.c_double), _f32p]),
    "cvs_transform_target_window": (C.c_int, [P(transform_params), P(box2i), P(box2i), P(box2i)]),
    "cvs_transform_source_window": (C.c_int, [P(transform_params), P(box2i), P(box2i)]),
    "cvs_blur_over_f16_dev": (C.c_int, [_F16, _F16, _f32p, C.c_int, P(_F16), C.c_int, _vp]),
    "cvs_resample_lanczos_f32_dev": (C.c_int, [_F32, _F32, C.c_float, C.c_float, C.c_int, _vp]),
    "cvs_resample_lanczos_f16_dev": (C.c_int, [_F16, _F16, C.c_float, C.c_float, C.c_int, _vp]),
    "cvs_blur_lanczos_f16_dev": (C.c_int, [_F16, _F16, _f32p, C.c_int, C.c_float, C.c_float, C.c_int, _vp]),
    "cvs_blur_over_f16_batch_dev": (C.c_int, [P(_F16), P(_F16), _f32p, C.c_int, P(_F16), C.c_int, C.c_int, _vp]),
    "cvs_scale_bilinear_f16_batch_dev": (C.c_int, [P(_F16), v2f, P(_F16), v2f, v2f, C.c_int, _vp]),
    "cvs_scale_bilinear_f32_batch_dev": (C.c_int, [P(_F32), v2f, P(_F32), v2f, v2f, C.c_int, _vp]),
    "cvs_blur_lanczos_f16_batch_dev": (C.c_int, [P(_F16), P(_F16), C.c_int, _f32p, C.c_int, C.c_float, C.c_float, C.c_int, _vp]),
    "cvs_fir_path_override": (None, [C.c_int]),
    # (3) fused chain
    "cvs_chain_color_over_f16_dev": (C.c_int, [P(chain_job), C.c_int, _f32p, C.c_int, C.c_int, _vp]),
    "cvs_chain_last_was_fused": (C.c_int, []),
    "cvs_scale_last_was_fused": (C.c_int, []),
    "cvs_fir_last_kernel": (C.c_int, []),
    "cvs_fir_fell_through_count": (C.c_int, []),
    "cvs_chain_last_launch_count": (C.c_int, []),
    "cvs_mix_cross_f16_dev": (C.c_int, [_F16, _F16, _F16, C.c_float, _vp]),
}

# the same for include/canvas_scope.h (video scopes): name -> (restype, argtypes), every function that header declares
SCOPE_SIGNATURES = {
    "cvs_scope_count": (C.c_size_t, [P(scope_params)]),
    "cvs_scope_picture_size": (C.c_int, [P(scope_params), P(v2i)]),
    "cvs_scope_counts_f16_dev": (C.c_int, [_vp, _F16, P(scope_params), _vp]),
    "cvs_scope_render_f16_dev": (C.c_int, [_F16, P(box2i), _vp, P(scope_params), C.c_float, _vp]),
    "video_scope_counts": (C.c_int, [_vp, _F16, P(scope_params)]),
}

# the same for include/canvas_lut3d.h (3D colour LUT)
LUT3D_SIGNATURES = {
    "cvs_lut3d_bytes": (C.c_size_t, [C.c_int]),
    "cvs_lut3d_pack": (C.c_int, [_f32p, _f32p, C.c_int]),
    "cvs_lut3d_f16_dev": (C.c_int, [_F16, _F16, _vp, P(lut3d_params), _vp]),
    "cvs_lut3d_f32_dev": (C.c_int, [_F32, _F32, _vp, P(lut3d_params), _vp]),
}

# the same for include/canvas_primary.h (primary colour correction: curves, matrix, curves)
PRIMARY_SIGNATURES = {
    "cvs_curves_bytes": (C.c_size_t, [C.c_int]),
    "cvs_curves_pack": (C.c_int, [_f32p, _f32p, C.c_int]),
    "cvs_primary_f16_dev": (C.c_int, [_F16, _F16, P(primary_params), _vp, _vp, _vp]),
    "cvs_primary_f32_dev": (C.c_int, [_F32, _F32, P(primary_params), _vp, _vp, _vp]),
}

# the same for include/canvas_secondary.h (secondaries: the HSL qualifier and the mix through a matte)
SECONDARY_SIGNATURES = {
    "cvs_qualify_f16_dev": (C.c_int, [_F16, _F16, _F16, P(qualifier_params), _vp]),
    "cvs_qualify_f32_dev": (C.c_int, [_F32, _F32, _F32, P(qualifier_params), _vp]),
    "cvs_matte_mix_f16_dev": (C.c_int, [_F16, _F16, _F16, _F16, P(matte_mix_params), _vp]),
    "cvs_matte_mix_f32_dev": (C.c_int, [_F32, _F32, _F32, _F32, P(matte_mix_params), _vp]),
}

# the same for include/canvas_perspective.h (corner pin)
PERSPECTIVE_SIGNATURES = {
    "cvs_perspective_f32_dev": (C.c_int, [_F32, _F32, P(perspective_params), _vp]),
    "cvs_perspective_f16_dev": (C.c_int, [_F16, _F16, P(perspective_params), _vp]),
    "cvs_perspective_from_quad": (C.c_int, [P(C.c_double), P(C.c_double * 2), C.c_int, P(perspective_params)]),
    "cvs_perspective_target_window": (C.c_int, [P(perspective_params), P(box2i), P(box2i), P(box2i)]),
    "cvs_perspective_source_window": (C.c_int, [P(perspective_params), P(box2i), P(box2i)]),
}

# the same for include/canvas_deinterlace.h (motion-adaptive deinterlace)
DEINTERLACE_SIGNATURES = {
    "cvs_deinterlace_adaptive_f16_dev": (C.c_int, [_F16, _F16, _F16, _F16, P(deinterlace_params), _vp]),
}

# the same for include/canvas_median.h (3 x 3 / 5 x 5 median)
MEDIAN_SIGNATURES = {
    "cvs_median_f16_dev": (C.c_int, [_F16, _F16, P(median_params), _vp]),
    "cvs_median_f32_dev": (C.c_int, [_F32, _F32, P(median_params), _vp]),
}

# the same for include/canvas_temporal.h (motion-adaptive temporal denoise): out, prev2, prev1, cur, next1, next2
TEMPORAL_SIGNATURES = {
    "cvs_temporal_denoise_f16_dev": (C.c_int, [_F16, _F16, _F16, _F16, _F16, _F16, P(temporal_params), _vp]),
}

# the same for include/canvas_ycc422.h (4:2:2 Y'CbCr edges): width, height, layout, flags (0 or YCC_REC709)
YCC422_PLANAR8, YCC422_PLANAR10, YCC422_UYVY, YCC422_V210 = 0, 1, 2, 3
YCC422_SIGNATURES = {
    "cvs_ycc422_layout": (C.c_int, [C.c_int, C.c_int, C.c_int, P(C.c_int), P(C.c_int)]),
    "cvs_reconstruct_422_dev": (C.c_int, [_F16, P(coded_image), C.c_int, C.c_int, C.c_int, C.c_int, _vp]),
    "cvs_subsample_422_dev": (C.c_int, [P(coded_image), _F16, C.c_int, C.c_int, C.c_int, C.c_int, _vp]),
}

# the same for include/canvas_ycc420.h (4:2:0 Y'CbCr edges): width, height, layout, flags (YCC_REC709 and the bits below)
YCC420_PLANAR8, YCC420_PLANAR10, YCC420_NV12, YCC420_P010 = 0, 1, 2, 3
YCC_REC2020, YCC_FULL_RANGE, YCC_SITING_CENTER, YCC_SITING_TOPLEFT, YCC_NO_TRANSFER = 4, 8, 16, 32, 64
YCC420_SIGNATURES = {
    "cvs_ycc420_layout": (C.c_int, [C.c_int, C.c_int, C.c_int, P(C.c_int), P(C.c_int)]),
    "cvs_reconstruct_420_dev": (C.c_int, [_F16, P(coded_image), C.c_int, C.c_int, C.c_int, C.c_int, _vp]),
    "cvs_subsample_420_dev": (C.c_int, [P(coded_image), _F16, C.c_int, C.c_int, C.c_int, C.c_int, _vp]),
}

# the five function-pointer globals of half.c:87-91
HALF_POINTER_GLOBALS = {
    "half_convert_to_float": C.CFUNCTYPE(None, _f32p, _u16p, C.c_int),
    "half_convert_from_float": C.CFUNCTYPE(None, _u16p, _f32p, C.c_int),
    "half_convert_to_float_fast": C.CFUNCTYPE(None, _f32p, _u16p, C.c_int),
    "half_convert_from_float_fast": C.CFUNCTYPE(None, _u16p, _f32p, C.c_int),
    "half_lookup": C.CFUNCTYPE(None, _u16p, _u16p, _u16p, C.c_int),
}

_lib = None


class LibraryMissing(RuntimeError):
    pass


def load():
    """Load and bind the shared library.  Raises LibraryMissing when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise LibraryMissing(
            "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or make -C canvas_amd/csrc).  There is no CPU fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in list(SIGNATURES.items()) + list(SCOPE_SIGNATURES.items()) + list(LUT3D_SIGNATURES.items()) + list(PERSPECTIVE_SIGNATURES.items()) + list(DEINTERLACE_SIGNATURES.items()) + list(MEDIAN_SIGNATURES.items()) + list(TEMPORAL_SIGNATURES.items()) + list(YCC422_SIGNATURES.items()) + list(YCC420_SIGNATURES.items()) + list(PRIMARY_SIGNATURES.items()) + list(SECONDARY_SIGNATURES.items()):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    _lib = lib
    return lib


def half_pointer(name):
    """Read one of the half.c function-pointer globals (NULL before init_half())."""
    lib = load()
    addr = C.c_void_p.in_dll(lib, name).value
    return HALF_POINTER_GLOBALS[name](addr) if addr else None


def last_error():
    return load().cvs_last_error().decode()


def check(rc, what="call"):
    if rc != 0:
        raise RuntimeError("%s failed (%d): %s" % (what, rc, last_error()))
