"""Seeded cases shared by the tests that pin the oracle and the kernels to a build of the reference's own code:
tests/test_oracle_against_reference.py (oracle against reference, CPU), tests/golden/make_reference_golden.py (records the
reference's results) and tests/test_reference_fixtures_gpu.py (library against the recordings, no oracle in between).

An "implementation" is anything with the reference's ABI: RefAbi wraps a library exporting the reference's own symbol names
(the reference builds of oracle/ref_build.py, and libcanvas_hip.so's host-frame entry points), OrcAbi the oracle's
restatement.  Every case returns {name: (codes, window)}: codes are the canonical bit patterns (tests/util.py canon_f16 /
canon_f32, nothing else folded) of the WHOLE target buffer, window the reported current_window or None.
"""
import ctypes as C
import hashlib

import numpy as np

from canvas_amd.abi import HostFrame, box2i, fir_filter, v2f, video_source
from tests.util import canon_f16, canon_f32

ALL_CODES = np.arange(65536, dtype=np.uint16)
TRANSFER_NAMES = ["video_transfer_rec709_to_linear_scene", "video_transfer_rec709_to_linear_display",
                  "video_transfer_linear_to_rec709", "video_transfer_linear_to_sRGB"]
MIXES = (1.0, 0.3, 0.0, 1.7)
SENTINEL_F32 = np.float32(-77.25)
SENTINEL_F16 = 0xD4D4

# the 13 configurations of test_gpu_parity.MIX_WINDOWS (frames of 24 x 12), and the same on frames of 51 x 26
MIX_FULL = (0, 0, 23, 11)
MIX_WINDOWS = [
    (MIX_FULL, MIX_FULL), (MIX_FULL, (3, 2, 10, 6)), ((3, 2, 10, 6), MIX_FULL), (MIX_FULL, (0, 0, -1, -1)),
    ((0, 0, -1, -1), (2, 1, 9, 7)), ((0, 0, 11, 11), (0, 0, 23, 11)), ((1, 1, 6, 3), (1, 5, 6, 8)), ((1, 1, 6, 3), (9, 1, 14, 3)),
    ((1, 1, 6, 3), (9, 6, 14, 9)), ((2, 1, 12, 7), (6, 4, 20, 10)), ((6, 4, 20, 10), (2, 1, 12, 7)), ((0, 5, 12, 9), (5, 0, 20, 7)),
    ((4, 0, 9, 11), (0, 3, 23, 8)),
]
BIG_FULL = (0, 0, 50, 25)


def _grow(w):
    if w[2] < w[0] or w[3] < w[1]:
        return w
    return (round(w[0] * 50 / 23), round(w[1] * 25 / 11), round(w[2] * 50 / 23), round(w[3] * 25 / 11))


BIG_WINDOWS = [(_grow(p), _grow(q)) for p, q in MIX_WINDOWS]

COPY_WINDOWS = [      # out.full, in.full, in.current (test_gpu_parity.WINDOW_CASES)
    ((0, 0, 15, 8), (0, 0, 15, 8), (0, 0, 15, 8)), ((0, 0, 15, 8), (0, 0, 15, 8), (3, 2, 10, 6)),
    ((-1, -1, 1, 1), (0, 0, 3, 3), (0, 0, 2, 2)), ((0, 0, 15, 8), (-4, -4, 20, 12), (-2, -3, 18, 11)),
    ((0, 0, 15, 8), (0, 0, 15, 8), (0, 0, -1, -1)), ((0, 0, 15, 8), (20, 20, 30, 30), (21, 21, 29, 29)),
]
TAP_GRID = [(s, o) for s in (0.25, 0.5, 0.75, 1.0, 2.0, 3.5, 4.0) for o in (0.0, 0.25, 0.5, 0.999)]   # test_fir_taps
SCALE_FACTORS = [(0.5, 0.5), (1.7, 0.6), (2.0, 3.0)]
WIDE_TARGET = (1100, 37, (2.0, 2.0))          # test_scale_wide_targets_two_columns_per_lane: f32, the tiles


def digest(codes, window=None):
    h = hashlib.sha256(np.ascontiguousarray(codes).tobytes())
    if window is not None:
        h.update(repr(tuple(int(v) for v in window)).encode())
    return h.hexdigest()


def win_of(frame):
    """The reported window; every empty box is the same box (only emptiness is contractual)."""
    w = frame.current_window
    return (0, 0, -1, -1) if w.is_empty() else w.tuple()


# ------------------------------------------------------------------------------------------------ inputs

def lively_f32(rng, full, win):
    """Values inside and outside [0, 1], alpha exactly 0 and exactly 1 on a fifth of the pixels each, and a sprinkle of
    NaN, +-Inf and denormals."""
    fw = box2i.of(*full)
    a = rng.uniform(-0.5, 1.5, (fw.height, fw.width, 4)).astype(np.float32)
    al = rng.uniform(0, 1, a.shape[:2]).astype(np.float32)
    al[rng.uniform(size=al.shape) < 0.2] = 0
    al[rng.uniform(size=al.shape) < 0.2] = 1
    a[..., 3] = al
    flat = a.reshape(-1)
    wild = np.array([np.nan, np.inf, -np.inf, 1e-40, -1e-41, 1.4e-45, 3e38, -3e38], np.float32)
    idx = rng.choice(flat.size, max(8, flat.size // 40), replace=False)
    flat[idx] = wild[rng.integers(0, len(wild), idx.size)]
    return HostFrame(full, np.float32, a, win)


def lively_f16(rng, full, win):
    fw = box2i.of(*full)
    # finite halfs of both signs up to 4.0, plus every kind of special code
    codes = rng.integers(0, 0x4400, (fw.height, fw.width, 4)).astype(np.uint16)
    codes[rng.uniform(size=codes.shape) < 0.25] |= 0x8000
    flat = codes.reshape(-1)
    wild = np.array([0x7C00, 0xFC00, 0x7E00, 0x0001, 0x8001, 0x03FF, 0x7BFF, 0xFBFF, 0x8000], np.uint16)
    idx = rng.choice(flat.size, max(8, flat.size // 40), replace=False)
    flat[idx] = wild[rng.integers(0, len(wild), idx.size)]
    return HostFrame(full, np.uint16, codes, win)


def f2h_probes(h2f):
    """The probe set of test_gpu_parity.test_f2h_probe_set (`h2f`: any correct half_to_float), every exponent class of
    both signs included; NaN inputs are left out there and here."""
    rng = np.random.default_rng(7)
    probes = [
        rng.uniform(-4, 4, 300001).astype(np.float32),
        rng.uniform(-70000, 70000, 50000).astype(np.float32),
        (rng.uniform(-1, 1, 50000) * 2.0 ** rng.integers(-30, -10, 50000)).astype(np.float32),
        h2f(ALL_CODES[(ALL_CODES & 0x7C00) != 0x7C00]),
        np.array([0.0, -0.0, 65504.0, 65519.9, 65520.0, 65535.9, 65536.0, -65536.0, 1e30, -1e30, np.inf, -np.inf,
                  2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -24, 2.0 ** -14, 2.0 ** -14 * (1 - 2.0 ** -11), 1e-45, -1e-45], np.float32),
    ]
    bits = rng.integers(0, 2 ** 32, 400000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    probes.append(bits[~np.isnan(bits)])
    # every exponent class: 256 exponents x 2 signs x (lowest, a middle, highest mantissa), NaNs dropped
    e = (np.arange(512, dtype=np.uint32) << 23)[:, None] | np.array([0, 0x2AAAAA, 0x7FFFFF], np.uint32)[None, :]
    cls = e.reshape(-1).view(np.float32)
    probes.append(cls[~np.isnan(cls)])
    return probes


def scaler_setups(rng):
    """The 66 set-ups of test_oracle_pins.test_triangle_scaler_matches_model: (target full, source full, source current,
    target point, source point, factors).  Draws from `rng` exactly as that test always has."""
    cases = [((0, 0, 31, 17), (0, 0, 15, 8), (0, 0, 15, 8), (0, 0), (0, 0), (2.0, 2.0)),
             ((0, 0, 15, 8), (0, 0, 31, 17), (0, 0, 31, 17), (0, 0), (0, 0), (0.5, 0.5)),
             ((0, 0, 40, 30), (0, 0, 15, 8), (0, 0, 15, 8), (3.5, 2.25), (1.0, 0.5), (2.5, 3.0)),
             ((0, 0, 20, 40), (0, 0, 15, 8), (0, 0, 15, 8), (0, 0), (0, 0), (1.3, 4.0)),
             ((0, 0, 15, 8), (0, 0, 15, 8), (0, 0, 15, 8), (2.0, 0.0), (0, 0), (1.0, 1.0)),
             ((-8, -4, 23, 13), (0, 0, 15, 8), (0, 0, 15, 8), (0, 0), (8.0, 4.0), (2.0, 2.0))]
    for _ in range(60):
        sfull = (int(rng.integers(-4, 3)), int(rng.integers(-3, 3)), int(rng.integers(8, 22)), int(rng.integers(5, 14)))
        tfull = (int(rng.integers(-4, 3)), int(rng.integers(-3, 3)), int(rng.integers(8, 30)), int(rng.integers(5, 22)))
        ax, bx = sorted(int(v) for v in rng.integers(sfull[0], sfull[2] + 1, 2))
        ay, by = sorted(int(v) for v in rng.integers(sfull[1], sfull[3] + 1, 2))
        fac = (float(rng.choice([0.25, 0.5, 0.75, 1.0, 1.5, 2.0, 3.0])), float(rng.choice([0.25, 0.5, 0.8, 1.0, 1.25, 2.0, 4.0])))
        tp = (float(rng.choice([0.0, 0.5, 2.25])), float(rng.choice([0.0, 1.0, 3.5])))
        sp = (float(rng.choice([0.0, 0.75, 2.0])), float(rng.choice([0.0, 0.5, 1.0])))
        cases.append((tfull, sfull, (ax, ay, bx, by), tp, sp, fac))
    return cases


def scale_defined_in_reference(ref, tfull, sfull, scur, tp, sp, fac):
    """False for the one shape of call the reference leaves undefined.  With x resampled first (video_scale.c:252-268), a
    horizontal pass that reaches no source pixel leaves the intermediate window at (INT_MAX .. INT_MIN) (:140,:191,:225);
    the vertical pass then computes `xmax - xmin + 1` on it (:38-39,:81), a signed overflow, and reads through the result
    (observed: a segmentation fault).  The oracle and the library define that call as an empty window; the reference
    defines nothing to compare with.  Decided by the reference itself: its own horizontal-only pass (a defined,
    single-pass call) into the same intermediate window, run on a zero source of the same geometry."""
    if not (fac[0] < fac[1]) or (fac[0] == 1.0 and tp[0] == sp[0]) or (fac[1] == 1.0 and tp[1] == sp[1]):
        return True
    f32 = np.float32
    x0 = int(f32(sp[0]) - (f32(tp[0]) - f32(tfull[0])) * f32(fac[0]))
    x1 = int(f32(sp[0]) + (f32(tfull[2]) - f32(tp[0])) * f32(fac[0]))
    mid = (max(x0, tfull[0]), max(scur[1], tfull[1]), min(x1, tfull[2]), min(scur[3], tfull[3]))
    if mid[2] < mid[0] or mid[3] < mid[1]:
        return False
    src = HostFrame(sfull, np.float32, None, scur)
    out = HostFrame(mid, np.float32)
    ref.scale(out, (tp[0], 0.0), src, (sp[0], 0.0), (fac[0], 1.0))
    return not out.current_window.is_empty()


def dv_planes():
    rng = np.random.default_rng(304)
    return [np.ascontiguousarray(rng.integers(0, 256, (480, s), dtype=np.uint8)) for s in (720, 180, 180)]


def dv_frame():
    """Linear-light halfs in [0, 1]: every coded value lands inside a byte (a float beyond it has no defined conversion in C)."""
    rng = np.random.default_rng(305)
    return HostFrame((0, -1, 719, 478), np.uint16, rng.integers(0, 0x3C01, (480, 720, 4)).astype(np.uint16))


def workspace_layers(full=(0, 0, 63, 35)):
    """Three solid items, translucent ones above an opaque one; z-order differs from insertion order.
    Every upper window starts below line 0: video_mix.c:265 compares out's min.x with the upper frame's min.Y, and where
    that picks the upper frame as `left` the reference copies pixels its scratch frame never received.
    -> [(colour, window, z)]"""
    return [((0.25, 0.5, 0.75, 1.0), full, 0), ((0.9, 0.1, 0.3, 0.35), (10, 4, 50, 30), 7), ((0.2, 1.3, -0.1, 0.6), (30, 1, 63, 20), 3)]


def solid_source(color, window, keep):
    """A video_source with an f32 slot only, painting `color` into `window` clipped by the frame (SolidColorVideoSource)."""
    from canvas_amd.abi import GET_FRAME_F16, GET_FRAME_F32, video_frame_source_funcs

    def g32(self, idx, fp):
        f = fp.contents
        fw = f.full_window
        x0, y0 = max(window[0], fw.min.x), max(window[1], fw.min.y)
        x1, y1 = min(window[2], fw.max.x), min(window[3], fw.max.y)
        dst = np.ctypeslib.as_array(C.cast(f.data, C.POINTER(C.c_float)), shape=(fw.height, fw.width, 4))
        dst[y0 - fw.min.y: y1 - fw.min.y + 1, x0 - fw.min.x: x1 - fw.min.x + 1] = np.array(color, np.float32)
        f.current_window = box2i.of(x0, y0, x1, y1)

    cb32 = GET_FRAME_F32(g32)
    funcs = video_frame_source_funcs(0, C.cast(None, GET_FRAME_F16), cb32, None)
    src = video_source(None, C.pointer(funcs))
    keep += [cb32, funcs, src]
    return src


# ------------------------------------------------------------------------------------------------ implementations

def _u16(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint16))


def _f32(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


class RefAbi:
    """A library that exports the reference's own symbols.  `half`: name -> callable for the five pointer globals."""

    def __init__(self, lib, half, coded_image, free_image):
        self.lib, self.half, self.coded_image, self.free_image = lib, half, coded_image, free_image

    def h2f(self, codes, fast=False):
        out = np.empty(codes.shape, np.float32)
        self.half("half_convert_to_float_fast" if fast else "half_convert_to_float")(_f32(out), _u16(codes), codes.size)
        return out

    def f2h(self, values, fast=False):
        values = np.ascontiguousarray(values, np.float32)
        out = np.empty(values.shape, np.uint16)
        self.half("half_convert_from_float_fast" if fast else "half_convert_from_float")(_u16(out), _f32(values), values.size)
        return out

    def table(self, which):
        out = np.empty(65536, np.uint16)
        getattr(self.lib, TRANSFER_NAMES[which])(_u16(out), _u16(ALL_CODES), 65536)
        return out

    def ramp(self):
        return np.ctypeslib.as_array(self.lib.video_get_gamma45_ramp(), shape=(65536,)).copy()

    def _taps(self, fn, *args):
        f = fir_filter(None, 0, 0)
        fn(*args, C.byref(f))
        res = (np.ctypeslib.as_array(f.coeff, shape=(f.width,)).copy(), f.width, f.center)
        self.lib.filter_free(C.byref(f))
        return res

    def triangle(self, sub, offset):
        return self._taps(self.lib.filter_createTriangle, C.c_float(sub), C.c_float(offset))

    def lanczos(self, sub, size, offset):
        return self._taps(self.lib.filter_createLanczos, C.c_float(sub), size, C.c_float(offset))

    def copy_f16(self, out, src):
        self.lib.video_copy_frame_f16(out.ref(), src.ref())

    def copy_alpha(self, out, src, alpha):
        self.lib.video_copy_frame_alpha_f32(out.ref(), src.ref(), C.c_float(alpha))

    def over(self, out, b, mix):
        self.lib.video_mix_over_f32(out.ref(), b.ref(), C.c_float(mix))

    def cross(self, out, a, b, mix):
        self.lib.video_mix_cross_f32(out.ref(), a.ref(), b.ref(), C.c_float(mix))

    def scale(self, target, tp, source, sp, fac):
        self.lib.video_scale_bilinear_f32(target.ref(), v2f(*tp), source.ref(), v2f(*sp), v2f(*fac))

    def to_xyz(self, frame):
        self.lib.video_color_rgb_to_xyz_sdtv(frame.ref())

    def to_srgb(self, frame):
        self.lib.video_color_xyz_to_srgb(frame.ref())

    def reconstruct_dv(self, frame, planes):
        img = self.coded_image()
        for i, p in enumerate(planes):
            img.data[i], img.stride[i], img.line_count[i] = p.ctypes.data, p.shape[1], p.shape[0]
        self.lib.video_reconstruct_dv(frame.ref(), C.byref(img))

    def subsample_dv(self, frame):
        img = self.lib.video_subsample_dv(frame.ref())
        c = img.contents
        planes = [np.ctypeslib.as_array(C.cast(c.data[i], C.POINTER(C.c_uint8)), shape=(c.line_count[i], c.stride[i])).copy()
                  for i in range(3)]
        self.free_image(img)
        return planes

    def workspace(self, layers, frame_index, out):
        keep = []
        ws = self.lib.workspace_create()
        for color, window, z in layers:
            s = solid_source(color, window, keep)
            self.lib.workspace_add_item(ws, C.cast(C.pointer(s), C.c_void_p), 0, 10, 0, z, None)
        vs = video_source()
        self.lib.workspace_as_video_source(ws, C.byref(vs))
        self.lib.video_get_frame_f32(C.byref(vs), frame_index, out.ref())
        self.lib.workspace_free(ws)


class OrcAbi:
    """The oracle's restatement (the build that `orc.lib()` currently answers with: see oracle.flavour)."""

    def __init__(self, orc):
        self.orc = orc

    def h2f(self, codes, fast=False):
        out = np.empty(codes.shape, np.float32)
        fn = self.orc.lib().orc_half_to_float_fast if fast else self.orc.lib().orc_half_to_float
        fn(_f32(out), _u16(codes), codes.size)
        return out

    def f2h(self, values, fast=False):
        values = np.ascontiguousarray(values, np.float32)
        out = np.empty(values.shape, np.uint16)
        fn = self.orc.lib().orc_float_to_half_fast if fast else self.orc.lib().orc_float_to_half
        fn(_u16(out), _f32(values), values.size)
        return out

    def table(self, which):
        return self.orc.transfer_table(which)

    def ramp(self):
        return self.orc.gamma45_ramp()

    def triangle(self, sub, offset):
        t, c = self.orc.fir_triangle(sub, offset)
        return t, len(t), c

    def lanczos(self, sub, size, offset):
        t, c = self.orc.fir_lanczos(sub, size, offset)
        return t, len(t), c

    def copy_f16(self, out, src):
        self.orc.lib().orc_copy_frame_f16(out.ref(), src.ref())

    def copy_alpha(self, out, src, alpha):
        self.orc.lib().orc_copy_frame_alpha_f32(out.ref(), src.ref(), C.c_float(alpha))

    def over(self, out, b, mix):
        self.orc.lib().orc_mix_over_f32(out.ref(), b.ref(), C.c_float(mix))

    def cross(self, out, a, b, mix):
        self.orc.lib().orc_mix_cross_f32(out.ref(), a.ref(), b.ref(), C.c_float(mix))

    def scale(self, target, tp, source, sp, fac):
        self.orc.lib().orc_scale_bilinear_f32(target.ref(), v2f(*tp), source.ref(), v2f(*sp), v2f(*fac))

    def to_xyz(self, frame):
        self.orc.lib().orc_color_rgb_to_xyz_sdtv(frame.ref())

    def to_srgb(self, frame):
        self.orc.lib().orc_color_xyz_to_srgb(frame.ref())

    def reconstruct_dv(self, frame, planes):
        self.orc.lib().orc_reconstruct_dv(frame.ref(), (C.c_void_p * 3)(*[p.ctypes.data for p in planes]),
                                          (C.c_int * 3)(*[p.shape[1] for p in planes]))

    def subsample_dv(self, frame):
        back = [np.zeros((480, s), np.uint8) for s in (720, 180, 180)]
        self.orc.lib().orc_subsample_dv((C.c_void_p * 3)(*[p.ctypes.data for p in back]), (C.c_int * 3)(720, 180, 180), frame.ref())
        return back

    def workspace(self, layers, frame_index, out):
        keep = []
        srcs = [solid_source(color, window, keep) for color, window, _ in layers]
        items = (self.orc.ws_item * len(layers))(*[self.orc.ws_item(0, 10, z, 0, C.pointer(s)) for s, (_, _, z) in zip(srcs, layers)])
        self.orc.lib().orc_workspace_get_frame_f32(items, len(layers), frame_index, out.ref())


def ref_abi(lib):
    """RefAbi over one of oracle.ref()'s libraries."""
    import oracle
    return RefAbi(lib, lambda name: getattr(lib, name), oracle.coded_image, oracle.free_coded_image)


# ------------------------------------------------------------------------------------------------ the recorded cases

def over_case(impl, i, mix, windows=BIG_WINDOWS, full=BIG_FULL):
    pw, qw = windows[i]
    rng = np.random.default_rng(1000 + i)
    out, upper = lively_f32(rng, full, pw), lively_f32(rng, full, qw)
    before = upper.array.copy()
    impl.over(out, upper, mix)
    assert np.array_equal(before.view(np.uint32), upper.array.view(np.uint32)), "over wrote its input"
    return canon_f32(out.array), win_of(out)


def cross_case(impl, i, mix, windows=BIG_WINDOWS, full=BIG_FULL):
    pw, qw = windows[i]
    rng = np.random.default_rng(2000 + i)
    a, b = lively_f32(rng, full, pw), lively_f32(rng, full, qw)
    out = HostFrame(full, np.float32, fill=SENTINEL_F32)
    ba, bb = a.array.copy(), b.array.copy()
    impl.cross(out, a, b, mix)
    assert np.array_equal(ba.view(np.uint32), a.array.view(np.uint32)) and np.array_equal(bb.view(np.uint32), b.array.view(np.uint32))
    return canon_f32(out.array), win_of(out)


def scale_source():
    rng = np.random.default_rng(4242)
    src = rng.uniform(-0.5, 1.5, (36, 64, 4)).astype(np.float32)
    return HostFrame((0, 0, 63, 35), np.float32, src, (1, 0, 62, 34))          # inset: odd left edge, ragged bottom


def scale_case(impl, fac):
    src = scale_source()
    before = src.array.copy()
    out = HostFrame((0, 0, 99, 79), np.float32, fill=SENTINEL_F32)
    impl.scale(out, (0.5, 0.25), src, (1.0, 0.0), fac)
    assert np.array_equal(before, src.array)
    return canon_f32(out.array), win_of(out)


def scale_source_f16():
    from canvas_amd.synth import truncate_to_half
    s = scale_source()
    return HostFrame(s.full_window, np.uint16, truncate_to_half(s.array), s.current_window)


def scale_case_f16(impl, fac):
    """What the f16 twin is defined as: widen -> video_scale_bilinear_f32 -> truncate, the whole target: the scaler zero-fills
    all of it before it accumulates (video_scale.c:25-32,44,142), so nothing of a sentinel survives."""
    s16 = scale_source_f16()
    src = HostFrame(s16.full_window, np.float32, impl.h2f(s16.array), s16.current_window)
    mid = HostFrame((0, 0, 99, 79), np.float32, fill=SENTINEL_F32)
    impl.scale(mid, (0.5, 0.25), src, (1.0, 0.0), fac)
    out = HostFrame((0, 0, 99, 79), np.uint16, impl.f2h(mid.array), mid.current_window)
    return canon_f16(out.array), win_of(out)


def wide_source():
    tw, th, fac = WIDE_TARGET
    sw, sh = int(tw / fac[0]) + 2, int(th / fac[1]) + 2
    rng = np.random.default_rng(4100 + tw)
    return HostFrame((0, 0, sw - 1, sh - 1), np.float32, rng.uniform(-0.5, 1.5, (sh, sw, 4)).astype(np.float32))


def wide_case(impl):
    tw, th, fac = WIDE_TARGET
    out = HostFrame((0, 0, tw - 1, th - 1), np.float32, fill=SENTINEL_F32)
    impl.scale(out, (0, 0), wide_source(), (0, 0), fac)
    return canon_f32(out.array), win_of(out)


COLOUR_FULL, COLOUR_WINDOW = (0, 0, 32, 19), (3, 1, 29, 17)          # 33 x 20, odd left edge, inset


def colour_case(impl, which):
    rng = np.random.default_rng(5150)
    f = lively_f16(rng, COLOUR_FULL, COLOUR_WINDOW)
    (impl.to_xyz if which == "xyz" else impl.to_srgb)(f)
    return canon_f16(f.array), win_of(f)


def workspace_case(impl):
    out = HostFrame((0, 0, 63, 35), np.float32, fill=SENTINEL_F32)
    impl.workspace(workspace_layers(), 4, out)
    return canon_f32(out.array), win_of(out)


def taps_cases(impl):
    res = {}
    for sub, off in TAP_GRID:
        for kind, t in (("tri", impl.triangle(sub, off)), ("lan", impl.lanczos(sub, 3, off))):
            res["taps/%s/%g/%g" % (kind, sub, off)] = (t[0].view(np.uint32).copy(), (t[1], t[2]))
    return res


def dv_cases(impl):
    frame = HostFrame((0, -1, 719, 478), np.uint16, fill=SENTINEL_F16)
    impl.reconstruct_dv(frame, dv_planes())
    src = dv_frame()
    planes = impl.subsample_dv(src)
    return {"dv/reconstruct": (canon_f16(frame.array), win_of(frame)),
            "dv/subsample": (np.concatenate([p.reshape(-1) for p in planes]), None),
            "dv/subsample_input_after": (canon_f16(src.array), None)}         # the reference encodes its input in place


def domain_digests(impl):
    """SHA-256 over whole-domain results: h2f on every code, the four tables, the ramp (where the conversion to a byte is
    defined: non-negative, not NaN), f2h and the _fast pair on their probe sets."""
    d = {"h2f": digest(canon_f32(impl.h2f(ALL_CODES)))}
    for which in range(4):
        d["table%d" % which] = digest(canon_f16(impl.table(which)))
    ok = ((ALL_CODES & 0x7FFF) <= 0x7C00) & (ALL_CODES < 0x8000)
    d["ramp"] = digest(impl.ramp()[ok])
    h2f = impl.h2f
    d["f2h"] = digest(np.concatenate([impl.f2h(p) for p in f2h_probes(h2f)]))
    normal = ALL_CODES[((ALL_CODES >> 10) & 0x1F != 0) & ((ALL_CODES >> 10) & 0x1F != 31)]
    fast = impl.h2f(normal, fast=True)
    d["h2f_fast"] = digest(fast.view(np.uint32))
    d["f2h_fast"] = digest(impl.f2h(fast, fast=True))
    return d


def small_cases(impl):
    """Every small-frame case of the GPU module: {name: (codes, window)}."""
    res = {}
    for i in range(len(BIG_WINDOWS)):
        for mix in MIXES:
            res["over/%d/%g" % (i, mix)] = over_case(impl, i, mix)
            res["cross/%d/%g" % (i, mix)] = cross_case(impl, i, mix)
    for fac in SCALE_FACTORS:
        res["scale/f32/%g,%g" % fac] = scale_case(impl, fac)
        res["scale/f16/%g,%g" % fac] = scale_case_f16(impl, fac)
    res["scale/wide"] = wide_case(impl)
    res["colour/xyz"] = colour_case(impl, "xyz")
    res["colour/srgb"] = colour_case(impl, "srgb")
    res["workspace"] = workspace_case(impl)
    res.update(taps_cases(impl))
    res.update(dv_cases(impl))
    return res


# ------------------------------------------------------------------------------------------------ the recordings

def load_fixture():
    """tests/golden/reference_built.npz (tests/golden/make_reference_golden.py) -> {flavour: (index, {name: codes})}."""
    import json
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_built.npz"))
    res = {}
    for flavour in ("gcc", "fma"):
        raw = {k[len(flavour) + 1:-len("/codes")]: z[k] for k in z.files if k.startswith(flavour + "/") and k.endswith("/codes")}
        res[flavour] = (json.loads(str(z[flavour + "/index"])), raw)
    return res


def assert_matches_recording(fixture, name, got, what="library"):
    """`got` = (canonical codes of the whole buffer, window) against the recording of one flavour."""
    index, raw = fixture
    codes, win = got
    want = index["cases"][name]
    assert (None if win is None else [int(v) for v in win]) == want["win"], "%s: %s reports %r, the reference %r" % (name, what, win, want["win"])
    if name in raw:
        ref = raw[name]
        assert ref.shape == codes.shape and ref.dtype == codes.dtype, (name, ref.shape, codes.shape)
        if not np.array_equal(ref, codes):
            bad = np.argwhere(ref != codes)
            i = tuple(bad[0])
            raise AssertionError("%s: %d of %d codes differ from the reference; first at %s: %s 0x%x, reference 0x%x"
                                 % (name, len(bad), ref.size, i, what, codes[i], ref[i]))
    assert digest(codes, win) == want["sha"], "%s: the %s's whole buffer is not the reference's (SHA-256 of the canonical codes)" % (name, what)
