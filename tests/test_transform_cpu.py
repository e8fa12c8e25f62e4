"""VideoTransformFilter without a GPU: the five C symbols are declared, exported and mirrored, the ctypes struct has the C struct's
layout; every refusal of the contract (DESIGN.md "Affine transform") comes back as -1 with a message naming the entry and an
empty window before anything is launched; cvs_transform_from_parts and the two window helpers against the float64 formulas of
the numpy model (tests/transform_model.py); the windows are safe by brute force over the model; self-checks of the model the GPU
tests hold the kernel to; the built code object holds the four k_transform instances without scratch memory and passes the
load-in-flight check; the node's surface; a pull without a device or without a source ends with an empty window."""
import ctypes as C
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from tests import transform_model as tm
from tests.models import f2h_rz_model
from tests.test_unsharp_cpu import _kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("cvs_transform_f32_dev", "cvs_transform_f16_dev")
HELPERS = ("cvs_transform_from_parts", "cvs_transform_target_window", "cvs_transform_source_window")
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
EVERYWHERE = (-(1 << 29), -(1 << 29), 1 << 29, 1 << 29)
FILTERS = (tm.NEAREST, tm.BILINEAR)


@pytest.fixture(scope="module")
def process():
    from fluggo.media import process
    return process


@pytest.fixture(scope="module")
def lib():
    from canvas_amd import _lib
    return _lib.load()


def _box(t):
    from canvas_amd.abi import box2i
    return box2i.empty() if t is None else box2i.of(*t)


def _tuple(b):
    return None if b.is_empty() else b.tuple()


def _from_parts(lib, anchor, scale, rotation, position, m=None):
    pair = C.c_double * 2
    m = (C.c_float * 6)(*([7.0] * 6)) if m is None else m
    rc = lib.cvs_transform_from_parts(pair(*anchor), pair(*scale), rotation, pair(*position), m)
    return rc, tuple(m)


def _target_window(lib, m, filt, S, tfull):
    from canvas_amd import _lib
    win = _box((5, 5, 6, 6))
    rc = lib.cvs_transform_target_window(C.byref(_lib.transform(m, filt)), C.byref(_box(S)), C.byref(_box(tfull)), C.byref(win))
    return rc, _tuple(win)


def _source_window(lib, m, filt, window):
    from canvas_amd import _lib
    need = _box((5, 5, 6, 6))
    rc = lib.cvs_transform_source_window(C.byref(_lib.transform(m, filt)), C.byref(_box(window)), C.byref(need))
    return rc, _tuple(need)


def _transforms(seed, count, reach):
    """Seeded general transforms: (S, parts, m).  S up to 10 x 10 somewhere within +-reach, rotations of any angle, scales e^+-2 of
    either sign, the anchor inside S, the layer put anywhere within +-reach."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        w, h = (int(v) for v in rng.integers(1, 11, 2))
        x0, y0 = (int(v) for v in rng.integers(-reach, reach - 10, 2))
        S = (x0, y0, x0 + w - 1, y0 + h - 1)
        parts = dict(anchor=(x0 + float(rng.uniform(0, w)), y0 + float(rng.uniform(0, h))),
                     scale=tuple(float(v) for v in np.exp(rng.uniform(-2, 2, 2)) * rng.choice([-1.0, 1.0], 2)),
                     rotation=float(rng.uniform(-360, 360)) if len(out) % 5 else float(rng.integers(-8, 9) * 45),
                     position=tuple(float(v) for v in rng.uniform(-reach + 200, reach - 200, 2)))
        out.append((S, parts, tm.from_parts(**parts)))
    return out


# ---------------------------------------------------------------- the C surface

def test_symbols_declared_exported_and_mirrored():
    header = open(os.path.join(ROOT, "include", "canvas_hip.h")).read()
    for fmt in ("f32", "f16"):
        decl = (r"CVS_EXPORT int cvs_transform_%s_dev\(rgba_frame_%s \*target, const rgba_frame_%s \*source, const cvs_transform \*t, cvs_stream_t s\);"
                % (fmt, fmt, fmt))
        assert re.search(decl, header), decl
    assert "CVS_EXPORT int cvs_transform_from_parts(const double anchor[2], const double scale[2], double rotation_degrees, const double position[2], float m[6]);" in header
    assert "CVS_EXPORT int cvs_transform_target_window(const cvs_transform *t, const box2i *source_current, const box2i *target_full, box2i *win);" in header
    assert "CVS_EXPORT int cvs_transform_source_window(const cvs_transform *t, const box2i *target_window, box2i *need);" in header
    assert "enum { CVS_TRANSFORM_NEAREST = 0, CVS_TRANSFORM_BILINEAR = 1 };" in header
    assert "enum { CVS_TRANSFORM_MAX_COORD = 1 << 23 };" in header
    from canvas_amd import _lib
    from canvas_amd.abi import box2i
    raw = C.CDLL(_lib.LIB_PATH)
    P = C.POINTER
    for name, frame in (("cvs_transform_f32_dev", _lib.rgba_frame_f32), ("cvs_transform_f16_dev", _lib.rgba_frame_f16)):
        assert hasattr(raw, name) and _lib.SIGNATURES[name] == (C.c_int, [P(frame), P(frame), P(_lib.transform_params), C.c_void_p])
    assert _lib.SIGNATURES["cvs_transform_from_parts"] == (C.c_int, [P(C.c_double), P(C.c_double), C.c_double, P(C.c_double), P(C.c_float)])
    assert _lib.SIGNATURES["cvs_transform_target_window"] == (C.c_int, [P(_lib.transform_params), P(box2i), P(box2i), P(box2i)])
    assert _lib.SIGNATURES["cvs_transform_source_window"] == (C.c_int, [P(_lib.transform_params), P(box2i), P(box2i)])
    assert (_lib.TRANSFORM_NEAREST, _lib.TRANSFORM_BILINEAR, _lib.TRANSFORM_MAX_COORD) == (0, 1, 1 << 23)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], stdout=subprocess.PIPE, text=True).stdout
    assert all(re.search(r"\b%s\b" % name, out) for name in ENTRIES + HELPERS)
    symbols = subprocess.run(["nm", _lib.LIB_PATH], stdout=subprocess.PIPE, text=True).stdout
    assert re.search(r"\bcvk_transform\b", symbols) and not re.search(r"\bcvk_transform_fma\b", symbols)


def test_struct_mirror_has_the_c_layout():
    """sizeof and every offset, from a probe compiled against the header."""
    from canvas_amd import _lib
    fields = [name for name, _ in _lib.transform_params._fields_]
    assert fields == ["m", "filter", "flags"]
    probe = ('#include <stddef.h>\n#include <stdio.h>\n#include "canvas_hip.h"\nint main(void) {\n    printf("%zu", sizeof(cvs_transform));\n'
             + "".join('    printf(" %%zu", offsetof(cvs_transform, %s));\n' % f for f in fields)
             + '    printf(" %d %d %d\\n", CVS_TRANSFORM_NEAREST, CVS_TRANSFORM_BILINEAR, CVS_TRANSFORM_MAX_COORD);\n    return 0;\n}\n')
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "probe.c"), os.path.join(tmp, "probe")
        with open(src, "w") as f:
            f.write(probe)
        subprocess.run(["gcc", "-std=gnu11", "-I" + os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout.split()]
    want = ([C.sizeof(_lib.transform_params)] + [getattr(_lib.transform_params, f).offset for f in fields]
            + [_lib.TRANSFORM_NEAREST, _lib.TRANSFORM_BILINEAR, _lib.TRANSFORM_MAX_COORD])
    assert got == want and got[0] == 32
    t = _lib.transform()
    assert (tuple(t.m), t.filter, t.flags) == (IDENTITY, _lib.TRANSFORM_BILINEAR, 0)
    t = _lib.transform((0.5, 2, -3, 4, 0.25, 6), _lib.TRANSFORM_NEAREST)
    assert (tuple(t.m), t.filter, t.flags) == ((0.5, 2.0, -3.0, 4.0, 0.25, 6.0), 0, 0)


def test_entries_refuse_bad_arguments_before_any_launch(lib):
    from canvas_amd import _lib
    from canvas_amd.abi import HostFrame
    full = (0, 0, 7, 7)
    nan, inf = float("nan"), float("inf")

    def built(m=IDENTITY, filt=1, flags=0):
        t = _lib.transform(m, filt)
        t.flags = flags
        return t

    def with_m(k, v):
        m = list(IDENTITY)
        m[k] = v
        return m

    bad = ([("filter", built(filt=f)) for f in (2, -1, 7)]
           + [("flags", built(flags=f)) for f in (1, 2, -1, 0x100)]
           + [("finite", built(with_m(k, v))) for k in range(6) for v in (nan, inf, -inf)]
           + [("determinant", built(m)) for m in ((0, 0, 0, 0, 0, 0), (1, 2, 0, 2, 4, 0), (0, 0, 5, 0, 1, 0), (1, 0, 3, 0, 0, 4))])
    for name, dtype, struct in ((ENTRIES[1], np.uint16, _lib.rgba_frame_f16), (ENTRIES[0], np.float32, _lib.rgba_frame_f32)):
        entry = getattr(lib, name)

        def refused(target, source, t, what):
            lib.cvs_clear_last_error()
            assert entry(target, source, t, None) == -1, what
            assert name in _lib.last_error(), (what, _lib.last_error())
        good = HostFrame(full, dtype, current_window=full)
        for word, t in bad:
            out = HostFrame(full, dtype, current_window=full)
            refused(out.ref(), good.ref(), C.byref(t), (word, tuple(t.m), t.filter, t.flags))
            assert out.current_window.is_empty(), word
            assert word in _lib.last_error(), (word, _lib.last_error())
        out, outside = HostFrame(full, dtype, current_window=full), HostFrame(full, dtype, current_window=(0, 0, 8, 7))
        refused(out.ref(), outside.ref(), C.byref(built()), "source window outside its buffer")
        assert out.current_window.is_empty() and "outside" in _lib.last_error()
        out = HostFrame(full, dtype, current_window=full)
        refused(out.ref(), None, C.byref(built()), "NULL source")
        assert out.current_window.is_empty()
        out = HostFrame(full, dtype, current_window=full)
        refused(out.ref(), good.ref(), None, "NULL transform")
        assert out.current_window.is_empty()
        refused(None, good.ref(), C.byref(built()), "NULL target")
        assert good.current_window.tuple() == full                   # a refused call leaves its source alone
        # coordinates a float does not hold exactly: frames that describe buffers nobody allocates (nothing is dereferenced)
        lim = _lib.TRANSFORM_MAX_COORD
        for sbox, tbox in (((lim - 3, 0, lim + 1, 3), full), ((0, -lim - 1, 3, -lim + 2), full), (full, (0, 0, lim + 1, 3)), (full, (-lim - 1, 0, 3, 3))):
            source = struct(good.c.data, _box(sbox), _box(sbox))
            target = struct(HostFrame(full, dtype).c.data, _box(tbox), _box(tbox))
            refused(C.byref(target), C.byref(source), C.byref(built()), (sbox, tbox))
            assert target.current_window.is_empty() and str(lim) in _lib.last_error()
        # not in place: the same buffer as target and source, through one frame struct and through two
        same = HostFrame(full, dtype, current_window=full)
        refused(same.ref(), same.ref(), C.byref(built()), "in place")
        assert same.current_window.is_empty() and "in place" in _lib.last_error()
        twin = HostFrame(full, dtype, good.array, full)
        twin.c.data = good.c.data
        refused(twin.ref(), good.ref(), C.byref(built()), "in place, two structs")
        assert twin.current_window.is_empty() and good.current_window.tuple() == full
    # the helpers refuse what the entries refuse of a transform, with an empty box
    for word, t in bad:
        win = _box((1, 1, 2, 2))
        lib.cvs_clear_last_error()
        assert lib.cvs_transform_target_window(C.byref(t), C.byref(_box(full)), C.byref(_box(full)), C.byref(win)) == -1 and win.is_empty()
        assert word in _lib.last_error()
        need = _box((1, 1, 2, 2))
        assert lib.cvs_transform_source_window(C.byref(t), C.byref(_box(full)), C.byref(need)) == -1 and need.is_empty()
    assert lib.cvs_transform_target_window(None, C.byref(_box(full)), C.byref(_box(full)), C.byref(_box(full))) == -1
    assert lib.cvs_transform_source_window(C.byref(built()), None, C.byref(_box(full))) == -1


# ---------------------------------------------------------------- coefficients

def test_from_parts_right_angles_are_exact(lib):
    for scale in ((1.0, 1.0), (2.0, 0.5), (-4.0, 0.25), (0.125, -8.0)):
        ix, iy = 1.0 / scale[0], 1.0 / scale[1]
        for rotation, want in ((0.0, (ix, 0, 0, iy)), (90.0, (0, ix, -iy, 0)), (180.0, (-ix, 0, 0, -iy)), (270.0, (0, -ix, iy, 0)),
                               (-90.0, (0, -ix, iy, 0)), (450.0, (0, ix, -iy, 0)), (-360.0, (ix, 0, 0, iy)), (720.0 + 180.0, (-ix, 0, 0, -iy))):
            rc, m = _from_parts(lib, (0.0, 0.0), scale, rotation, (0.0, 0.0))
            assert rc == 0 and (m[0], m[1], m[3], m[4]) == want and m[2] == 0 and m[5] == 0, (scale, rotation, m)
            assert m == tm.from_parts((0.0, 0.0), scale, rotation, (0.0, 0.0))
            # about an anchor, put somewhere: still exact, the offsets integers over the scale
            rc, m = _from_parts(lib, (3.0, -2.0), scale, rotation, (16.0, 40.0))
            assert rc == 0 and (m[0], m[1], m[3], m[4]) == want and all(float(v * 8).is_integer() for v in m), (scale, rotation, m)
    # source (x, y) -> target (-y, x) at 90 degrees: clockwise on a screen whose y runs down
    rc, m = _from_parts(lib, (0.0, 0.0), (1.0, 1.0), 90.0, (0.0, 0.0))
    tx, ty = -5.0, 2.0                                               # where source (2, 5) lands
    assert (m[0] * tx + m[1] * ty + m[2], m[3] * tx + m[4] * ty + m[5]) == (2.0, 5.0)


def test_from_parts_degenerate_and_refused(lib):
    from canvas_amd import _lib
    nan, inf = float("nan"), float("inf")
    for scale in ((0.0, 1.0), (1.0, 0.0), (0.0, 0.0), (-0.0, 2.0)):
        rc, m = _from_parts(lib, (1.0, 2.0), scale, 30.0, (3.0, 4.0))
        assert rc == 1 and m == (7.0,) * 6                           # degenerate: m untouched
        assert tm.from_parts((1.0, 2.0), scale, 30.0, (3.0, 4.0)) is None
    good = dict(anchor=(1.0, 2.0), scale=(1.5, 0.5), rotation=30.0, position=(3.0, 4.0))
    for name in good:
        for v in (nan, inf, -inf):
            parts = dict(good)
            parts[name] = v if name == "rotation" else (good[name][0], v)
            lib.cvs_clear_last_error()
            rc, m = _from_parts(lib, parts["anchor"], parts["scale"], parts["rotation"], parts["position"])
            assert rc == -1 and m == (7.0,) * 6 and "cvs_transform_from_parts" in _lib.last_error(), (name, v)
    # a finite input whose inverse no f32 holds
    rc, m = _from_parts(lib, (0.0, 0.0), (1e-200, 1.0), 0.0, (0.0, 0.0))
    assert rc == -1 and m == (7.0,) * 6
    assert _from_parts(lib, *[good[k] for k in ("anchor", "scale", "rotation", "position")])[0] == 0


def test_from_parts_inverts_the_forward_map(lib):
    """200 seeded transforms with coordinates up to 4096 and scales between 1/2 and 2 of either sign: a point sent forward in
    float64 and back through the six f32 coefficients returns to within 1e-2 pixel.  Each coefficient carries a relative
    rounding of 2^-24; with |m0|, |m1| <= 2 and |m2| <= 2 * 3 * 4096 the three terms are off by at most
    2 * (2 * 4096 * 2^-24) + 24576 * 2^-24 = 2.5e-3: the bound has a fourfold margin."""
    rng = np.random.default_rng(200)
    worst = 0.0
    for _ in range(200):
        anchor, position, p = (tuple(float(v) for v in rng.uniform(-4096, 4096, 2)) for _ in range(3))
        scale = tuple(float(v) for v in np.exp(rng.uniform(-math.log(2), math.log(2), 2)) * rng.choice([-1.0, 1.0], 2))
        rotation = float(rng.uniform(-720, 720))
        rc, m = _from_parts(lib, anchor, scale, rotation, position)
        assert rc == 0 and m == tm.from_parts(anchor, scale, rotation, position)
        c, s = math.cos(math.radians(rotation)), math.sin(math.radians(rotation))
        dx, dy = scale[0] * (p[0] - anchor[0]), scale[1] * (p[1] - anchor[1])
        tx, ty = position[0] + (c * dx - s * dy), position[1] + (s * dx + c * dy)
        bx, by = m[0] * tx + m[1] * ty + m[2], m[3] * tx + m[4] * ty + m[5]
        worst = max(worst, abs(bx - p[0]), abs(by - p[1]))
    print("worst round trip: %.3g pixel" % worst)
    assert worst <= 1e-2


# ---------------------------------------------------------------- windows

def test_window_helpers_equal_the_models_formulas(lib):
    cases = _transforms(31, 200, 4096)
    for S, parts, m in cases:
        for filt in FILTERS:
            for tfull in (EVERYWHERE, (S[0] - 7, S[1] - 40, S[0] + 30, S[1] + 3), (-4096, -4096, 4096, 4096)):
                assert _target_window(lib, m, filt, S, tfull) == (0, tm.target_window(m, filt, S, tfull)), (S, parts, filt, tfull)
            window = (int(parts["position"][0]) - 4, int(parts["position"][1]) - 2, int(parts["position"][0]) + 9, int(parts["position"][1]) + 5)
            assert _source_window(lib, m, filt, window) == (0, tm.source_window(m, window)), (parts, window)
    # one pixel under the identity: grown by the filter's reach and the margin
    one = (5, -3, 5, -3)
    assert _target_window(lib, IDENTITY, tm.BILINEAR, one, EVERYWHERE) == (0, (3, -5, 7, -1)) == (0, tm.target_window(IDENTITY, tm.BILINEAR, one, EVERYWHERE))
    assert _target_window(lib, IDENTITY, tm.NEAREST, one, EVERYWHERE) == (0, (3, -5, 7, -1)) == (0, tm.target_window(IDENTITY, tm.NEAREST, one, EVERYWHERE))
    assert _source_window(lib, IDENTITY, tm.BILINEAR, one) == (0, (3, -5, 7, -1)) == (0, tm.source_window(IDENTITY, one))
    # clipped to the target, disjoint from it, empty inputs
    assert _target_window(lib, IDENTITY, 1, (0, 0, 9, 9), (4, 4, 30, 30)) == (0, (4, 4, 11, 11))
    assert _target_window(lib, IDENTITY, 1, (0, 0, 9, 9), (40, 0, 50, 9)) == (0, None) and tm.target_window(IDENTITY, 1, (0, 0, 9, 9), (40, 0, 50, 9)) is None
    assert _target_window(lib, IDENTITY, 1, None, EVERYWHERE) == (0, None) and _target_window(lib, IDENTITY, 1, (0, 0, 9, 9), None) == (0, None)
    assert _source_window(lib, IDENTITY, 1, None) == (0, None)
    # the clamp: a magnification of 2^40 sends the corners far beyond what an int holds
    huge = (2.0 ** -40, 0.0, 0.0, 0.0, 2.0 ** -40, 0.0)
    far = (-(1 << 31), -(1 << 31), (1 << 31) - 1, (1 << 31) - 1)
    lim = 1 << 30
    assert _target_window(lib, huge, 1, (-4, 2, 9, 9), far) == (0, (-lim, lim, lim, lim)) == (0, tm.target_window(huge, 1, (-4, 2, 9, 9), far))
    tiny = (2.0 ** 40, 0.0, 0.0, 0.0, -(2.0 ** 40), 0.0)
    assert _source_window(lib, tiny, 1, (-4, 2, 9, 9)) == (0, (-lim, -lim, lim, -lim)) == (0, tm.source_window(tiny, (-4, 2, 9, 9)))


def _tapped(m, filt, S, window):
    """Which pixels of target window `window` have a tap inside S (the model's f32 arithmetic), and the tap planes"""
    u, v = tm.source_coords(m, window)
    with np.errstate(all="ignore"):
        if filt == tm.NEAREST:
            taps = [(np.floor((u + np.float32(0.5)).astype(np.float32)), np.floor((v + np.float32(0.5)).astype(np.float32)))]
        else:
            i, j = np.floor(u), np.floor(v)
            taps = [((i + np.float32(di)).astype(np.float32), (j + np.float32(dj)).astype(np.float32)) for dj in (0, 1) for di in (0, 1)]
    hit = np.zeros(u.shape, bool)
    for ti, tj in taps:
        hit |= tm.inside(ti, tj, S)
    return hit, taps


def test_windows_are_safe_by_brute_force():
    """1000 seeded transforms with coordinates within +-2^14, both filters: no target pixel outside the target window has a tap
    inside S (looked for in a ring of 6 pixels around it), and every source pixel that the taps of a target window touch lies
    inside the source window."""
    slack = None
    for S, parts, m in _transforms(14, 1000, 1 << 14):
        for filt in FILTERS:
            win = tm.target_window(m, filt, S, EVERYWHERE)
            assert win is not None
            ring = (win[0] - 6, win[1] - 6, win[2] + 6, win[3] + 6)
            assert (ring[2] - ring[0]) * (ring[3] - ring[1]) < 1 << 18, (S, parts, win)
            hit, _ = _tapped(m, filt, S, ring)
            ys, xs = np.nonzero(hit)
            if not len(xs):                                          # a layer shrunk to less than a pixel can miss every sample
                continue
            x0, x1, y0, y1 = ring[0] + xs.min(), ring[0] + xs.max(), ring[1] + ys.min(), ring[1] + ys.max()
            assert win[0] <= x0 and x1 <= win[2] and win[1] <= y0 and y1 <= win[3], (S, parts, filt, win, (x0, y0, x1, y1))
            least = min(x0 - win[0], win[2] - x1, y0 - win[1], win[3] - y1)
            slack = least if slack is None else min(slack, least)
            # a target window about where the layer lands, some of it off the layer
            px, py = int(parts["position"][0]), int(parts["position"][1])
            window = (px - 5, py - 9, px + 8, py + 3)
            need = tm.source_window(m, window)
            _, taps = _tapped(m, filt, EVERYWHERE, window)
            for ti, tj in taps:
                assert need[0] <= ti.min() and ti.max() <= need[2] and need[1] <= tj.min() and tj.max() <= need[3], (parts, filt, window, need)
    print("smallest slack of the target window: %d pixel" % slack)


# ---------------------------------------------------------------- the model

def _frames(rng, h, w):
    f32 = rng.uniform(-0.25, 1.25, (h, w, 4)).astype(np.float32)
    f32[..., 3] = rng.uniform(0.0, 1.0, (h, w)).astype(np.float32)
    f32[0, 0] = [np.nan, -0.0, 1e-40, 0.5]
    codes = rng.integers(0, 0x3C01, (h, w, 4), dtype=np.uint16)
    codes[0, 0] = [0x7C01, 0x8000, 0x0001, 0x3555]
    return f32, codes


def _bits(a):
    return a if a.dtype == np.uint16 else np.ascontiguousarray(a).view(np.uint32)


def test_model_exact_maps_are_permutations_of_the_codes():
    """Identity, an integer shift, the mirrors and the three right-angle rotations about anchors with integer results move the
    source's codes, NaN payloads and zero signs included, in both filters and both formats."""
    h, w = 5, 7
    S = (0, 0, w - 1, h - 1)
    for source in _frames(np.random.default_rng(9), h, w):
        for filt in FILTERS:
            def run(window, **parts):
                return _bits(tm.transform_plane(source, S, tm.from_parts(**parts), filt, window))
            s = _bits(source)
            assert np.array_equal(run(S), s)
            assert np.array_equal(run((3, -2, w + 2, h - 3), position=(3, -2)), s)
            assert np.array_equal(run(S, scale=(-1, 1), position=(w - 1, 0)), s[:, ::-1])
            assert np.array_equal(run(S, scale=(1, -1), position=(0, h - 1)), s[::-1])
            assert np.array_equal(run((0, 0, h - 1, w - 1), rotation=90, position=(h - 1, 0)), np.rot90(s, -1))
            assert np.array_equal(run(S, rotation=180, position=(w - 1, h - 1)), np.rot90(s, 2))
            assert np.array_equal(run((0, 0, h - 1, w - 1), rotation=270, position=(0, w - 1)), np.rot90(s, 1))
            assert np.array_equal(run((0, 0, h - 1, w - 1), rotation=-90, anchor=(w - 1, 0), position=(0, 0)), np.rot90(s, 1))
            # beyond the layer: zeros
            wide = run((-2, -2, w + 1, h + 1))
            assert np.array_equal(wide[2:-2, 2:-2], s) and not wide[:2].any() and not wide[-2:].any() and not wide[:, :2].any() and not wide[:, -2:].any()


# twice the worst the model showed over the 500 transforms of seed 500 (the test prints it: 2, 2, 2 and 1 ulp of the constant)
CONSTANT_BOUND_ULPS = np.array([4.0, 4.0, 4.0, 2.0])


def test_model_constant_opaque_frame_stays_constant_in_the_interior():
    """500 seeded transforms of a constant opaque frame: where all four taps are inside S the weights sum to 1 within rounding and
    the colour comes back.  A guard of the model against edits, not a bar for the kernel."""
    rng = np.random.default_rng(500)
    colour = np.array([0.8125, 0.3, 0.05, 1.0], np.float32)
    S = (-6, -4, 13, 11)
    source = np.broadcast_to(colour, (16, 20, 4)).copy()
    worst = np.zeros(4)
    seen = 0
    for _ in range(500):
        m = tm.from_parts(anchor=tuple(rng.uniform(-6, 13, 2)), scale=tuple(np.exp(rng.uniform(-1, 1, 2)) * rng.choice([-1.0, 1.0], 2)),
                          rotation=float(rng.uniform(-360, 360)), position=tuple(rng.uniform(-20, 20, 2)))
        window = tm.target_window(m, tm.BILINEAR, S, (-60, -60, 60, 60))
        if window is None:
            continue
        out = tm.transform_plane(source, S, m, tm.BILINEAR, window)
        u, v = tm.source_coords(m, window)
        i, j = np.floor(u), np.floor(v)
        interior = tm.inside(i, j, S) & tm.inside(i + np.float32(1), j + np.float32(1), S)
        seen += int(interior.sum())
        for ch in range(4):
            off = np.abs(out[..., ch][interior].astype(np.float64) - float(colour[ch])) / float(np.spacing(colour[ch]))
            worst[ch] = max(worst[ch], off.max() if off.size else 0.0)
    print("worst deviation in ulps (r, g, b, a):", worst, "over", seen, "interior pixels")
    assert seen > 10000
    assert (worst <= CONSTANT_BOUND_ULPS).all(), worst


def test_model_edges_keep_their_colour_and_only_alpha_falls_off():
    colour = np.array([0.8125, 0.3, 0.05, 1.0], np.float32)
    S = (0, 0, 9, 7)
    for source in (np.broadcast_to(colour, (8, 10, 4)).copy(), np.broadcast_to(np.array([0x3A80, 0x34CD, 0x2A66, 0x3C00], np.uint16), (8, 10, 4)).copy()):
        half = source.dtype == np.uint16
        m = tm.from_parts(position=(0.5, 0.5))                       # u = x - 0.5, v = y - 0.5: every weight is 1/4
        window = tm.target_window(m, tm.BILINEAR, S, EVERYWHERE)
        assert window == (-2, -2, 12, 10)
        out = tm.transform_plane(source, S, m, tm.BILINEAR, window)
        wide = tm.widen(out) if half else out
        want = tm.widen(source[0, 0]) if half else source[0, 0]
        alpha = wide[..., 3]
        covered = alpha != 0
        # columns 0 .. 10 and rows 0 .. 8 of the target see the layer
        assert np.array_equal(np.argwhere(covered.any(axis=0)).ravel() + window[0], np.arange(0, 11))
        assert np.array_equal(np.argwhere(covered.any(axis=1)).ravel() + window[1], np.arange(0, 9))
        for ch in range(3):
            assert (wide[..., ch][covered] == want[ch]).all(), ch    # the colour everywhere the layer reaches, the rim included
            assert (wide[..., ch][~covered] == 0).all()
        row = lambda y: alpha[y - window[1], 2 - window[0]]          # noqa: E731
        col = lambda x: alpha[3 - window[1], x - window[0]]          # noqa: E731
        assert (col(0), col(1), col(10)) == (0.5, 1.0, 0.5) and (row(0), row(1), row(8)) == (0.5, 1.0, 0.5)
        assert alpha[0 - window[1], 0 - window[0]] == 0.25 and alpha[8 - window[1], 10 - window[0]] == 0.25


def test_model_transparent_neighbourhoods_give_zeros():
    rng = np.random.default_rng(6)
    source = rng.uniform(0.1, 1.0, (12, 14, 4)).astype(np.float32)
    source[3:9, 4:11, 3] = 0.0                                       # a hole whose colour is still there
    source[5, 6, :3] = [np.inf, -3.0, 6.0e4]
    S = (0, 0, 13, 11)
    m = tm.from_parts(position=(0.25, 0.5))
    window = (0, 0, 13, 11)
    for pixels in (source, f2h_rz_model(source)):
        out = tm.transform_plane(pixels, S, m, tm.BILINEAR, window)
        assert not out[4:9, 5:11].any()                              # all four taps transparent: colour exactly 0, alpha 0
        assert out[2, 5].all() and out[4, 4, 3] != 0
        near = tm.transform_plane(pixels, S, tm.from_parts(rotation=90, position=(11, 0)), tm.NEAREST, (0, 0, 11, 13))
        assert np.array_equal(_bits(near), np.rot90(_bits(pixels), -1))   # nearest copies the hole, colour and all


def test_model_sampler_is_the_one_both_warps_share():
    """transform_plane is sample() over its own coordinates, and the corner pin's plane with affine coefficients and zero origins
    is the same bytes: the model-side twin of test_affine_coefficients_with_zero_origins_give_the_transforms_bytes."""
    from tests import perspective_model as pm
    rng = np.random.default_rng(11)
    source = rng.uniform(0.0, 1.0, (7, 9, 4)).astype(np.float32)
    source[2:4, 3:6, 3] = 0.0
    S, win = (0, 0, 8, 6), (-2, -1, 9, 8)                            # 9 x 7 under a 12 x 10 window: taps outside S on every side
    m = tm.from_parts(anchor=(4.0, 3.0), rotation=30.0, position=(4.0, 3.0))
    p = (tuple(m) + (0.0, 0.0, 1.0), (0, 0), (0, 0))
    for pixels in (f2h_rz_model(source), source):
        for filt in FILTERS:
            plane = tm.transform_plane(pixels, S, m, filt, win)
            assert plane.dtype == pixels.dtype and plane.shape == (10, 12, 4) and plane.any() and not plane[0, 0].any()
            assert plane.tobytes() == tm.sample(pixels, S, *tm.source_coords(m, win), filt).tobytes()
            assert plane.tobytes() == pm.perspective_plane(pixels, S, p, filt, win).tobytes()


# ---------------------------------------------------------------- the code object

def test_code_object_holds_every_instance_without_scratch():
    """One build for both arithmetic flavours; f32 / f16 x nearest / bilinear."""
    assert os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"), "the ROCm LLVM tools the build itself needs are missing"
    found = _kernels("transform_ops.hip.o")
    names = [n for n in found if "k_transform" in n]
    assert len(names) == 4 and len(found) == 4, sorted(found)
    for half in (0, 1):
        for bilinear in (0, 1):
            assert any("k_transformILi%dELi%dELi" % (half, bilinear) in n for n in names), (half, bilinear)
    for name, (scratch, spills) in found.items():
        assert scratch == 0 and spills == 0, (name, scratch, spills)
    assert not os.path.exists(os.path.join(ROOT, "canvas_amd", "csrc", "build", "transform_ops.fma.hip.o"))
    spec = __import__("importlib.util").util.spec_from_file_location("check_asm_loads", os.path.join(ROOT, "tools", "check_asm_loads.py"))
    chk = __import__("importlib.util").util.module_from_spec(spec)
    spec.loader.exec_module(chk)
    checked, problems = chk.check_paths([os.path.join(ROOT, "canvas_amd", "csrc", "build", "transform_ops.hip.o")])
    assert checked >= 4 and not problems, problems[:5]


# ---------------------------------------------------------------- the node

def test_node_surface(process):
    from fluggo.media import basetypes as bt
    red = process.SolidColorVideoSource((1, 0, 0, 1))
    cls = process.VideoTransformFilter
    assert issubclass(cls, process.VideoSource)
    rect = bt.box2i(0, 0, 31, 17)
    node = cls(red, rect)
    cap = node._video_frame_source_funcs
    assert type(cap).__name__ == "PyCapsule" and '"_video_frame_source_funcs"' in repr(cap)
    assert node.source is red and node.source_rect == rect
    assert (node.anchor, node.scale, node.rotation, node.position, node.filter) == ((0.0, 0.0), (1.0, 1.0), 0.0, (0.0, 0.0), "bilinear")
    assert node.inverse_at(0) == IDENTITY
    node = cls(red, rect, (3, 2), (2, 0.5), 90, (16, 40), "nearest")
    assert (node.anchor, node.scale, node.rotation, node.position, node.filter) == ((3, 2), (2, 0.5), 90, (16, 40), "nearest")
    assert node.inverse_at(5) == tm.from_parts((3, 2), (2, 0.5), 90, (16, 40)) == (0.0, 0.5, -17.0, -2.0, 0.0, 34.0)
    node = cls(source=red, filter="bilinear", position=bt.v2f(1.5, 2), rotation=-17.5, scale=(1.5, 0.75), anchor=(8, 8), source_rect=rect)
    assert node.inverse_at(0) == tm.from_parts((8, 8), (1.5, 0.75), -17.5, (1.5, 2))
    other = process.SolidColorVideoSource((0, 1, 0, 1))
    node.set_source(other)
    assert node.source is other
    node.source = red
    assert node.source is red
    node.set_source(None)
    assert node.source is None
    spin = process.LerpFunc((0.0,), (90.0,), 2.0)
    slide = process.LerpFunc((0.0, 0.0), (4.0, 8.0), 2.0)
    for name, value, func in (("anchor", (1.5, -2.0), slide), ("scale", (0.5, 2.0), slide), ("position", (7.0, 9.0), slide), ("rotation", 33.5, spin),
                              ("source_rect", bt.box2i(1, 2, 3, 4), process.LerpFunc((0, 0, 9, 9), (4, 4, 13, 13), 2.0))):
        setattr(node, name, value)
        assert getattr(node, name) == value
        setattr(node, name, func)
        assert getattr(node, name) is func
        for bad in ("much", None, object(), (), (1, 2, 3), ((1, 2),), 5 if name != "rotation" else (5, 5), (float("nan"), 1.0) if name != "rotation" else float("inf")):
            with pytest.raises(Exception):
                setattr(node, name, bad)
            assert getattr(node, name) is func                      # a refused value leaves the old one
        setattr(node, name, value)
        assert getattr(node, name) == value
    node.rotation = spin
    node.anchor, node.scale, node.position = (0, 0), (1, 1), (0, 0)
    assert node.inverse_at(0) == IDENTITY and node.inverse_at(2) == tm.from_parts(rotation=90) and node.inverse_at(1) == tm.from_parts(rotation=45)
    node.scale = (0, 1)
    assert node.inverse_at(0) is None                                # degenerate: nothing to draw
    node.scale = (1, 1)
    for good in ("nearest", "bilinear"):
        node.filter = good
        assert node.filter == good
    for bad in ("bicubic", "", 1, None, b"nearest"):
        with pytest.raises(Exception):
            node.filter = bad
        assert node.filter == "bilinear"
    for bad in (object(), 3, "source"):
        with pytest.raises(Exception):
            cls(bad, rect)
        with pytest.raises(Exception):
            node.set_source(bad)
    with pytest.raises(TypeError):
        cls()
    with pytest.raises(TypeError):
        cls(red)                                                     # source_rect is required
    for kw in (dict(anchor="far"), dict(anchor=None), dict(scale=2), dict(rotation=(1, 2)), dict(rotation="quarter"), dict(position=(1, 2, 3)), dict(filter="cubic"),
               dict(filter=0)):
        with pytest.raises(Exception):
            cls(red, rect, **kw)
    with pytest.raises(Exception):
        cls(red, (0, 0))


# ---------------------------------------------------------------- without a device

def test_pull_without_a_device_or_a_source_gives_an_empty_window():
    """In a child process that sees no GPU: pulled as f16 and as f32, with and without a source, drawable and degenerate."""
    script = r"""
import sys
sys.path.insert(0, %r)
from fluggo.media import process, basetypes
window = basetypes.box2i(0, 0, 31, 17)
red = process.SolidColorVideoSource((1, 0, 0, 1))
for source in (None, red):
    for scale in ((0, 1), (1, 1)):
        for filter in ("bilinear", "nearest"):
            node = process.VideoTransformFilter(source, window, (16, 9), scale, 30.0, (16, 9), filter)
            assert node.get_frame_f16(0, window).current_window.empty()
            assert node.get_frame_f32(0, window).current_window.empty()
            assert process.last_error() or (source is None and scale[0] == 0), "no message"
print("message:", process.last_error())
""" % ROOT
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    p = subprocess.run([os.sys.executable, "-c", script], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout
    assert "message:" in p.stdout and re.search(r"device|HIP|hip", p.stdout), p.stdout
