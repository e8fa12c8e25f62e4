"""The corner pin without a GPU (DESIGN.md "Corner pin"): include/canvas_perspective.h against the library and its bindings;
cvs_perspective_from_quad and the two window functions of host/perspective.c against the float64 model
(tests/perspective_model.py), bit for bit; the margins of the two windows against the f32 pixel rule by brute force; every refusal
of the two device entries; the catalogue of tests/perspective_cases.py; the built code object."""
import ctypes as C
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from tests import perspective_model as pm
from tests.test_unsharp_cpu import _kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
HEADER = "canvas_perspective.h"
FIELDS = ["h", "target_origin", "source_origin", "filter", "flags"]


@pytest.fixture(scope="module")
def lib():
    from canvas_amd import _lib
    return _lib.load()


# ---------------------------------------------------------------- the header, the library, the bindings

def test_struct_mirror_has_the_c_layout():
    """sizeof, every offset and the constant, from a probe compiled against the header."""
    from canvas_amd import _lib
    assert [name for name, _ in _lib.perspective_params._fields_] == FIELDS
    probe = ('#include <stddef.h>\n#include <stdio.h>\n#include "%s"\nint main(void) {\n    printf("%%zu", sizeof(cvs_perspective));\n' % HEADER
             + "".join('    printf(" %%zu", offsetof(cvs_perspective, %s));\n' % f for f in FIELDS)
             + '    printf(" %d\\n", CVS_PERSPECTIVE_MAX_SPAN);\n    return 0;\n}\n')
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "probe.c"), os.path.join(tmp, "probe")
        with open(src, "w") as f:
            f.write(probe)
        subprocess.run(["gcc", "-std=gnu11", "-I" + os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout.split()]
    want = [C.sizeof(_lib.perspective_params)] + [getattr(_lib.perspective_params, f).offset for f in FIELDS] + [_lib.PERSPECTIVE_MAX_SPAN]
    assert got == want and got[0] == 60 and got[-1] == 1 << 23
    p = _lib.perspective((1, 2, 3, 4, 5, 6, 7, 8, 9), (-3, 5), (7, -11), _lib.TRANSFORM_NEAREST)
    assert (list(p.h), list(p.target_origin), list(p.source_origin), p.filter, p.flags) == ([1, 2, 3, 4, 5, 6, 7, 8, 9], [-3, 5], [7, -11], 0, 0)
    P = C.POINTER
    assert _lib.PERSPECTIVE_SIGNATURES == {
        "cvs_perspective_f32_dev": (C.c_int, [P(_lib.rgba_frame_f32), P(_lib.rgba_frame_f32), P(_lib.perspective_params), C.c_void_p]),
        "cvs_perspective_f16_dev": (C.c_int, [P(_lib.rgba_frame_f16), P(_lib.rgba_frame_f16), P(_lib.perspective_params), C.c_void_p]),
        "cvs_perspective_from_quad": (C.c_int, [P(C.c_double), P(C.c_double * 2), C.c_int, P(_lib.perspective_params)]),
        "cvs_perspective_target_window": (C.c_int, [P(_lib.perspective_params), P(_lib.box2i), P(_lib.box2i), P(_lib.box2i)]),
        "cvs_perspective_source_window": (C.c_int, [P(_lib.perspective_params), P(_lib.box2i), P(_lib.box2i)]),
    }


def _declared(header):
    """(every function include/<header> declares with CVS_EXPORT, its cvs_*_dev functions whose last parameter is a cvs_stream_t)"""
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    text = "\n".join(l for l in text.splitlines() if not l.lstrip().startswith("#"))
    funcs = sorted(set(re.findall(r"CVS_EXPORT\s+[^;(]*?\b(\w+)\s*\(", text)))
    entries = [name for name, params in re.findall(r"CVS_EXPORT\s+int\s+(cvs_\w+_dev)\s*\(([^;{]*?)\)\s*;", text, flags=re.S)
               if params.split(",")[-1].split()[0] == "cvs_stream_t"]
    return funcs, sorted(entries)


def test_every_symbol_of_the_header_is_exported_and_bound(lib):
    """What tests/test_abi_cpu.py holds canvas_hip.h to, for include/canvas_perspective.h and its own table of bindings."""
    from canvas_amd import _lib
    funcs, entries = _declared(HEADER)
    assert funcs == sorted(_lib.PERSPECTIVE_SIGNATURES) and len(funcs) == 5
    assert entries == ["cvs_perspective_f16_dev", "cvs_perspective_f32_dev"]
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert not [f for f in funcs if f not in exported]
    assert not set(_lib.PERSPECTIVE_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.SCOPE_SIGNATURES) | set(_lib.LUT3D_SIGNATURES))
    for name in funcs:
        assert getattr(lib, name).argtypes == _lib.PERSPECTIVE_SIGNATURES[name][1] and getattr(lib, name).restype is _lib.PERSPECTIVE_SIGNATURES[name][0], name
    for name in entries:
        assert _lib.PERSPECTIVE_SIGNATURES[name][1][-1] is C.c_void_p, name
    # one launcher, one arithmetic flavour
    symbols = subprocess.run(["nm", _lib.LIB_PATH], stdout=subprocess.PIPE, text=True).stdout
    assert re.search(r"\bcvk_perspective\b", symbols) and not re.search(r"\bcvk_perspective_fma\b", symbols)


def test_the_header_compiles_as_c_and_as_cpp():
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "t.c")
        with open(src, "w") as f:
            f.write('#include "%s"\nint main(void) { cvs_perspective p; p.filter = CVS_TRANSFORM_BILINEAR; p.flags = 0; '
                    'return sizeof p == 60 && CVS_PERSPECTIVE_MAX_SPAN == 8388608 && p.filter == 1 ? 0 : 1; }\n' % HEADER)
        for cc, std, lang in (("gcc", "-std=c99", "c"), ("g++", "-std=c++14", "c++")):
            exe = os.path.join(tmp, "t_" + cc)
            subprocess.run([cc, std, "-Wall", "-Werror", "-x", lang, src, "-I", os.path.join(ROOT, "include"), "-o", exe], check=True)
            assert subprocess.run([exe]).returncode == 0


def test_code_object_holds_the_four_instances_without_scratch():
    """One build for both arithmetic flavours; f32 / f16 x nearest / bilinear; no private segment, no spills, and no register read
    between a load into it and the wait that retires it."""
    assert os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"), "the ROCm LLVM tools the build itself needs are missing"
    found = _kernels("perspective_ops.hip.o")
    assert len(found) == 4 and all("k_perspective" in n for n in found), sorted(found)
    for half in (0, 1):
        for bilinear in (0, 1):
            assert any("k_perspectiveILi%dELi%dEEE" % (half, bilinear) in n for n in found), (half, bilinear, sorted(found))
    for name, (scratch, spills) in found.items():
        assert scratch == 0 and spills == 0, (name, scratch, spills)
    assert not os.path.exists(os.path.join(ROOT, "canvas_amd", "csrc", "build", "perspective_ops.fma.hip.o"))
    spec = __import__("importlib.util").util.spec_from_file_location("check_asm_loads", os.path.join(ROOT, "tools", "check_asm_loads.py"))
    chk = __import__("importlib.util").util.module_from_spec(spec)
    spec.loader.exec_module(chk)
    checked, problems = chk.check_paths([os.path.join(ROOT, "canvas_amd", "csrc", "build", "perspective_ops.hip.o")])
    assert checked >= 4 and not problems, problems[:5]


# ---------------------------------------------------------------- cvs_perspective_from_quad

def _from_quad(lib, rect, quad, filt=pm.BILINEAR, p=None):
    from canvas_amd import _lib
    r = (C.c_double * 4)(*[float(v) for v in rect])
    q = ((C.c_double * 2) * 4)(*[(C.c_double * 2)(float(a), float(b)) for a, b in quad])
    p = _lib.perspective() if p is None else p
    lib.cvs_clear_last_error()
    return lib.cvs_perspective_from_quad(r, q, filt, C.byref(p)), p


def _triple(p):
    return tuple(float(v) for v in p.h), tuple(p.target_origin), tuple(p.source_origin)


BOX = (3, 1, 24, 12)                                                  # 22 x 12 samples
RECT = pm.outer(BOX)
W, H = RECT[2] - RECT[0], RECT[3] - RECT[1]


def _moved(quad, dx, dy):
    return [(x + dx, y + dy) for x, y in quad]


def _turned(k):
    """the rectangle's picture turned by k right angles about (10.5, 20.5): every corner on a pixel's corner"""
    c = [(-W / 2, -H / 2), (W / 2, -H / 2), (W / 2, H / 2), (-W / 2, H / 2)]
    for _ in range(k):
        c = [(-y, x) for x, y in c]
    return [(x + 10.5, y + 20.5) for x, y in c]


KEYSTONE = [(RECT[0] + 0.2 * W, RECT[1]), (RECT[0] + 0.8 * W, RECT[1]), (RECT[2], RECT[3]), (RECT[0], RECT[3])]
GENERAL = [(5.25, -2.5), (31.0, 3.75), (27.5, 22.125), (-1.75, 15.5)]
QUADS = [("identity", pm.rect_quad(RECT)), ("integer shift", _moved(pm.rect_quad(RECT), 7, -4)),
         ("mirror x", [pm.rect_quad(RECT)[k] for k in (1, 0, 3, 2)]), ("mirror y", [pm.rect_quad(RECT)[k] for k in (3, 2, 1, 0)]),
         ("turn 0", _turned(0)), ("turn 90", _turned(1)), ("turn 180", _turned(2)), ("turn 270", _turned(3)),
         ("half-pixel shift", _moved(pm.rect_quad(RECT), 0.5, 0.5)), ("keystone", KEYSTONE), ("general", GENERAL),
         ("general mirrored", [GENERAL[k] for k in (1, 0, 3, 2)])]
FAR = (2 ** 15 + 1, -2 ** 16)


@pytest.mark.parametrize("name,quad", QUADS, ids=[q[0] for q in QUADS])
def test_from_quad_is_the_model_bit_for_bit(lib, name, quad):
    want = pm.from_quad(RECT, quad)
    assert want is not None
    for filt in (pm.NEAREST, pm.BILINEAR):
        rc, p = _from_quad(lib, RECT, quad, filt)
        assert rc == 0 and p.filter == filt and p.flags == 0
        got = _triple(p)
        assert np.array_equal(np.array(got[0], F32).view(np.uint32), np.array(want[0], F32).view(np.uint32)), (got, want)
        assert got[1:] == want[1:]
    h = want[0]
    if name in ("identity", "integer shift", "mirror x", "mirror y") or name.startswith("turn"):
        assert h[6:] == (0.0, 0.0, 1.0) and all(v in (0.0, 1.0, -1.0) for v in (h[0], h[1], h[3], h[4])) and h[2] == int(h[2]) and h[5] == int(h[5]), h
    if name == "identity":
        assert h == (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0) and want[1] == want[2]
    if name == "half-pixel shift":
        # source = target - 1/2, said between the two origins
        assert h[:2] + h[3:5] + h[6:] == (1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0) and abs(h[2]) == 0.5 and abs(h[5]) == 0.5
        assert h[2] + want[2][0] - want[1][0] == -0.5 and h[5] + want[2][1] - want[1][1] == -0.5
    if name in ("keystone", "general", "general mirrored"):
        # the four corners map back to the rectangle's, and w is +1 at the quad's centre
        corners = pm.rect_quad(RECT)
        for (x, y), (rx, ry) in zip(quad, corners):
            x, y = x - want[1][0], y - want[1][1]
            w = h[6] * x + h[7] * y + h[8]
            assert w > 0
            assert abs((h[0] * x + h[1] * y + h[2]) / w + want[2][0] - rx) < 1e-4 and abs((h[3] * x + h[4] * y + h[5]) / w + want[2][1] - ry) < 1e-4
        cx, cy = sum(q[0] for q in quad) / 4 - want[1][0], sum(q[1] for q in quad) / 4 - want[1][1]
        assert abs(h[6] * cx + h[7] * cy + h[8] - 1.0) < 1e-6
    # moved far: h is unchanged, only the origins move
    far_rect = (RECT[0] + FAR[0], RECT[1] + FAR[1], RECT[2] + FAR[0], RECT[3] + FAR[1])
    rc, p = _from_quad(lib, far_rect, _moved(quad, *FAR))
    assert rc == 0
    got, model = _triple(p), pm.from_quad(far_rect, _moved(quad, *FAR))
    assert got == model
    assert got[0] == want[0] and got[1] == (want[1][0] + FAR[0], want[1][1] + FAR[1]) and got[2] == (want[2][0] + FAR[0], want[2][1] + FAR[1])


def test_from_quad_gives_1_for_a_quad_that_is_not_convex(lib):
    from canvas_amd import _lib
    bad = {"concave": [(0, 0), (10, 0), (3, 3), (0, 10)], "bow-tie": [(0, 0), (10, 0), (0, 10), (10, 10)],
           "three collinear corners": [(0, 0), (5, 0), (10, 0), (0, 10)], "a repeated corner": [(0, 0), (10, 0), (10, 0), (0, 10)],
           "a point": [(1, 1)] * 4}
    for name, quad in bad.items():
        assert pm.from_quad(RECT, quad) is None, name
        p = _lib.perspective((9, 8, 7, 6, 5, 4, 3, 2, 1), (11, 12), (13, 14), pm.NEAREST)
        rc, p = _from_quad(lib, RECT, quad, pm.BILINEAR, p)
        assert rc == 1 and not _lib.last_error(), (name, rc)
        assert _triple(p) == ((9, 8, 7, 6, 5, 4, 3, 2, 1), (11, 12), (13, 14)) and p.filter == pm.NEAREST, name


def test_from_quad_refuses_what_is_not_finite_or_not_ascending(lib):
    from canvas_amd import _lib
    nan, inf = float("nan"), float("inf")
    good = pm.rect_quad(RECT)
    cases = [((0, 0, nan, 5), good, "finite"), ((0, -inf, 4, 5), good, "finite"), (RECT, [(nan, 0)] + good[1:], "finite"), (RECT, good[:3] + [(0, inf)], "finite"),
             ((5, 0, 5, 4), good, "not ascending"), ((0, 4, 5, 4), good, "not ascending"), ((6, 0, 5, 4), good, "not ascending"), ((0, 9, 5, 4), good, "not ascending")]
    for rect, quad, word in cases:
        rc, _p = _from_quad(lib, rect, quad)
        assert rc == -1 and "cvs_perspective_from_quad" in _lib.last_error() and word in _lib.last_error(), (rect, quad, _lib.last_error())
    for filt in (2, -1):
        rc, _p = _from_quad(lib, RECT, good, filt)
        assert rc == -1 and "filter" in _lib.last_error()
    r = (C.c_double * 4)(*RECT)
    q = ((C.c_double * 2) * 4)()
    p = _lib.perspective()
    assert lib.cvs_perspective_from_quad(None, q, 1, C.byref(p)) == -1 and "need" in _lib.last_error()
    assert lib.cvs_perspective_from_quad(r, None, 1, C.byref(p)) == -1 and lib.cvs_perspective_from_quad(r, q, 1, None) == -1


# ---------------------------------------------------------------- the windows

def _windows(lib, triple, filt, S, target_full, window):
    from canvas_amd import _lib
    box = _lib.box2i.of
    p = _lib.perspective(*triple, filter=filt)
    win, need = box(0, 0, -1, -1), box(0, 0, -1, -1)
    assert lib.cvs_perspective_target_window(C.byref(p), C.byref(box(*S)), C.byref(box(*target_full)), C.byref(win)) == 0
    assert lib.cvs_perspective_source_window(C.byref(p), C.byref(box(*window)), C.byref(need)) == 0
    return (None if win.is_empty() else win.tuple()), need.tuple()


@pytest.mark.parametrize("name,quad", QUADS, ids=[q[0] for q in QUADS])
def test_windows_are_the_models(lib, name, quad):
    for d in ((0, 0), FAR):
        rect = (RECT[0] + d[0], RECT[1] + d[1], RECT[2] + d[0], RECT[3] + d[1])
        triple = pm.from_quad(rect, _moved(quad, *d))
        mv = lambda b: (b[0] + d[0], b[1] + d[1], b[2] + d[0], b[3] + d[1])
        for filt in (pm.NEAREST, pm.BILINEAR):
            for S in (BOX, (5, 2, 5, 2), (4, 3, 20, 9)):
                for tfull in ((-60, -60, 90, 90), (0, 0, 20, 10), (200, 200, 220, 220)):
                    for window in ((0, 0, 63, 63), (-5, 7, 11, 8)):
                        got = _windows(lib, triple, filt, mv(S), mv(tfull), mv(window))
                        want = (pm.target_window(triple, filt, mv(S), mv(tfull)), pm.source_window(triple, mv(window)))
                        assert got == want, (name, d, filt, S, tfull, window, got, want)


def test_a_window_on_the_vanishing_line_gives_the_whole_range(lib):
    """h = (1,0,0, 0,1,0, 0.1,0,1): w = 1 + 0.1 x vanishes at x = -10.  Seen from the source, S = (0,0)-(63,15) reaches the line
    u = 10 where 1/w vanishes, so its picture is unbounded: the target window is target_full.  A target window that reaches
    x <= -10 may ask for any source pixel."""
    triple = ((1, 0, 0, 0, 1, 0, F32(0.1), 0, 1), (0, 0), (0, 0))
    S, tfull = (0, 0, 63, 15), (-40, -20, 40, 20)
    for filt in (pm.NEAREST, pm.BILINEAR):
        win, need = _windows(lib, triple, filt, S, tfull, tfull)
        assert win == tfull == pm.target_window(triple, filt, S, tfull)
        assert need == pm.WHOLE == pm.source_window(triple, tfull)
        # on the near side of both lines the windows are bounded
        win, need = _windows(lib, triple, filt, (0, 0, 7, 15), tfull, (-9, -20, 40, 20))
        assert win == pm.target_window(triple, filt, (0, 0, 7, 15), tfull) and win != tfull
        assert need == pm.source_window(triple, (-9, -20, 40, 20)) and need != pm.WHOLE
        win, need = _windows(lib, triple, filt, S, tfull, (-10, 0, 0, 0))
        assert need == pm.WHOLE


def _draw(rng):
    """One convex quad of the generator DESIGN.md "Corner pin" states: (source box, S, quad)"""
    rw, rh = int(rng.integers(2, 60)), int(rng.integers(2, 40))
    x0, y0 = int(rng.integers(-100, 41)), int(rng.integers(-100, 61))
    box = (x0, y0, x0 + rw - 1, y0 + rh - 1)
    angle, scale = rng.uniform(0.0, 2.0 * math.pi), math.exp(rng.uniform(-1.5, 1.5))
    cx, cy = rng.uniform(-100.0, 100.0, 2)
    c, s = math.cos(angle), math.sin(angle)
    quad = []
    for hx, hy in ((-rw / 2, -rh / 2), (rw / 2, -rh / 2), (rw / 2, rh / 2), (-rw / 2, rh / 2)):
        r, t = 0.35 * min(rw, rh) * scale * math.sqrt(rng.uniform()), rng.uniform(0.0, 2.0 * math.pi)
        quad.append((cx + scale * (c * hx - s * hy) + r * math.cos(t), cy + scale * (s * hx + c * hy) + r * math.sin(t)))
    if rng.uniform() < 0.3:
        quad = [quad[k] for k in (1, 0, 3, 2)]
    a, b = sorted(rng.integers(box[0], box[2] + 1, 2)), sorted(rng.integers(box[1], box[3] + 1, 2))
    return box, (int(a[0]), int(b[0]), int(a[1]), int(b[1])), quad


def _taps(u, v, w, filt):
    """per pixel the tap coordinates (float32 planes) of the f32 pixel rule, and which pixels sample at all"""
    with np.errstate(all="ignore"):
        if filt == pm.NEAREST:
            i, j = np.floor((u + F32(0.5)).astype(F32)), np.floor((v + F32(0.5)).astype(F32))
            return [(i, j)], w > 0
        i, j = np.floor(u), np.floor(v)
        return [(i, j), (i + F32(1), j), (i, j + F32(1)), (i + F32(1), j + F32(1))], w > 0


def test_the_margins_hold_against_the_pixel_rule_by_brute_force(lib):
    """600 quads of the generator, none skipped.  No pixel with a tap in S lies outside the target window; no tap of a 64 x 64
    tile that lies in the source rectangle lies outside the source window.  The smallest slack found is in DESIGN.md.  The map
    and the windows walked are the library's: each is the model's, bit for bit, on every draw."""
    rng = np.random.default_rng(20261019)
    slack_t, slack_s, folded_t, folded_s, sampled = 10 ** 9, 10 ** 9, 0, 0, 0
    huge = (-2000, -2000, 2000, 2000)
    for n in range(600):
        box, S, quad = _draw(rng)
        assert all(abs(v) <= 300 for q in quad for v in q), quad
        filt = n & 1
        p = pm.from_quad(pm.outer(box), quad)
        assert p is not None, (n, quad)                               # every draw is convex: nothing is left out
        _h, to, so = p
        rc, made = _from_quad(lib, pm.outer(box), quad, filt)
        assert rc == 0 and _triple(made) == p, (n, _triple(made), p)
        win = pm.target_window(p, filt, S, huge)
        if win == huge:
            folded_t += 1
        else:
            region = (win[0] - 8, win[1] - 8, win[2] + 8, win[3] + 8)
            u, v, w = pm.source_coords(p, region)
            taps, front = _taps(u, v, w, filt)
            rel = (S[0] - so[0], S[1] - so[1], S[2] - so[0], S[3] - so[1])
            hit = np.zeros(u.shape, bool)
            for i, j in taps:
                hit |= pm.tm.inside(i, j, rel)
            hit &= front
            if hit.any():                                             # (a strongly reduced S may fall between the samples)
                sampled += 1
                ys, xs = np.nonzero(hit)
                xs, ys = xs + region[0], ys + region[1]
                slack_t = min(slack_t, xs.min() - win[0], win[2] - xs.max(), ys.min() - win[1], win[3] - ys.max())
        # a 64 x 64 tile of the target that holds the quad's first corner
        tx, ty = int(math.floor(quad[0][0])) - int(rng.integers(0, 64)), int(math.floor(quad[0][1])) - int(rng.integers(0, 64))
        tile = (tx, ty, tx + 63, ty + 63)
        need = pm.source_window(p, tile)
        assert _windows(lib, p, filt, S, huge, tile) == (win, need), (n, win, need)
        if need == pm.WHOLE:
            folded_s += 1
        else:
            u, v, w = pm.source_coords(p, tile)
            taps, front = _taps(u, v, w, filt)
            assert front.all()
            rel = (box[0] - so[0], box[1] - so[1], box[2] - so[0], box[3] - so[1])
            for i, j in taps:
                ok = pm.tm.inside(i, j, rel)
                if ok.any():
                    ii, jj = i[ok].astype(np.int64) + so[0], j[ok].astype(np.int64) + so[1]
                    slack_s = min(slack_s, ii.min() - need[0], need[2] - ii.max(), jj.min() - need[1], need[3] - jj.max())
    print("smallest slack: target window %d, source window %d; windows on the vanishing line: %d target, %d source" % (slack_t, slack_s, folded_t, folded_s))
    assert slack_t >= 0 and slack_s >= 0
    assert folded_t < 300 and folded_s < 300 and sampled > 300       # (most draws exercise the margins)


# ---------------------------------------------------------------- refusals of the device entries

def test_entries_refuse_before_anything_is_launched(lib):
    from canvas_amd import _lib
    from canvas_amd.abi import HostFrame
    full = (0, 0, 7, 7)
    lim, span = _lib.MAX_COORD, _lib.PERSPECTIVE_MAX_SPAN
    nan, inf = float("nan"), float("inf")
    ident = (1, 0, 0, 0, 1, 0, 0, 0, 1)
    for name, dtype, frame_t in (("cvs_perspective_f16_dev", np.uint16, _lib.rgba_frame_f16), ("cvs_perspective_f32_dev", np.float32, _lib.rgba_frame_f32)):
        entry = getattr(lib, name)

        def refused(target, source, p, word):
            lib.cvs_clear_last_error()
            assert entry(target, source, p, None) == -1, (name, word)
            assert name in _lib.last_error() and word in _lib.last_error(), (name, word, _lib.last_error())

        def fresh():
            return HostFrame(full, dtype, current_window=full)
        good, ok = fresh(), _lib.perspective()
        cases = [(None, "need")]
        cases += [(_lib.perspective(filter=f), "filter") for f in (2, -1, 7)]
        cases += [(_lib.perspective(flags=f), "unknown flags") for f in (1, 2, -1, 0x100)]
        for k in range(9):
            for bad in (nan, inf, -inf):
                cases.append((_lib.perspective(ident[:k] + (bad,) + ident[k + 1:]), "not finite"))
        cases += [(_lib.perspective(h), "determinant") for h in ((0,) * 9, (1, 2, 0, 2, 4, 0, 0, 0, 1), (1, 0, 0, 0, 1, 0, 0, 0, 0), (1, 2, 3, 4, 5, 6, 7, 8, 9))]
        cases += [(_lib.perspective(target_origin=o), "beyond") for o in ((span + 1, 0), (0, -span - 1), (7 - span - 1, 0), (lim, lim), (-2 ** 31, 0), (0, 2 ** 31 - 1))]
        cases += [(_lib.perspective(source_origin=o), "beyond") for o in ((span + 1, 0), (0, -span - 1), (0, 7 - span - 1), (lim, lim), (-2 ** 31, 0), (0, 2 ** 31 - 1))]
        for p, word in cases:
            out = fresh()
            refused(out.ref(), good.ref(), None if p is None else C.byref(p), word)
            assert out.current_window.is_empty(), word
        out = fresh()
        refused(out.ref(), None, C.byref(ok), "need")
        assert out.current_window.is_empty()
        refused(None, good.ref(), C.byref(ok), "need")
        out, outside = fresh(), HostFrame(full, dtype, current_window=(0, 0, 8, 7))
        refused(out.ref(), outside.ref(), C.byref(ok), "outside its buffer")
        assert out.current_window.is_empty()
        # coordinates beyond the bound: frames that describe buffers nobody allocates (nothing is dereferenced)
        box = _lib.box2i.of
        far = frame_t(good.c.data, box(lim - 6, 0, lim + 1, 7), box(lim - 6, 0, lim + 1, 7))
        out = fresh()
        refused(out.ref(), C.byref(far), C.byref(_lib.perspective(source_origin=(lim, 0))), "beyond")
        assert out.current_window.is_empty()
        far = frame_t(good.c.data, box(0, -lim - 1, 7, -lim + 6), box(0, 0, 7, 7))
        refused(C.byref(far), good.ref(), C.byref(_lib.perspective(target_origin=(0, -lim))), "beyond")
        assert far.current_window.is_empty() and good.current_window.tuple() == full       # a refused call leaves its source alone
        # the span is that of the target's full window and of S: an origin on the bound itself is accepted up to the device
        both = fresh()
        refused(both.ref(), both.ref(), C.byref(ok), "not in place")
        assert both.current_window.is_empty()
        if lib.cvs_device_count() == 0:
            # without a device a call that nothing refuses still fails, loudly, and computes nothing on the CPU
            for p in (ok, _lib.perspective(target_origin=(span, 7 - span), source_origin=(-span + 7, span))):
                lib.cvs_clear_last_error()
                out = HostFrame(full, dtype, current_window=full)
                assert entry(out.ref(), good.ref(), C.byref(p), None) != 0 and "no CPU path" in _lib.last_error(), _lib.last_error()
                assert out.current_window.is_empty()


def test_window_functions_refuse_as_the_entries_do(lib):
    from canvas_amd import _lib
    box = _lib.box2i.of
    b = box(0, 0, 7, 7)
    for p, word in ((_lib.perspective(filter=3), "filter"), (_lib.perspective(flags=1), "unknown flags"),
                    (_lib.perspective((1, 0, 0, 0, 1, 0, 0, float("nan"), 1)), "not finite"), (_lib.perspective((0,) * 9), "determinant")):
        win = box(1, 1, 2, 2)
        assert lib.cvs_perspective_target_window(C.byref(p), C.byref(b), C.byref(b), C.byref(win)) == -1 and word in _lib.last_error() and win.is_empty()
        win = box(1, 1, 2, 2)
        assert lib.cvs_perspective_source_window(C.byref(p), C.byref(b), C.byref(win)) == -1 and word in _lib.last_error() and win.is_empty()
    ok, win = _lib.perspective(), box(1, 1, 2, 2)
    assert lib.cvs_perspective_target_window(None, C.byref(b), C.byref(b), C.byref(win)) == -1 and win.is_empty()
    assert lib.cvs_perspective_source_window(C.byref(ok), None, C.byref(win)) == -1
    empty = box(0, 0, -1, -1)
    assert lib.cvs_perspective_target_window(C.byref(ok), C.byref(empty), C.byref(b), C.byref(win)) == 0 and win.is_empty()
    assert lib.cvs_perspective_source_window(C.byref(ok), C.byref(empty), C.byref(win)) == 0 and win.is_empty()


# ---------------------------------------------------------------- the catalogue

def test_every_device_entry_of_the_header_has_its_catalogue_cases():
    """What tests/test_entry_cases_cpu.py holds tests/entry_cases.py to, for tests/perspective_cases.py: every cvs_*_dev entry the
    header declares is CALLED by a case, each call is handed the factory's stream, every case has an output and asks for the same
    operands every time, and the Shifted factory moves every frame AND both origins and changes no buffer and no coefficient, so
    the far-window harness runs the cases as it runs the catalogue's."""
    from canvas_amd import _lib
    from tests import entry_cases as ec
    from tests import perspective_cases as pc
    from tests.test_entry_cases_cpu import OFFSET, Geometry, HostOnly, Recorder, _check_shifted
    _funcs, entries = _declared(HEADER)
    assert entries == sorted(pc.ENTRIES)
    seen, stream, cases = {}, 0x5EED, 0
    for gid, build in pc.GROUPS:
        rec = Recorder()
        for what, case in build(rec):
            cases += 1
            before = len(rec.calls)
            fac = HostOnly(rec, stream)
            assert case(fac) == 0
            made = rec.calls[before:]
            assert len(made) == 1 and made[0][1] == stream, (gid, what, made)
            seen.setdefault(made[0][0], []).append(what)
            assert any(o.out for o in fac.objects) and all(o.frame is not None for o in fac.objects) and len(fac.objects) == 2, (gid, what)
            again = HostOnly(rec, stream)
            case(again)
            spec = lambda f: [(o.cls, o.name, o.out, o.cmp, o.nbytes, o.row_bytes, o.reads) for o in f.objects]
            assert spec(fac) == spec(again), (gid, what)
            boxes = [(o.out, o.frame.c.full_window.tuple()) for o in fac.objects if o.frame is not None]
            assert len(ec.far_offsets(pc.FAR_RULE, boxes)) >= 4, (gid, what)
    assert sorted(seen) == entries and len(seen["cvs_perspective_f16_dev"]) == len(seen["cvs_perspective_f32_dev"]) == 36 and cases == 72
    for word in ("half-pixel shift", "keystone", "general", "nearest", "bilinear"):
        assert any(word in w for w in seen["cvs_perspective_f16_dev"]), word
    frames = 0
    for gid, build in pc.GROUPS:
        a, b = Geometry(), Geometry()
        for (what, near), (_, far) in zip(build(a), build(b)):
            frames += _check_shifted(gid, what, (near, far, a, b), pc.FAR_RULE["source_scale"])
    assert frames == 2 * cases                                       # two frame arguments per call

    # the origins move with the frames, the coefficients do not
    class Params(Recorder):
        def __getattr__(self, name):
            def call(*args):
                p = args[2]._obj
                self.calls.append((tuple(p.h), tuple(p.target_origin), tuple(p.source_origin), p.filter, p.flags))
                return 0
            return call
    for gid, build in pc.GROUPS:
        near, far = Params(), Params()
        for (what, a), (_, b) in zip(build(near), build(far)):
            a(HostOnly(near, 1))
            b(ec.Shifted(HostOnly(far, 1), OFFSET))
        assert len(near.calls) == len(far.calls) == 36
        for n, f in zip(near.calls, far.calls):
            assert f[0] == n[0] and f[3:] == n[3:] and n[4] == 0
            assert f[1] == (n[1][0] + OFFSET[0], n[1][1] + OFFSET[1]) and f[2] == (n[2][0] + OFFSET[0], n[2][1] + OFFSET[1])
            assert not (n[0][6] == 0 and n[0][7] == 0) or n[0][8] == 1
        assert any(n[0][6] != 0 or n[0][7] != 0 for n in near.calls)
