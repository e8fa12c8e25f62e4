"""The Catmull-Rom filter's catalogue of device-entry calls, in the form of tests/perspective_cases.py: a case is a function
case(fac) that makes ONE call of cvs_transform_f16_dev / _f32_dev (include/canvas_hip.h) or cvs_perspective_f16_dev / _f32_dev
(include/canvas_perspective.h) with filter CVS_TRANSFORM_CATMULL_ROM on operands it takes from a factory, in the same order every
time, on the stream fac.stream, and returns the entry's return code.  So the harnesses that run the catalogue -- frames packed
into a guarded arena, a stream that records and replays, windows far from the origin -- run these calls with no harness code of
their own (tests/test_cubic_harness_gpu.py), and tests/test_cubic_cpu.py holds the cases to the headers without a GPU.

Geometry goes through the factory: the affine coefficients through fac.matrix, the corner pin's two origins through fac.box
(tests/perspective_cases.py params), so that a factory which moves the frames moves them too.  Far from the origin the corner
pin gives the origin's bytes (FAR_RULE["perspective"], equivariant); the affine warp forms positions from absolute coordinates in
float and is compared with tests/cubic_model.py at the same far arguments, inside the transform's own bound
(FAR_RULE["transform"])."""
import ctypes as C
import math

import numpy as np

from canvas_amd import _lib
from tests import perspective_cases as pc
from tests import perspective_model as pm
from tests.entry_cases import _ANY, blank, px

ENTRIES = ("cvs_transform_f16_dev", "cvs_transform_f32_dev", "cvs_perspective_f16_dev", "cvs_perspective_f32_dev")
WIDTHS = [31, 33, 65]
HEIGHTS = (7, 9)
FAR_RULE = {"transform": dict(_ANY, limit=_lib.TRANSFORM_MAX_COORD), "perspective": _ANY}
FILTER = _lib.TRANSFORM_CATMULL_ROM


def source_of(tw, th):
    """A source smaller than the target whose window is its whole buffer: a clamped tap sits on the allocation's first and last pixel"""
    return (3, 1, tw - 6, th - 2)


def affine_maps(tw, th, sfull):
    """(name, m): a half-pixel shift, 30 degrees, a reduction to half, an enlargement to double and a mirror, the last four about
    the centres of the target and the source"""
    cx, cy = (tw - 1) / 2.0, (th - 1) / 2.0
    sx, sy = (sfull[0] + sfull[2]) / 2.0, (sfull[1] + sfull[3]) / 2.0
    c, s = math.cos(math.radians(30.0)), math.sin(math.radians(30.0))
    return [("half-pixel shift", (1.0, 0.0, 0.5, 0.0, 1.0, 0.5)),
            ("30 degrees", (c, -s, sx - c * cx + s * cy, s, c, sy - s * cx - c * cy)),
            # (off the samples by a fraction: about the centres alone a reduction to half would only copy)
            ("half size", (2.0, 0.0, sx - 2.0 * cx + 0.25, 0.0, 2.0, sy - 2.0 * cy + 0.375)),
            ("double size", (0.5, 0.0, sx - 0.5 * cx + 0.125, 0.0, 0.5, sy - 0.5 * cy)),
            ("mirror", (-1.0, 0.0, sx + cx, 0.0, 1.0, sy - cy))]


def transform(cvs, half):
    cases = []
    for tw in WIDTHS:
        for th in HEIGHTS:
            tfull, sfull = (0, 0, tw - 1, th - 1), source_of(tw, th)
            for name, m in affine_maps(tw, th, sfull):
                def case(fac, tw=tw, th=th, tfull=tfull, sfull=sfull, m=m):
                    t = _lib.transform(fac.matrix(m), FILTER)
                    rng = np.random.default_rng(2700 + tw + th)
                    src = fac.frame(px(rng, half, sfull))
                    out = fac.frame(blank(half, tfull), out=True, cmp="f16" if half else "f32")
                    entry = cvs.cvs_transform_f16_dev if half else cvs.cvs_transform_f32_dev
                    return entry(out.ref(), src.ref(), C.byref(t), fac.stream)
                cases.append(("cubic transform %dx%d %s" % (tw, th, name), case))
    return cases


def perspective(cvs, half):
    cases = []
    for tw in WIDTHS:
        for th in HEIGHTS:
            tfull, sfull = (0, 0, tw - 1, th - 1), source_of(tw, th)
            for name, quad in pc.quads(tw, th, pm.outer(sfull)):
                def case(fac, tw=tw, th=th, tfull=tfull, sfull=sfull, quad=quad):
                    p = pc.params(fac, pm.outer(sfull), quad, FILTER)
                    rng = np.random.default_rng(2800 + tw + th)
                    src = fac.frame(px(rng, half, sfull))
                    out = fac.frame(blank(half, tfull), out=True, cmp="f16" if half else "f32")
                    entry = cvs.cvs_perspective_f16_dev if half else cvs.cvs_perspective_f32_dev
                    return entry(out.ref(), src.ref(), C.byref(p), fac.stream)
                cases.append(("cubic perspective %dx%d %s" % (tw, th, name), case))
    return cases


def warp_of(gid):
    """"transform" or "perspective": which of the two warps a group calls, and so which far rule its cases follow"""
    return gid.split("[")[0].split("_")[1]


GROUPS = [("cubic_%s[%s]" % (fn.__name__, name), lambda cvs, fn=fn, half=half: fn(cvs, half))
          for fn in (transform, perspective) for name, half in (("f16", True), ("f32", False))]
