"""The corner pin's catalogue of device-entry calls, in the form of tests/entry_cases.py and tests/lut3d_cases.py: a case is a
function case(fac) that makes ONE call of cvs_perspective_f16_dev or cvs_perspective_f32_dev (include/canvas_perspective.h) on
operands it takes from a factory, in the same order every time, on the stream fac.stream, and returns the entry's return code.  So
the harnesses that run the catalogue -- frames packed into a guarded arena, a stream that records and replays, windows far from
the origin -- run these calls with no harness code of their own (tests/test_perspective_harness_gpu.py), and
tests/test_perspective_cpu.py holds the cases to the header without a GPU.

The two origins of the cvs_perspective are taken through fac.box, so that a factory which moves the frames (entry_cases.Shifted)
moves them too: h is the same nine floats wherever the frames lie, which is what makes the far result the origin's, byte for
byte."""
import ctypes as C

import numpy as np

from canvas_amd import _lib
from tests import perspective_model as pm
from tests.entry_cases import _ANY, blank, px

ENTRIES = ("cvs_perspective_f16_dev", "cvs_perspective_f32_dev")
WIDTHS = [31, 33, 65]
# positions are formed relative to origins that move with the frames: far from the origin the entries give the origin's bytes
# (tests/entry_cases.py FAR_CLASSES: "equivariant", any offset within CVS_MAX_COORD)
FAR_RULE = _ANY


def quads(tw, th, rect):
    """(name, quad) for a target of tw x th pixels and the source rectangle `rect` (outer edges): where the rectangle's
    top-left, top-right, bottom-right and bottom-left corners land"""
    w, h = float(tw), float(th)
    shifted = [(x + 0.5, y + 0.5) for x, y in pm.rect_quad(rect)]
    keystone = [(0.2 * w - 0.5, 0.5), (0.8 * w - 0.5, 0.5), (w - 0.5, h - 1.5), (-0.5, h - 1.5)]            # top edge 0.6 of the bottom
    general = [(0.11 * w, 0.3), (0.93 * w, 1.4), (0.78 * w, h - 0.8), (0.02 * w + 1.0, h - 2.1)]
    return [("half-pixel shift", shifted), ("keystone", keystone), ("general", general)]


def params(fac, rect, quad, filt):
    """The cvs_perspective of the quad, its origins moved by the factory"""
    h, to, so = pm.from_quad(rect, quad)
    t, s = fac.box(to[0], to[1], to[0], to[1]), fac.box(so[0], so[1], so[0], so[1])
    return _lib.perspective(h, (t.min.x, t.min.y), (s.min.x, s.min.y), filt)


def perspective(cvs, half):
    """Targets of 31, 33 and 65 columns x 7 and 9 rows; a source smaller than the target whose window is its whole buffer, so
    that a clamped tap sits on the allocation's first and last pixel."""
    cases = []
    for tw in WIDTHS:
        for th in (7, 9):
            tfull = (0, 0, tw - 1, th - 1)
            sfull = (3, 1, tw - 6, th - 2)
            for name, quad in quads(tw, th, pm.outer(sfull)):
                for filt in (_lib.TRANSFORM_NEAREST, _lib.TRANSFORM_BILINEAR):
                    def case(fac, tw=tw, th=th, tfull=tfull, sfull=sfull, quad=quad, filt=filt):
                        p = params(fac, pm.outer(sfull), quad, filt)
                        rng = np.random.default_rng(1200 + tw + th)
                        src = fac.frame(px(rng, half, sfull))
                        out = fac.frame(blank(half, tfull), out=True, cmp="f16" if half else "f32")
                        entry = cvs.cvs_perspective_f16_dev if half else cvs.cvs_perspective_f32_dev
                        return entry(out.ref(), src.ref(), C.byref(p), fac.stream)
                    cases.append(("perspective %dx%d %s %s" % (tw, th, name, "bilinear" if filt else "nearest"), case))
    return cases


GROUPS = [("perspective[%s]" % name, lambda cvs, half=half: perspective(cvs, half)) for name, half in (("f16", True), ("f32", False))]
