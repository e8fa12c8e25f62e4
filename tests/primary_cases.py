"""The primary colour corrector's catalogue of device-entry calls, in the form of tests/entry_cases.py and tests/lut3d_cases.py: a
case is a function case(fac) that makes ONE call of cvs_primary_f16_dev or cvs_primary_f32_dev (include/canvas_primary.h) on
operands it takes from a factory, in the same order every time, on the stream fac.stream, and returns the entry's return code.  So
the harnesses that run the catalogue -- frames packed into a guarded arena, a stream that records and replays, windows far from
the origin -- run these calls with no harness code of their own (tests/test_primary_harness_gpu.py), and
tests/test_primary_cpu.py holds the cases to the header without a GPU.

A curve set is a flat buffer of the class "f32": it lies on a 16-byte boundary, as an f32 pixel does, so the arena places it at
that class's residues (0, 16, 48, 144 modulo 256) with guards around it.  The "bytes" residues (4, 12) are addresses the contract
refuses."""
import ctypes as C

import numpy as np

from canvas_amd import _lib
from tests import primary_model as pm
from tests.entry_cases import _ANY, DISPLAY_GEOMETRIES, _stream_geometries, all_codes, blank, px

ENTRIES = ("cvs_primary_f16_dev", "cvs_primary_f32_dev")
WIDTHS = [1, 2, 129, 130]
# a per-pixel map: far from the origin it gives the origin's bytes (tests/entry_cases.py FAR_CLASSES: "equivariant", any offset
# within CVS_MAX_COORD)
FAR_RULE = _ANY
MATRIX = [0.75, 0.5, -0.25, 0.0625, 0.0, -1.0, 2.0, 0.0, 0.3, 0.3, 0.3, -0.2]
# (pre, matrix?, post): sizes and domains; every one of the seven combinations, table sizes whose tables are no multiple of 16 bytes,
# and the fullest call, 4097 + 4097 nodes: 98 328 bytes of LDS, the launch that asks for more dynamic LDS than the default allows
# and runs one workgroup a CU
STAGES = [((5, pm.UNIT), True, (17, pm.WIDE)), ((1025, pm.SKEWED), False, None), (None, True, None), (None, False, (3, pm.SKEWED)),
          ((2, pm.WIDE), True, None), (None, True, (1024, pm.UNIT)), ((17, pm.SKEWED), False, (5, pm.WIDE)), ((4097, pm.SKEWED), True, (4097, pm.WIDE))]


def _entry(cvs, half):
    return cvs.cvs_primary_f16_dev if half else cvs.cvs_primary_f32_dev


def _params(stages):
    pre, matrix, post = stages
    return _lib.primary((pre[0],) + pre[1] if pre else None, MATRIX if matrix else None, (post[0],) + post[1] if post else None)


def _tables(fac, stages):
    """the device pointers of the two stages (None for an absent one), taken from the factory pre first"""
    pre, _, post = stages
    return (fac.buffer(pm.distinct(pre[0], pre[1], 1).planar(), "f32", name="pre") if pre else None,
            fac.buffer(pm.distinct(post[0], post[1], 2).planar(), "f32", name="post") if post else None)


def primary(cvs, half):
    """Streams of 1, 2, 129 and 130 columns over the stream geometries (odd and even first columns, an odd buffer origin, a target
    with an odd base column), out of place and -- every other case -- in place, the eight stage sets in turn (the seven combinations, and the fullest call); for halfs
    also frames that hold every half code, NaN, Inf and negatives included."""
    cases = []
    cmp = "f16" if half else "f32"
    for width in WIDTHS:
        for height in (1, 9):
            for g, (sfull, scur, tfull) in enumerate(_stream_geometries(width, height)):
                stages = STAGES[(g + height + width) % len(STAGES)]
                p = _params(stages)

                def case(fac, g=g, width=width, height=height, sfull=sfull, scur=scur, tfull=tfull, stages=stages, p=p):
                    rng = np.random.default_rng(1900 + g + height + width)
                    src = fac.frame(px(rng, half, sfull, scur))
                    out = fac.frame(blank(half, tfull), out=True, cmp=cmp)
                    pre, post = _tables(fac, stages)
                    return _entry(cvs, half)(out.ref(), src.ref(), C.byref(p), pre, post, fac.stream)
                cases.append(("primary %dx%d %r %r" % (width, height, stages, (sfull, scur, tfull)), case))
                if g % 2 == 0:
                    def in_place(fac, g=g, width=width, height=height, sfull=sfull, scur=scur, stages=stages, p=p):
                        rng = np.random.default_rng(1950 + g + height + width)
                        frame = fac.frame(px(rng, half, sfull, scur), out=True, cmp=cmp, in_place=True)
                        pre, post = _tables(fac, stages)
                        return _entry(cvs, half)(frame.ref(), frame.ref(), C.byref(p), pre, post, fac.stream)
                    cases.append(("primary in place %dx%d %r %r" % (width, height, stages, (sfull, scur)), in_place))
    if half:
        for k, (full, cur) in enumerate(DISPLAY_GEOMETRIES[1:]):
            stages = STAGES[k % len(STAGES)]
            p = _params(stages)

            def codes(fac, full=full, cur=cur, stages=stages, p=p):
                src = fac.frame(all_codes(full, cur))
                out = fac.frame(blank(True, full), out=True, cmp="f16")
                pre, post = _tables(fac, stages)
                return cvs.cvs_primary_f16_dev(out.ref(), src.ref(), C.byref(p), pre, post, fac.stream)
            cases.append(("primary all codes %r %r" % (stages, (full, cur)), codes))
    return cases


GROUPS = [("primary[%s]" % name, lambda cvs, half=half: primary(cvs, half)) for name, half in (("f16", True), ("f32", False))]
