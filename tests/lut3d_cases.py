"""The 3D LUT's catalogue of device-entry calls, in the form of tests/entry_cases.py and tests/scope_cases.py: a case is a function
case(fac) that makes ONE call of cvs_lut3d_f16_dev or cvs_lut3d_f32_dev (include/canvas_lut3d.h) on operands it takes from a
factory, in the same order every time, on the stream fac.stream, and returns the entry's return code.  So the harnesses that run
the catalogue -- frames packed into a guarded arena, a stream that records and replays, windows far from the origin -- run these
calls with no harness code of their own (tests/test_lut3d_harness_gpu.py), and tests/test_lut3d_cpu.py holds the cases to the
header without a GPU.

The lattice is a flat buffer of the class "f32": a node is 16 bytes on a 16-byte boundary, as an f32 pixel is, so the arena places
it at that class's residues (0, 16, 48, 144 modulo 256).  The "bytes" residues (4, 12) are addresses the contract refuses."""
import ctypes as C

import numpy as np

from canvas_amd import _lib
from tests import lut3d_model as lm
from tests.entry_cases import _ANY, DISPLAY_GEOMETRIES, _stream_geometries, all_codes, blank, px

ENTRIES = ("cvs_lut3d_f16_dev", "cvs_lut3d_f32_dev")
WIDTHS = [1, 2, 129, 130]
# a per-pixel map: far from the origin it gives the origin's bytes (tests/entry_cases.py FAR_CLASSES: "equivariant", any offset
# within CVS_MAX_COORD)
FAR_RULE = _ANY
# (size, domain): a domain that is not [0, 1] and differs per channel among them
TABLES = [(5, lm.UNIT), (4, ((-0.25, 0.0, 0.125), (1.5, 2.0, 0.875))), (17, ((0.0, -1.0, 0.0), (1.0, 1.0, 4.0)))]


def _entry(cvs, half):
    return cvs.cvs_lut3d_f16_dev if half else cvs.cvs_lut3d_f32_dev


def _lattice(fac, size):
    return fac.buffer(lm.packed(lm.distinct(size, size)), "f32", name="lattice")


def lut3d(cvs, half):
    """Streams of 1, 2, 129 and 130 columns over the stream geometries (odd and even first columns, an odd buffer origin, a target
    with an odd base column), out of place and -- every other case -- in place; for halfs also frames that hold every half
    code, NaN, Inf and negatives included."""
    cases = []
    cmp = "f16" if half else "f32"
    for width in WIDTHS:
        for height in (1, 9):
            for g, (sfull, scur, tfull) in enumerate(_stream_geometries(width, height)):
                size, domain = TABLES[(g + height + width) % len(TABLES)]
                p = _lib.lut3d(size, *domain)

                def case(fac, g=g, width=width, height=height, sfull=sfull, scur=scur, tfull=tfull, size=size, p=p):
                    rng = np.random.default_rng(900 + g + height + width)
                    src = fac.frame(px(rng, half, sfull, scur))
                    out = fac.frame(blank(half, tfull), out=True, cmp=cmp)
                    return _entry(cvs, half)(out.ref(), src.ref(), _lattice(fac, size), C.byref(p), fac.stream)
                cases.append(("lut3d %dx%d N=%d %r" % (width, height, size, (sfull, scur, tfull)), case))
                if g % 2 == 0:
                    def in_place(fac, g=g, width=width, height=height, sfull=sfull, scur=scur, size=size, p=p):
                        rng = np.random.default_rng(950 + g + height + width)
                        frame = fac.frame(px(rng, half, sfull, scur), out=True, cmp=cmp, in_place=True)
                        return _entry(cvs, half)(frame.ref(), frame.ref(), _lattice(fac, size), C.byref(p), fac.stream)
                    cases.append(("lut3d in place %dx%d N=%d %r" % (width, height, size, (sfull, scur)), in_place))
    if half:
        for k, (full, cur) in enumerate(DISPLAY_GEOMETRIES[1:]):
            size, domain = TABLES[k % len(TABLES)]
            p = _lib.lut3d(size, *domain)

            def codes(fac, full=full, cur=cur, size=size, p=p):
                src = fac.frame(all_codes(full, cur))
                out = fac.frame(blank(True, full), out=True, cmp="f16")
                return cvs.cvs_lut3d_f16_dev(out.ref(), src.ref(), _lattice(fac, size), C.byref(p), fac.stream)
            cases.append(("lut3d all codes N=%d %r" % (size, (full, cur)), codes))
    return cases


GROUPS = [("lut3d[%s]" % name, lambda cvs, half=half: lut3d(cvs, half)) for name, half in (("f16", True), ("f32", False))]
