"""The scopes' catalogue of device-entry calls, in the form of tests/entry_cases.py: a case is a function case(fac) that makes
ONE call of cvs_scope_counts_f16_dev or cvs_scope_render_f16_dev (include/canvas_scope.h) on operands it takes from a factory,
in the same order every time, on the stream fac.stream, and returns the entry's return code.  So the harnesses that run the
catalogue -- frames packed into a guarded arena, a stream that records and replays, windows far from the origin -- run these
calls with no harness code of their own (tests/test_scope_harness_gpu.py), and tests/test_scope_cpu.py holds the cases to the
header without a GPU.  Every box a case hands comes from fac.box(): the region inside the struct, and the place."""
import ctypes as C

import numpy as np

from canvas_amd import _lib
from tests.entry_cases import _ANY, DISPLAY_GEOMETRIES, PAD, all_codes, blank

KINDS = [("histogram", _lib.SCOPE_HISTOGRAM), ("waveform", _lib.SCOPE_WAVEFORM), ("parade", _lib.SCOPE_PARADE), ("vectorscope", _lib.SCOPE_VECTORSCOPE)]
ENTRIES = ("cvs_scope_counts_f16_dev", "cvs_scope_render_f16_dev")
RENDER_TARGET = (1, 20, 12, 90)              # smaller than every picture placed at RENDER_PLACE
RENDER_PLACE = (-2, -5)
# far from the origin a scope gives the origin's result byte for byte: columns are counted from region.min.x, and the region, the
# place and the frames move together (tests/entry_cases.py FAR_CLASSES: "equivariant", any offset within CVS_MAX_COORD)
FAR_RULE = _ANY


def count(kind, columns):
    """cvs_scope_count, restated: the cases are also built against stand-ins for the library."""
    return {_lib.SCOPE_HISTOGRAM: 5 * 256, _lib.SCOPE_WAVEFORM: columns * 256, _lib.SCOPE_PARADE: 3 * columns * 256, _lib.SCOPE_VECTORSCOPE: 256 * 256}[kind]


def picture_size(kind, columns):
    return {_lib.SCOPE_WAVEFORM: (columns, 256), _lib.SCOPE_PARADE: (3 * columns, 256), _lib.SCOPE_VECTORSCOPE: (256, 256)}[kind]


def scopes(cvs, kind):
    """Counts of all_codes frames over the display geometries -- the region reaches past the current window on the left and
    below where the buffer does, and ends inside it on the right; 7 columns through the widget's table, one column per pixel of
    the window through the exporter's and without the transparent pixels -- and, for the kinds that have a picture, one render of
    a table of small counters into a target that every side of the picture but the left one overhangs."""
    cases = []
    for full, cur in DISPLAY_GEOMETRIES:
        width = cur[2] - cur[0] + 1
        region = (max(cur[0] - 2, full[0]), cur[1], cur[2] - (1 if width > 1 else 0), min(cur[3] + 3, full[3]))       # inside the buffer's box: it moves with it
        for columns in (7, width):
            def counts(fac, full=full, cur=cur, region=region, columns=columns):
                frame = fac.frame(all_codes(full, cur))
                table = fac.buffer(np.full(count(kind, columns) * 4, PAD, np.uint8), "bytes", out=True, name="count table")
                widget = columns == 7
                p = _lib.scope(kind, fac.box(*region), columns=columns, pre_lut=_lib.LUT_LINEAR_TO_SRGB if widget else _lib.LUT_NONE,
                               rendering_intent=1.25 if widget else 0.0, flags=0 if widget else _lib.SCOPE_SKIP_TRANSPARENT)
                return cvs.cvs_scope_counts_f16_dev(table, frame.ref(), C.byref(p), fac.stream)
            cases.append(("scope counts, kind %d, %d columns %r" % (kind, columns, (full, cur)), counts))
    if kind != _lib.SCOPE_HISTOGRAM:
        columns = 7
        size = picture_size(kind, columns)

        def render(fac):
            n = count(kind, columns)
            counters = (np.arange(n, dtype=np.uint64) * 2654435761 % 41).astype(np.uint32)
            table = fac.buffer(counters, "bytes", name="count table")
            target = fac.frame(blank(True, RENDER_TARGET), out=True, name="scope picture")
            x0, y0 = RENDER_PLACE
            place = fac.box(x0, y0, x0 + size[0] - 1, y0 + size[1] - 1)
            p = _lib.scope(kind, fac.box(0, 0, 0, 0), columns=columns)
            return cvs.cvs_scope_render_f16_dev(target.ref(), C.byref(place), table, C.byref(p), C.c_float(1.0 / 16.0), fac.stream)
        cases.append(("scope render, kind %d, %d columns" % (kind, columns), render))
    return cases


GROUPS = [("scopes[%s]" % name, lambda cvs, kind=kind: scopes(cvs, kind)) for name, kind in KINDS]
