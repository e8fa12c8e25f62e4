"""The adaptive deinterlacer's catalogue of device-entry calls, in the form of tests/entry_cases.py and tests/perspective_cases.py:
a case is a function case(fac) that makes ONE call of cvs_deinterlace_adaptive_f16_dev (include/canvas_deinterlace.h) on operands
it takes from a factory, in the same order every time, on the stream fac.stream, and returns the entry's return code.  So the
harnesses that run the catalogue -- frames packed into a guarded arena, a stream that records and replays, windows far from the
origin -- run these calls with no harness code of their own (tests/test_deinterlace_harness_gpu.py), and
tests/test_deinterlace_cpu.py holds the cases to the header without a GPU.

The pictures are tests/deinterlace_model.py's thirds, so that every class of the weight is met in every case that has a
neighbour; the first case has both neighbours, so that the harness which bends one operand at a time finds every operand."""
import ctypes as C

import numpy as np

from canvas_amd import _lib
from canvas_amd.abi import HostFrame
from tests import deinterlace_model as dm
from tests.entry_cases import _EVEN, blank

ENTRIES = ("cvs_deinterlace_adaptive_f16_dev",)
WIDTHS = [31, 33, 65]
HEIGHTS = [7, 9]
THRESHOLD, SOFTNESS = 0.05, 0.1
# row parity is that of the absolute coordinate: far from the origin the entry gives the origin's bytes where the rows keep
# their parity (tests/entry_cases.py FAR_CLASSES: "even dy", any offset within CVS_MAX_COORD)
FAR_RULE = _EVEN


def adaptive(cvs):
    """Frames of 31, 33 and 65 columns x 7 and 9 rows, both fields, with two, one (prev, then next) and no neighbours; the
    nine-row cases write into a buffer that lies one column left of and one row below the input's."""
    cases = []
    for w in WIDTHS:
        for h in HEIGHTS:
            full = (0, 0, w - 1, h - 1)
            tfull = full if h == 7 else (-1, 1, w - 2, h)
            for field in (0, 1):
                for which in ("both", "prev" if field == 0 else "next", "none"):
                    def case(fac, w=w, h=h, full=full, tfull=tfull, field=field, which=which):
                        rng = np.random.default_rng(1300 + w + h)
                        prev, cur, nxt = (HostFrame(full, np.uint16, codes, full) for codes in dm.thirds(rng, full, THRESHOLD, SOFTNESS))
                        a = fac.frame(prev) if which in ("both", "prev") else None
                        b = fac.frame(cur)
                        c = fac.frame(nxt) if which in ("both", "next") else None
                        out = fac.frame(blank(True, tfull), out=True, cmp="f16")
                        p = _lib.deinterlace_adaptive(field, THRESHOLD, SOFTNESS)
                        return cvs.cvs_deinterlace_adaptive_f16_dev(out.ref(), a.ref() if a else None, b.ref(), c.ref() if c else None, C.byref(p), fac.stream)
                    cases.append(("adaptive %dx%d field %d neighbours %s" % (w, h, field, which), case))
    return cases


GROUPS = [("deinterlace_adaptive", adaptive)]
