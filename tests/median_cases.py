"""The median's catalogue of device-entry calls, in the form of tests/entry_cases.py and tests/deinterlace_cases.py: a case is a
function case(fac) that makes ONE call of cvs_median_f16_dev or cvs_median_f32_dev (include/canvas_median.h) on operands it takes
from a factory, in the same order every time, on the stream fac.stream, and returns the entry's return code.  So the harnesses
that run the catalogue -- frames packed into a guarded arena, a stream that records and replays, windows far from the origin --
run these calls with no harness code of their own (tests/test_median_harness_gpu.py), and tests/test_median_cpu.py holds the
cases to the header without a GPU.

The pictures are tests/median_model.py's speck picture, so that with a threshold both classes, kept and replaced, are met."""
import ctypes as C

import numpy as np

from canvas_amd import _lib
from canvas_amd.abi import HostFrame
from tests import median_model as mm
from tests.entry_cases import _ANY, blank

ENTRIES = ("cvs_median_f16_dev", "cvs_median_f32_dev")
SIZES = [(31, 7), (33, 9), (65, 7), (130, 9)]
CHANNELS = ["rgba", "rgb", "a", "ga"]
# nothing depends on coordinates: far from the origin the entries give the origin's bytes at any offset within CVS_MAX_COORD
FAR_RULE = _ANY


def source(rng, half, sfull, scur):
    """The speck picture over scur inside a buffer of junk over sfull."""
    dtype = np.uint16 if half else np.uint32
    h, w = sfull[3] - sfull[1] + 1, sfull[2] - sfull[0] + 1
    codes = rng.integers(0, 0x3C01 if half else 0x3F800001, (h, w, 4)).astype(dtype)
    mm.crop(codes, sfull, scur)[...] = mm.speck_picture(rng, scur[2] - scur[0] + 1, scur[3] - scur[1] + 1, dtype)
    return HostFrame(sfull, np.uint16 if half else np.float32, codes if half else codes.view(np.float32), scur)


def median(cvs):
    """Both entries at both radii on 31 x 7, 33 x 9, 65 x 7 and 130 x 9 pixels, the threshold on and off, the four channel
    sets in turn; the nine-row cases read a window strictly inside the source's buffer and write into a buffer that lies one
    column left of and one row below it."""
    cases = []
    for n, (w, h) in enumerate(SIZES):
        scur = (0, 0, w - 1, h - 1)
        sfull = scur if h == 7 else (-2, -1, w + 1, h + 1)
        tfull = scur if h == 7 else (-1, 1, w - 2, h)
        for half in (True, False):
            for radius in (1, 2):
                threshold = mm.THRESHOLD if (radius + n) & 1 else 0.0
                channels = CHANNELS[(n + radius + half) % 4]

                def case(fac, w=w, h=h, sfull=sfull, scur=scur, tfull=tfull, half=half, radius=radius, threshold=threshold, channels=channels):
                    rng = np.random.default_rng(2100 + w + h)
                    src = fac.frame(source(rng, half, sfull, scur))
                    out = fac.frame(blank(half, tfull), out=True, cmp="f16" if half else "f32")
                    p = _lib.median(radius, threshold, mm.mask_of(channels))
                    entry = cvs.cvs_median_f16_dev if half else cvs.cvs_median_f32_dev
                    return entry(out.ref(), src.ref(), C.byref(p), fac.stream)
                cases.append(("median %dx%d %s radius %d threshold %g channels %s" % (w, h, "f16" if half else "f32", radius, threshold, channels), case))
    return cases


GROUPS = [("median", median)]
