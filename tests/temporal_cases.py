"""The temporal denoise's catalogue of device-entry calls, in the form of tests/entry_cases.py and tests/deinterlace_cases.py: a
case is a function case(fac) that makes ONE call of cvs_temporal_denoise_f16_dev (include/canvas_temporal.h) on operands it takes
from a factory, in the same order every time, on the stream fac.stream, and returns the entry's return code.  So the harnesses
that run the catalogue -- frames packed into a guarded arena, a stream that records and replays, windows far from the origin --
run these calls with no harness code of their own (tests/test_temporal_harness_gpu.py), and tests/test_temporal_cpu.py holds the
cases to the header without a GPU.

The pictures are tests/temporal_model.py's sequence, so that every class of every neighbour's weight is met in every case that
has a neighbour; the first case has all four neighbours, so that the harness which bends one operand at a time finds every
operand."""
import ctypes as C

import numpy as np

from canvas_amd import _lib
from canvas_amd.abi import HostFrame
from tests import temporal_model as tm
from tests.entry_cases import _ANY, blank

ENTRIES = ("cvs_temporal_denoise_f16_dev",)
SIZES = [(31, 7), (33, 9), (65, 7), (130, 9)]
THRESHOLD, SOFTNESS = 0.05, 0.1
# which of prev2, prev1, next1, next2 are handed in (the others NULL)
WHICH = {"all": (1, 1, 1, 1), "near": (0, 1, 1, 0), "before": (1, 1, 0, 0), "next1": (0, 0, 1, 0), "none": (0, 0, 0, 0)}
CHANNELS = [tm.ALL, tm.A, tm.R | tm.G | tm.B, tm.G | tm.A]
# nothing depends on coordinates (no row parity here): far from the origin the entry gives the origin's bytes at any offset within
# CVS_MAX_COORD
FAR_RULE = _ANY


def temporal(cvs):
    """Frames of 31 x 7, 33 x 9, 65 x 7 and 130 x 9 pixels with four, the two near, the two earlier, one and no neighbours, the
    four channel sets in turn, the ramp and (65 columns) the hard switch; the nine-row cases write into a buffer that lies one
    column left of and one row below the inputs'."""
    cases = []
    for n, (w, h) in enumerate(SIZES):
        full = (0, 0, w - 1, h - 1)
        tfull = full if h == 7 else (-1, 1, w - 2, h)
        softness = 0.0 if w == 65 else SOFTNESS
        for k, (word, which) in enumerate(WHICH.items()):
            channels = CHANNELS[(n + k) % 4]

            def case(fac, w=w, h=h, full=full, tfull=tfull, which=which, channels=channels, softness=softness):
                rng = np.random.default_rng(1700 + w + h)
                prev2, prev1, cur, next1, next2 = (HostFrame(full, np.uint16, codes, full) for codes in tm.sequence(rng, full, THRESHOLD, SOFTNESS))
                frames = [fac.frame(f) if on else None for f, on in zip((prev2, prev1), which[:2])]
                frames.append(fac.frame(cur))
                frames += [fac.frame(f) if on else None for f, on in zip((next1, next2), which[2:])]
                out = fac.frame(blank(True, tfull), out=True, cmp="f16")
                p = _lib.temporal_denoise(THRESHOLD, softness, channels)
                refs = [f.ref() if f else None for f in frames]
                return cvs.cvs_temporal_denoise_f16_dev(out.ref(), refs[0], refs[1], refs[2], refs[3], refs[4], C.byref(p), fac.stream)
            cases.append(("temporal %dx%d neighbours %s channels %x softness %g" % (w, h, word, channels, softness), case))
    return cases


GROUPS = [("temporal_denoise", temporal)]
