"""The 4:2:2 edges' catalogue of device-entry calls, in the form of tests/entry_cases.py's mpeg2(): a case is a function case(fac)
that makes ONE call of cvs_reconstruct_422_dev or cvs_subsample_422_dev (include/canvas_ycc422.h) on operands it takes from a
factory, in the same order every time -- the planes through fac.buffer(), the frame through fac.frame() -- on the stream
fac.stream, and returns the entry's return code.  So the harnesses that run the catalogue run these calls with no harness code of
their own (tests/test_ycc422_harness_gpu.py).

Every case is built from a SPEC, a plain dict, so that what the call must give can be worked out from the model alone
(expected()): tests/test_ycc422_gpu.py compares bit for bit, and tests/test_ycc422_cpu.py checks without a GPU that every rule of
the contract moves the expectation of at least one case.

The 8-bit layouts' buffers are of class "plane" (any byte address), the 10-bit layouts' of class "bytes" (whose placements keep
a multiple of 4).  Import inputs are random in EVERY bit: codes outside the legal range, garbage in bits 10-15 of a PLANAR10
sample, in bits 30-31 of a v210 word and in the fields of a last group beyond the width, and in the padding.  Export frames are
entry_cases.px16's: NaNs, infinities, negatives and values above 1 among the pixels."""
import ctypes as C

import numpy as np

from canvas_amd import _lib
from tests import ycc422_model as ym
from tests.entry_cases import PAD, _image, blank, px16

ENTRIES = ("cvs_reconstruct_422_dev", "cvs_subsample_422_dev")
LAYOUT_NAMES = ["planar8", "planar10", "uyvy", "v210"]
# pixels one lane owns (kernels/ycc422_*.hip): a wave's run is 63 lanes' worth, 126 or (v210) 378 columns
LANE_PIXELS = {"planar8": 2, "planar10": 2, "uyvy": 2, "v210": 6}
HEIGHTS = [1, 2, 3, 5]
# stride beyond the least per plane (kept on the layout's alignment) and lines beyond the height
PADS = {"planar8": [(0, 0, 0), (13, 5, 64), (1, 1, 0)], "planar10": [(0, 0, 0), (14, 6, 64), (2, 2, 0)],
        "uyvy": [(0, 0, 0), (13, 0, 0), (1, 0, 0)], "v210": [(0, 0, 0), (20, 0, 0), (4, 0, 0)]}
EXTRA = [(0, 0, 0), (2, 1, 3), (0, 0, 1)]
# the raster sits at the origin: nothing of it moves with the frame (tests/entry_cases.py "anchored")
FAR_RULE = None


def widths(layout):
    """The smallest, then one width each side of a wave's run of columns and of two waves'."""
    run = 63 * LANE_PIXELS[layout]
    return [2, 4, 6, 8, 10, 14, run - 2, run, run + 2, run + 6, 2 * run - 2, 2 * run + 2]


def frames_over(width, height):
    """Full windows: the raster's own, larger on every side, inside it, partly off it with a negative origin."""
    return [(0, 0, width - 1, height - 1), (-3, -1, width + 1, height), (1, 0, max(width - 2, 1), height - 1), (-2, -1, width // 2, max(height - 2, 0))]


def specs(layout):
    out = []
    for n, width in enumerate(widths(layout)):
        height = HEIGHTS[n % 4]
        pads, extra = PADS[layout][n % 3], EXTRA[n % 3]
        strides, lines = ym.least(layout, width, height)
        strides = [s + p for s, p in zip(strides, pads)]
        lines = [m + e for m, e in zip(lines, extra)]
        for direction in ("reconstruct", "subsample"):
            # the small widths take every frame in turn, the wave-run widths one (they are what the columns are about)
            for k, full in enumerate(frames_over(width, height)):
                if width > 14 and k != n % 4:
                    continue
                out.append(dict(direction=direction, layout=layout, matrix="709" if (n + k) % 2 else "601", width=width, height=height,
                                strides=strides, lines=lines, full=full, seed=2200 + 16 * n + k))
    return out


def name(spec):
    return "4:2:2 %s %s %dx%d %r matrix %s strides %r lines %r" % (spec["direction"], spec["layout"], spec["width"], spec["height"], spec["full"],
                                                                  spec["matrix"], spec["strides"], spec["lines"])


def _flags(spec):
    return _lib.YCC_REC709 if spec["matrix"] == "709" else 0


def planes_in(spec):
    """An import's planes: every byte random."""
    rng = np.random.default_rng(spec["seed"])
    return [rng.integers(0, 256, (n, s), dtype=np.uint8) for n, s in zip(spec["lines"], spec["strides"])]


def frame_in(spec):
    """An export's frame: the current window one column short of the buffer's part of the raster where there is room, on the left
    (as at mpeg2()) or, every other case, on the right, so that column 0 is inside the window in half of the cases."""
    full, width, height = spec["full"], spec["width"], spec["height"]
    short = 1 if width > 2 else 0
    left = spec["seed"] % 2
    cur = (max(full[0], 0) + (short if left else 0), max(full[1], 0), min(full[2], width - 1) - (0 if left else short), min(full[3], height - 1))
    if cur[0] > cur[2] or cur[1] > cur[3]:
        cur = (0, 0, -1, -1)
    return px16(np.random.default_rng(spec["seed"] + 1), full, cur)


def make_case(cvs, spec):
    layout, width, height, strides, lines = ym.LAYOUTS[spec["layout"]], spec["width"], spec["height"], spec["strides"], spec["lines"]
    cls = "plane" if ym.BITS[spec["layout"]] == 8 else "bytes"
    nplanes = len(strides)

    def image(ptrs):
        return _image(list(ptrs) + [None] * (3 - nplanes), list(strides) + [0] * (3 - nplanes), list(lines) + [0] * (3 - nplanes))

    def reconstruct(fac):
        ptrs = [fac.buffer(p, cls, name="plane %d" % k) for k, p in enumerate(planes_in(spec))]
        out = fac.frame(blank(True, spec["full"]), out=True, cmp="f16")
        return cvs.cvs_reconstruct_422_dev(out.ref(), C.byref(image(ptrs)), width, height, layout, _flags(spec), fac.stream)

    def subsample(fac):
        frame = fac.frame(frame_in(spec))
        ptrs = [fac.buffer(np.full((n, s), PAD, np.uint8), cls, out=True, name="plane %d" % k) for k, (n, s) in enumerate(zip(lines, strides))]
        return cvs.cvs_subsample_422_dev(C.byref(image(ptrs)), frame.ref(), width, height, layout, _flags(spec), fac.stream)
    return reconstruct if spec["direction"] == "reconstruct" else subsample


def expected(spec, orc, rules=ym.RULES):
    """What the case's call leaves in its outputs, from the model alone.  reconstruct: (frame codes, window or None); subsample:
    the planes as uint8 arrays (lines, stride), PAD wherever the call writes nothing."""
    width, height = spec["width"], spec["height"]
    if spec["direction"] == "reconstruct":
        raster = ym.reconstruct_model(spec["layout"], planes_in(spec), width, height, orc.transfer_table(0), orc.float_to_half, spec["matrix"], rules)
        return ym.expected_frame(blank(True, spec["full"]).array, spec["full"], raster, width, height)
    frame = frame_in(spec)
    return ym.subsample_model(spec["layout"], frame.array, spec["full"], frame.current_window.tuple(), width, height, orc.transfer_table(2), spec["matrix"],
                              spec["strides"], spec["lines"], PAD, rules)


def _group(layout):
    def build(cvs):
        return [(name(s), make_case(cvs, s)) for s in specs(layout)]
    return build


GROUPS = [("ycc422[%s]" % layout, _group(layout)) for layout in LAYOUT_NAMES]
