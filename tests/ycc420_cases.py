"""The 4:2:0 edges' catalogue of device-entry calls, in the form of tests/ycc422_cases.py: a case is a function case(fac) that
makes ONE call of cvs_reconstruct_420_dev or cvs_subsample_420_dev (include/canvas_ycc420.h) on operands it takes from a factory,
in the same order every time -- the planes through fac.buffer(), the frame through fac.frame() -- on the stream fac.stream, and
returns the entry's return code.  So the harnesses that run the catalogue run these calls with no harness code of their own
(tests/test_ycc420_harness_gpu.py).

Every case is built from a SPEC, a plain dict, so that what the call must give can be worked out from the model alone
(expected()): tests/test_ycc420_gpu.py compares bit for bit, and tests/test_ycc420_cpu.py checks without a GPU that every rule of
the contract moves the expectation of at least one case.

The 8-bit layouts' buffers are of class "plane" (any byte address), the 10-bit layouts' of class "bytes" (whose placements keep
a multiple of 4).  Import inputs are random in EVERY bit: codes outside the legal range, garbage in bits 10-15 of a PLANAR10
sample and in bits 0-5 of a P010 sample, and in the padding.  Export frames are entry_cases.px16's: NaNs, infinities, negatives
and values above 1 among the pixels.  Siting, range, matrix and transfer rotate over the cases, so that every value of each meets
every layout in both directions."""
import ctypes as C

import numpy as np

from tests import ycc420_model as ym
from tests.entry_cases import PAD, _image, blank, px16

ENTRIES = ("cvs_reconstruct_420_dev", "cvs_subsample_420_dev")
LAYOUT_NAMES = ["planar8", "planar10", "nv12", "p010"]
SITINGS, RANGES, MATRIX_NAMES, TRANSFERS = ["left", "center", "topleft"], ["studio", "full"], ["709", "601", "2020"], ["709", "none"]
# pixels one lane owns along a row (kernels/ycc420_*.hip): a wave's run is 63 lanes' worth, 126 columns; the import at centre
# siting keeps one lane more for the column on the left, 62 lanes' worth, which is the run less two columns
LANE_PIXELS = 2
RUN = 63 * LANE_PIXELS
# rows: a lane owns a row pair; a workgroup's strip is at most 32 pairs (kMaxStrip), 64 rows
STRIP_ROWS = 2 * 32
HEIGHTS = [2, 4, 6, 10, STRIP_ROWS - 2, STRIP_ROWS, STRIP_ROWS + 2]
# stride beyond the least per plane (kept on the layout's alignment) and lines beyond the least
PADS = {"planar8": [(0, 0, 0), (13, 5, 64), (1, 1, 0)], "planar10": [(0, 0, 0), (14, 6, 64), (2, 2, 0)],
        "nv12": [(0, 0), (13, 5), (1, 64)], "p010": [(0, 0), (14, 6), (2, 64)]}
EXTRA = [(0, 0, 0), (2, 1, 3), (0, 0, 1)]
# the raster sits at the origin: nothing of it moves with the frame (tests/entry_cases.py "anchored")
FAR_RULE = None
# The strip is the fewest chroma rows that leave no wave of the launch without a unit, so only a raster with more row pairs than
# the launch has waves gives a wave a second row: 256 CUs x 6 workgroups x 4 waves in the gathered form.  A 14-column raster of
# twice that many row pairs and a few more is 0.3 megapixels: strips of three chroma rows, the last one short.
TALL = (14, 2 * (2 * 256 * 6 * 4 + 2))


def widths():
    """The smallest, then one width each side of a wave's run of columns (126, at centre siting 124) and of two waves'."""
    return [2, 4, 6, 8, 10, 14, RUN - 4, RUN - 2, RUN, RUN + 2, 2 * RUN - 6, 2 * RUN - 4, 2 * RUN - 2, 2 * RUN, 2 * RUN + 2]


def frames_over(width, height):
    """Full windows: the raster's own, larger on every side, inside it, partly off it with a negative origin."""
    return [(0, 0, width - 1, height - 1), (-3, -1, width + 1, height), (1, 0, max(width - 2, 1), height - 1), (-2, -1, width // 2, max(height - 2, 0))]


def _spec(layout, direction, i, width, height, pads, extra, full, seed):
    strides, lines = ym.least(layout, width, height)
    return dict(direction=direction, layout=layout, siting=SITINGS[i % 3], range=RANGES[i % 2], matrix=MATRIX_NAMES[(i // 3) % 3],
                transfer=TRANSFERS[(i // 2) % 2], width=width, height=height, strides=[s + p for s, p in zip(strides, pads)],
                lines=[m + e for m, e in zip(lines, extra)], full=full, seed=seed)


def specs(layout):
    out = []
    for direction in ("reconstruct", "subsample"):
        i = LAYOUT_NAMES.index(layout)                  # the rotation starts elsewhere for every layout
        for n, width in enumerate(widths()):
            height = HEIGHTS[n % len(HEIGHTS)]
            # the small widths take every frame in turn, the wave-run widths one (they are what the columns are about) in every
            # siting (the import's run is a lane shorter at centre siting)
            for k, full in enumerate(frames_over(width, height)):
                if width > 14 and k != n % 4:
                    continue
                for siting in SITINGS if width > 14 else [None]:
                    spec = _spec(layout, direction, i, width, height, PADS[layout][n % 3], EXTRA[n % 3], full, 4200 + 16 * n + k)
                    out.append(spec if siting is None else dict(spec, siting=siting))
                    i += 1
    return out


def tall_specs(layout):
    """One raster per direction and siting whose strips hold three chroma rows (TALL); not part of GROUPS: the harnesses run the
    catalogue at many placements, and the strip is a matter of rows, not of where a buffer lies."""
    width, height = TALL
    return [_spec(layout, direction, i, width, height, PADS[layout][1], EXTRA[2], (0, 0, width - 1, height - 1), 4900 + i)
            for direction in ("reconstruct", "subsample") for i in range(3)]


def name(spec):
    return "4:2:0 %s %s %dx%d %r %s %s matrix %s transfer %s strides %r lines %r" % (
        spec["direction"], spec["layout"], spec["width"], spec["height"], spec["full"], spec["siting"], spec["range"], spec["matrix"], spec["transfer"],
        spec["strides"], spec["lines"])


def flags(spec):
    return ym.flags(spec["matrix"], spec["range"], spec["siting"], spec["transfer"])


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
        return cvs.cvs_reconstruct_420_dev(out.ref(), C.byref(image(ptrs)), width, height, layout, flags(spec), fac.stream)

    def subsample(fac):
        frame = fac.frame(frame_in(spec))
        ptrs = [fac.buffer(np.full((n, s), PAD, np.uint8), cls, out=True, name="plane %d" % k) for k, (n, s) in enumerate(zip(lines, strides))]
        return cvs.cvs_subsample_420_dev(C.byref(image(ptrs)), frame.ref(), width, height, layout, flags(spec), fac.stream)
    return reconstruct if spec["direction"] == "reconstruct" else subsample


def expected(spec, orc, rules=ym.RULES):
    """What the case's call leaves in its outputs, from the model alone.  reconstruct: (frame codes, window or None); subsample:
    the planes as uint8 arrays (lines, stride), PAD wherever the call writes nothing."""
    width, height = spec["width"], spec["height"]
    if spec["direction"] == "reconstruct":
        raster = ym.reconstruct_model(spec["layout"], planes_in(spec), width, height, orc.transfer_table(0), orc.float_to_half, spec["matrix"], spec["range"],
                                      spec["siting"], spec["transfer"], rules)
        return ym.expected_frame(blank(True, spec["full"]).array, spec["full"], raster, width, height)
    frame = frame_in(spec)
    return ym.subsample_model(spec["layout"], frame.array, spec["full"], frame.current_window.tuple(), width, height, orc.transfer_table(2), spec["matrix"],
                              spec["range"], spec["siting"], spec["transfer"], spec["strides"], spec["lines"], PAD, rules)


def _group(layout):
    def build(cvs):
        return [(name(s), make_case(cvs, s)) for s in specs(layout)]
    return build


GROUPS = [("ycc420[%s]" % layout, _group(layout)) for layout in LAYOUT_NAMES]
