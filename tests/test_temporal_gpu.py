"""The temporal denoise on the GPU, bit for bit against the numpy model of the contract (tests/temporal_model.py, DESIGN.md
"Temporal denoise") in both arithmetic flavours, which must give equal bytes.  tests/test_fields_gpu.py's scheme: the output buffer
is pre-filled with a sentinel so that untouched pixels are proven untouched, the inputs are checked unwritten, copied codes are
compared code for code and computed ones with the sign of zero and NaN payloads folded (tests/util.py canon_f16).  The pictures are
tests/temporal_model.py's sequences (a static, a ramp and a noise third, so that every class of every neighbour's weight is met:
tests/test_temporal_cpu.py holds every case listed here to that) with the band and scatter of special halfs.

Shapes: the kernel makes 62 lanes of columns per workgroup -- 124 columns in the pair form, 62 in the one-pixel form -- and walks
segments of at least 8 rows (rowstream::shape, kMinSeg), so 130 x 9 and 67 x 9 cross a wave seam and a segment seam in either
form.  A buffer one column wider than the window forces either form on any width (the pair form needs even pitches); a frame whose
base lies at 8 modulo 16 is the placement harness's (tests/test_temporal_harness_gpu.py).

The cases are lists built by functions (CASES_*), so that tests/test_temporal_cpu.py can hold them to the condition on the
weights by the model alone."""
import ctypes as C

import numpy as np
import pytest

from canvas_amd import _lib
from canvas_amd.abi import HostFrame
from canvas_amd.device import DeviceFrame
from tests import fields_model as fm
from tests import temporal_model as tm
from tests.test_fields_gpu import SENTINEL, _box, _run
from tests.util import canon_f16

pytestmark = pytest.mark.gpu

THRESHOLD, SOFTNESS = 0.05, 0.1
PREV2, PREV1, CUR, NEXT1, NEXT2 = range(5)


def sequence(seed, cw, pad=0, specials=True, windows=None):
    """[prev2, prev1, cur, next1, next2] as frames.  cur's current window is cw and its buffer `pad` columns wider on the right;
    windows: {index: window} gives a neighbour a current window of its own (the picture is continued there, in absolute
    coordinates) in a buffer of its own geometry, one row and two columns larger than that window."""
    rng = np.random.default_rng(seed)
    windows = windows or {}
    big = cw
    for win in windows.values():
        big = fm.bounding(big, win)
    codes = tm.sequence(rng, big, THRESHOLD, SOFTNESS, specials)
    frames = []
    for k in range(5):
        cur = windows.get(k, cw)
        full = (cur[0] - 2, cur[1], cur[2], cur[3] + 1) if k in windows else (cw[0], cw[1], cw[2] + pad, cw[3])
        array = rng.integers(0, 0x3C01, _box(full) + (4,), dtype=np.uint16)
        fm.crop(array, full, cur)[...] = fm.crop(codes[k], big, cur)
        frames.append((array, full, cur))
    return frames


def neighbours_of(frames):
    """the model's order: prev1, next1, prev2, next2"""
    return [frames[PREV1], frames[NEXT1], frames[PREV2], frames[NEXT2]]


def _entry(cvs, p, order):
    """call(out, *devs) for _run: `order` names, for prev2 .. next2, the index of the device frame handed in (None: NULL)"""
    def call(out, *devs):
        ref = [None if i is None else devs[i].ref() for i in order]
        return cvs.cvs_temporal_denoise_f16_dev(out.ref(), ref[0], ref[1], ref[2], ref[3], ref[4], C.byref(p), None)
    return call


def _operands(frames):
    """(device inputs, order): a frame that appears several times in `frames` (the same object) is ONE device frame handed in
    as several operands"""
    inputs, order = [], []
    for f in frames:
        if f is None:
            order.append(None)
            continue
        at = [i for i, g in enumerate(inputs) if g is f]
        if not at:
            inputs.append(f)
            at = [len(inputs) - 1]
        order.append(at[0])
    return inputs, order


def compare(got, want, exact, what):
    """exact: mask over the codes of those that are copies (compared code for code); the others fold -0 and NaN payloads."""
    g, w = np.where(exact, got, canon_f16(got)), np.where(exact, want, canon_f16(want))
    if not np.array_equal(g, w):
        bad = np.argwhere((g != w).any(axis=-1))
        y, x = bad[0]
        raise AssertionError("%s: %d pixels differ; first at buffer row %d column %d: got %s want %s" % (
            what, len(bad), y, x, [hex(v) for v in got[y, x]], [hex(v) for v in want[y, x]]))


def check(cvs, orc, case):
    """One call against the model.  case: (what, out_full, frames, threshold, softness, channels); frames are (codes, full,
    current), (codes, full, None) for an empty window, or None (NULL)."""
    what, out_full, frames, threshold, softness, channels = case
    inputs, order = _operands(frames)
    p = _lib.temporal_denoise(threshold, softness, channels)
    (rc, got, window), before = _run(cvs, _entry(cvs, p, order), out_full, inputs)
    assert rc == 0, "%s: %s" % (what, _lib.last_error())
    want, want_window, exact, w = tm.expected(before, out_full, frames[CUR], neighbours_of(frames), threshold, softness, channels, orc.float_to_half)
    assert window == want_window, "%s: window %r, want %r" % (what, window, want_window)
    compare(got, want, exact, what)
    return w


def _case(what, out_full, frames, threshold=THRESHOLD, softness=SOFTNESS, channels=tm.ALL):
    return (what, out_full, frames, threshold, softness, channels)


# (width, height, pairs): a wave seam and a segment seam in each form, and the smallest windows
SHAPES = [(130, 9, True), (130, 9, False), (67, 9, True), (67, 9, False), (1, 1, False), (1, 5, False), (5, 1, False), (3, 3, False), (2, 2, True)]


def cases_whole_frames(width, height, pairs):
    pad = (width & 1) if pairs else 1 - (width & 1)                  # an even pitch, or an odd one
    cases = []
    for n, (x0, y0) in enumerate([(0, 0), (1, -1)]):
        cw = (x0, y0, x0 + width - 1, y0 + height - 1)
        frames = sequence(width * 131 + height * 7 + n, cw, pad)
        for radius in (1, 2):
            given = frames if radius == 2 else [None, frames[1], frames[2], frames[3], None]
            cases.append(_case("%dx%d pad %d at (%d, %d) radius %d" % (width, height, pad, x0, y0, radius), frames[CUR][1], given))
    return cases


@pytest.mark.parametrize("width,height,pairs", SHAPES)
def test_whole_frames(cvs, orc, width, height, pairs):
    for case in cases_whole_frames(width, height, pairs):
        check(cvs, orc, case)


def cases_which_neighbours(pairs):
    """every pattern of which neighbours are present, an absent one NULL or empty in turn; one buffer as several operands"""
    width = 130 if pairs else 67
    cw = (0, -1, width - 1, 7)
    frames = sequence(79 + width, cw, 0 if pairs else 1 - (width & 1))
    empty = lambda f: (f[0], f[1], None)
    cases = []
    for mask in range(16):
        given = list(frames)
        for bit, k in enumerate((PREV2, PREV1, NEXT1, NEXT2)):
            if not mask & (1 << bit):
                given[k] = None if (mask + bit) & 1 else empty(frames[k])
        cases.append(_case("present %s (prev2 prev1 next1 next2), %s" % (format(mask, "04b")[::-1], "pairs" if pairs else "single"), frames[CUR][1], given))
    p2, p1, c, n1, n2 = frames
    cases += [_case("prev1 is next1", frames[CUR][1], [None, p1, c, p1, None]), _case("prev2 is prev1, next2 is next1", frames[CUR][1], [p1, p1, c, n1, n1]),
              _case("prev1 is cur", frames[CUR][1], [p2, c, c, n1, n2]), _case("all five are cur", frames[CUR][1], [c, c, c, c, c]),
              _case("one neighbour in all four places", frames[CUR][1], [n2, n2, c, n2, n2])]
    return cases


@pytest.mark.parametrize("pairs", [True, False])
def test_which_neighbours_are_given(cvs, orc, pairs):
    for case in cases_which_neighbours(pairs):
        check(cvs, orc, case)


PARAMETERS = [(THRESHOLD, 0.0), (-1.0, SOFTNESS), (-1.0, 0.0), (0.0, SOFTNESS), (0.0, 0.0), (131072.0, SOFTNESS), (131072.0, 0.0), (THRESHOLD, 1e-42), (THRESHOLD, 3e38)]


def cases_parameters(threshold, softness):
    cases = []
    for width, pad in ((130, 0), (67, 0)):
        cw = (0, 0, width - 1, 8)
        frames = sequence(80 + width, cw, pad)
        cases.append(_case("%dx9 threshold %g softness %g" % (width, threshold, softness), frames[CUR][1], frames, threshold, softness))
    return cases


@pytest.mark.parametrize("threshold,softness", PARAMETERS)
def test_thresholds_and_softness(cvs, orc, threshold, softness):
    for case in cases_parameters(threshold, softness):
        check(cvs, orc, case)


CHANNELS = [tm.R, tm.G, tm.B, tm.A, tm.ALL, tm.R | tm.B, tm.G | tm.B | tm.A]


def cases_channels(channels):
    cases = []
    for width, pad in ((130, 0), (67, 0)):
        cw = (1, 0, width, 8)
        frames = sequence(300 + width, cw, pad)
        cases.append(_case("%dx9 channels %x" % (width, channels), frames[CUR][1], frames, channels=channels))
        cases.append(_case("%dx9 channels %x hard, near frames" % (width, channels), frames[CUR][1], [None] + frames[1:4] + [None], softness=0.0, channels=channels))
    return cases


@pytest.mark.parametrize("channels", CHANNELS)
def test_channels(cvs, orc, channels):
    for case in cases_channels(channels):
        check(cvs, orc, case)


def cases_inner_windows(pairs):
    """out.full_window larger than, smaller than and offset against cur.current_window (rows above and below the output count,
    and so do columns left and right of it); neighbours whose windows are smaller than and offset from cur's, each in a buffer
    of its own geometry"""
    cw = (2, -3, 2 + 129, -3 + 17)
    pad = 0 if pairs else 1
    frames = sequence(77, cw, pad)
    cases = []
    for out_full in [(cw[0] - 4, cw[1] - 3, cw[2] + 5, cw[3] + 2), (cw[0] + 4, cw[1] + 3, cw[2] - 6, cw[3] - 5), (cw[0] + 3, cw[1] + 4, cw[2] - 5, cw[3] - 4),
                     (cw[0] + 60, cw[1] + 9, cw[2] + 30, cw[3] + 9), (cw[0] - 20, cw[1] - 10, cw[0] + 62, cw[1] + 8), (cw[0] + 7, cw[1] + 5, cw[0] + 7, cw[1] + 5),
                     (cw[2] + 1, cw[1], cw[2] + 9, cw[3])]:
        cases.append(_case("out %r cur %r" % (out_full, cw), out_full, frames))
    x0, y0, x1, y1 = cw
    for n, windows in enumerate([{PREV1: (x0 + 1, y0, x1, y1)}, {NEXT1: (x0, y0, x1 - 2, y1), PREV2: (x0, y0 + 1, x1, y1)},
                                 {PREV1: (x0 + 9, y0 + 2, x1 - 9, y1 - 1), NEXT2: (x0 + 2, y0, x1, y1 - 9)},
                                 {PREV2: (x0 - 3, y0 - 2, x1 - 5, y1 + 2), PREV1: (x0 - 1, y0 - 1, x1 + 1, y1 + 1), NEXT1: (x0 + 5, y0 + 3, x1 + 6, y1 + 4), NEXT2: (x0 + 6, y0 - 4, x1 + 2, y1 - 3)},
                                 {PREV1: (x0, y0 + 9, x1, y1), NEXT1: (x0 + 70, y0, x1, y1)},
                                 {PREV1: (x1 + 2, y0, x1 + 20, y1), NEXT1: (x0, y1 + 1, x1, y1 + 5), PREV2: (x0, y0, x1, y1), NEXT2: (x0 + 500, y0 + 500, x0 + 520, y0 + 510)}]):
        moved = sequence(400 + n, cw, pad, windows=windows)
        cases.append(_case("neighbour windows %d: %r" % (n, windows), moved[CUR][1], moved))
        cases.append(_case("neighbour windows %d, out inside" % n, (x0 + 3, y0 + 1, x1 - 4, y1 - 2), moved))
    return cases


@pytest.mark.parametrize("pairs", [True, False])
def test_inner_windows(cvs, orc, pairs):
    for case in cases_inner_windows(pairs):
        check(cvs, orc, case)


def cases_extents(width, height):
    cw = (0, 0, width - 1, height - 1)
    return [_case("%dx%d" % (width, height), cw, sequence(82, cw, specials=height < 100))]


@pytest.mark.parametrize("width,height", [(1, 4194305), (131073, 3)])
def test_tall_and_wide_windows(cvs, orc, width, height):
    """more rows of workgroups than a grid holds (the launcher folds them into longer segments), and a row of more than 2^16
    columns"""
    for case in cases_extents(width, height):
        check(cvs, orc, case)


def test_refusals(cvs):
    """every refusal of the contract: -1, its message, an empty window and an unwritten output"""
    full = (0, 0, 15, 15)
    lim = _lib.MAX_COORD
    sentinel = np.broadcast_to(SENTINEL, (16, 16, 4)).copy()
    out = DeviceFrame.from_host(HostFrame(full, np.uint16, sentinel))
    ins = [DeviceFrame.from_host(HostFrame(full, np.uint16, sentinel, full)) for _ in range(5)]
    ok = _lib.temporal_denoise(0.05, 0.1)
    nan, inf = float("nan"), float("inf")
    box = _lib.box2i.of

    def entry(o, refs, p):
        return cvs.cvs_temporal_denoise_f16_dev(o, refs[0], refs[1], refs[2], refs[3], refs[4], p, None)

    def alias(data, fullw=full, cur=full):
        return _lib.rgba_frame_f16(data, box(*fullw), box(*cur))

    refs = lambda: [f.ref() for f in ins]
    swapped = lambda k, value: refs()[:k] + [value] + refs()[k + 1:]
    cases = [("need", lambda: entry(out.ref(), swapped(CUR, None), C.byref(ok))), ("need", lambda: entry(out.ref(), refs(), None))]
    cases += [("channels", lambda c=c: entry(out.ref(), refs(), C.byref(_lib.temporal_denoise(channels=c)))) for c in (0, 16, -1, 0x1F)]
    cases += [("flags", lambda f=f: entry(out.ref(), refs(), C.byref(_lib.temporal_denoise(flags=f)))) for f in (1, -1, 0x100)]
    cases += [("threshold", lambda t=t: entry(out.ref(), refs(), C.byref(_lib.temporal_denoise(t, 0.1)))) for t in (nan, inf, -inf)]
    cases += [("softness", lambda t=t: entry(out.ref(), refs(), C.byref(_lib.temporal_denoise(0.05, t)))) for t in (nan, inf, -inf, -0.5)]
    keep = []
    for k in range(5):
        # (another frame struct over the output's buffer: the output's own struct has an empty window from the first line on)
        keep.append(alias(out.ptr))
        cases.append(("cannot be one of the inputs", lambda k=k, a=keep[-1]: entry(out.ref(), swapped(k, C.byref(a)), C.byref(ok))))
        keep.append(alias(ins[k].ptr, full, (0, 0, 16, 15)))
        cases.append(("outside its buffer", lambda k=k, a=keep[-1]: entry(out.ref(), swapped(k, C.byref(a)), C.byref(ok))))
        for fullw, cur in (((lim - 14, 0, lim + 1, 15), (lim - 14, 0, lim, 15)), ((0, -lim - 1, 15, -lim + 14), (0, -lim, 15, -lim + 14)),
                           ((0, 0, 2 ** 31 - 1, 15), full), ((-2 ** 31, 0, 15, 15), full), ((lim - 14, 0, lim + 1, 15), (0, 0, -1, -1))):
            keep.append(alias(ins[k].ptr, fullw, cur))
            cases.append(("beyond", lambda k=k, a=keep[-1]: entry(out.ref(), swapped(k, C.byref(a)), C.byref(ok))))
    cases.append(("cannot be one of the inputs", lambda: entry(out.ref(), [None, None, out.ref(), None, None], C.byref(ok))))
    try:
        for word, call in cases:
            out.c.current_window = out.c.full_window
            cvs.cvs_clear_last_error()
            assert call() == -1, word
            assert "cvs_temporal_denoise_f16_dev" in _lib.last_error() and word in _lib.last_error(), (word, _lib.last_error())
            assert out.current_window.is_empty(), word
        far = alias(out.ptr, (lim - 14, 0, lim + 1, 15), (0, 0, 15, 15))
        cvs.cvs_clear_last_error()
        assert entry(C.byref(far), refs(), C.byref(ok)) == -1 and "beyond" in _lib.last_error() and far.current_window.is_empty()
        cvs.cvs_clear_last_error()
        assert entry(None, refs(), C.byref(ok)) == -1 and "need" in _lib.last_error()
        _lib.check(cvs.cvs_stream_sync(None), "sync")
        assert np.array_equal(out.download().array, sentinel), "a refused call wrote"
        # an absent neighbour may share the output's buffer: it is never read
        gone = alias(out.ptr, full, (0, 0, -1, -1))
        assert entry(out.ref(), [C.byref(gone), None, ins[2].ref(), C.byref(gone), None], C.byref(ok)) == 0 and out.current_window.tuple() == full
    finally:
        for f in [out] + ins:
            f.free()


# ---------------------------------------------------------------- identities that need no model

def _call(cvs, out_full, frames, p):
    inputs, order = _operands(frames)
    (rc, got, window), _ = _run(cvs, _entry(cvs, p, order), out_full, inputs)
    assert rc == 0, _lib.last_error()
    return got, window


@pytest.mark.parametrize("pairs", [True, False])
def test_identities(cvs, pairs):
    cw = (-2, -1, 140, 17)
    frames = sequence(90, cw, 1 if pairs else 0)
    p2, p1, c, n1, n2 = frames
    out_full = (cw[0] - 1, cw[1] + 2, cw[2] - 3, cw[3] + 2)
    window = fm.intersect(out_full, cw)
    want = np.broadcast_to(SENTINEL, _box(out_full) + (4,)).copy()
    fm.crop(want, out_full, window)[...] = fm.crop(c[0], c[1], window)
    soft = _lib.temporal_denoise
    # no neighbour present, or nothing ever static: cur code for code
    for what, given, p in [("no neighbours", [None, None, c, None, None], soft(THRESHOLD, SOFTNESS)), ("never static", frames, soft(-1.0, 0.0)),
                           ("never static, alpha", frames, soft(-1.0, 0.0, tm.A)), ("only far frames", [p2, None, c, None, n2], soft(THRESHOLD, SOFTNESS))]:
        got = _call(cvs, out_full, given, p)
        assert got[1] == window and np.array_equal(got[0], want), what
    # prev and next swapped where prev1 == next1 as codes: the same sums in the same order
    a = _call(cvs, out_full, [p2, p1, c, p1, n2], soft(THRESHOLD, SOFTNESS))
    b = _call(cvs, out_full, [n2, p1, c, p1, p2], soft(THRESHOLD, SOFTNESS))
    assert a[1] == b[1] == window
    # (where at most one far frame has a weight the order of the two far frames changes no sum)
    wa = tm.weights(c, [p1, p1, p2, n2], THRESHOLD, SOFTNESS, tm.ALL)[0]
    mask = fm.crop((wa[2] == 0) | (wa[3] == 0), cw, window)
    assert mask.mean() > 0.3 and np.array_equal(fm.crop(a[0], out_full, window)[mask], fm.crop(b[0], out_full, window)[mask])
    # tiles equal the whole: split at a row and at columns
    whole, got_window = _call(cvs, cw, frames, soft(THRESHOLD, SOFTNESS))
    assert got_window == cw
    for tile in [(cw[0], cw[1], cw[2], 9), (cw[0], 10, cw[2], cw[3]), (cw[0], cw[1], 60, cw[3]), (61, cw[1], cw[2], cw[3]), (cw[0], cw[1], 61, cw[3]), (62, cw[1], cw[2], cw[3])]:
        part, got_window = _call(cvs, tile, frames, soft(THRESHOLD, SOFTNESS))
        assert got_window == tile and np.array_equal(part, fm.crop(whole, cw, tile)), tile
    # all five operands one frame of finite pixels, threshold = softness = 0: code for code (a NaN difference counts as motion)
    still = sequence(91, cw, 1 if pairs else 0, specials=False)[CUR]
    got, got_window = _call(cvs, cw, [still] * 5, soft(0.0, 0.0))
    assert got_window == cw and np.array_equal(got, fm.crop(still[0], still[1], cw))
