"""The motion-adaptive deinterlacer on the GPU, bit for bit against the numpy model of the contract (tests/deinterlace_model.py,
DESIGN.md "Adaptive deinterlace") in both arithmetic flavours, which must give equal bytes.  tests/test_fields_gpu.py's scheme:
the output buffer is pre-filled with a sentinel so that untouched pixels are proven untouched, the inputs are checked unwritten,
copied pixels are compared code for code and computed ones with the sign of zero and NaN payloads folded (tests/util.py canon_f16).
The pictures are tests/deinterlace_model.py's thirds (a static, a perturbed and a noise third, so that every class of the weight
k is met: tests/test_deinterlace_cpu.py holds them to that) with the band and scatter of special halfs.

Shapes: the kernel makes 62 lanes of columns per workgroup -- 124 columns in the pair form, 62 in the one-pixel form -- and walks
segments of at least 8 rows.  A buffer one column wider than the window forces either form on any width (the pair form needs
even pitches)."""
import ctypes as C

import numpy as np
import pytest

from canvas_amd import _lib
from canvas_amd.abi import HostFrame
from canvas_amd.device import DeviceFrame
from tests import deinterlace_model as dm
from tests import fields_model as fm
from tests.test_fields_gpu import SENTINEL, _box, _compare, _rows_mask, _run

pytestmark = pytest.mark.gpu

THRESHOLD, SOFTNESS = 0.05, 0.1


def _entry(cvs, p, order):
    """call(out, *devs) for _run: `order` names, for prev, cur and next, the index of the device frame handed in (None: NULL)"""
    def call(out, *devs):
        ref = lambda i: None if i is None else devs[i].ref()
        return cvs.cvs_deinterlace_adaptive_f16_dev(out.ref(), ref(order[0]), ref(order[1]), ref(order[2]), C.byref(p), None)
    return call


def _check(cvs, orc, out_full, cur, prev, nxt, field, what, threshold=THRESHOLD, softness=SOFTNESS, shared=None):
    """One call against the model.  Frames are (codes, full, current) or None (NULL).  shared: 'neighbours' hands one device
    frame in as prev and next, 'cur' hands cur in as prev too."""
    inputs, order = [cur], [None, 0, None]
    if shared == "cur":
        prev, order[0] = cur, 0
    elif prev is not None:
        inputs.append(prev); order[0] = len(inputs) - 1
    if shared == "neighbours":
        nxt, order[2] = prev, order[0]
    elif nxt is not None:
        inputs.append(nxt); order[2] = len(inputs) - 1
    p = _lib.deinterlace_adaptive(field, threshold, softness)
    (rc, got, window), before = _run(cvs, _entry(cvs, p, order), out_full, inputs)
    assert rc == 0, "%s: %s" % (what, _lib.last_error())
    want, want_window, exact, k = dm.expected(before, out_full, cur, prev, nxt, field, threshold, softness, orc.float_to_half)
    assert window == want_window, "%s: window %r, want %r" % (what, window, want_window)
    _compare(got, want, exact, what)
    return k


def _pictures(seed, cw, pad=0, specials=True):
    """prev, cur, next as frames whose current window is cw and whose buffer is `pad` columns wider on the right"""
    rng = np.random.default_rng(seed)
    full = (cw[0], cw[1], cw[2] + pad, cw[3])
    frames = []
    for codes in dm.thirds(rng, cw, THRESHOLD, SOFTNESS, specials):
        array = rng.integers(0, 0x3C01, _box(full) + (4,), dtype=np.uint16)
        fm.crop(array, full, cw)[...] = codes
        frames.append((array, full, cw))
    return frames


HEIGHTS = [1, 2, 3, 7, 9, 17, 36]
# (width, pairs): one column fewer than, exactly, one more than and twice the columns one workgroup makes, in both forms
WIDTHS = [(1, False), (2, True), (2, False), (3, False), (5, True), (5, False), (33, True), (33, False),
          (123, True), (124, True), (125, True), (248, True), (61, False), (62, False), (63, False), (124, False)]


@pytest.mark.parametrize("width,pairs", WIDTHS)
def test_whole_frames(cvs, orc, width, pairs):
    pad = (width & 1) if pairs else 1 - (width & 1)                  # an even pitch, or an odd one
    seen = np.zeros(3)
    for height in HEIGHTS:
        for n, (x0, y0) in enumerate([(0, 0), (1, -1), (1, 0), (0, -1)]):
            cw = (x0, y0, x0 + width - 1, y0 + height - 1)
            prev, cur, nxt = _pictures(width * 131 + height * 7 + n, cw, pad)
            out_full = cur[1]
            for field in (0, 1):
                k = _check(cvs, orc, out_full, cur, prev, nxt, field, "%dx%d pad %d at (%d, %d) field %d" % (width, height, pad, x0, y0, field))
                seen += np.array(dm.classes(k)) > 0
    if width >= 12:
        assert (seen > 0).all(), seen


def _shrunk(frame, side, by):
    """the frame with its current window cut by `by` columns or rows on one side"""
    array, full, (x0, y0, x1, y1) = frame
    cur = {"left": (x0 + by, y0, x1, y1), "right": (x0, y0, x1 - by, y1), "top": (x0, y0 + by, x1, y1), "bottom": (x0, y0, x1, y1 - by)}[side]
    return (array, full, cur)


def _moved(frame, dx, dy):
    array, full, cur = frame
    return (array, (full[0] + dx, full[1] + dy, full[2] + dx, full[3] + dy), (cur[0] + dx, cur[1] + dy, cur[2] + dx, cur[3] + dy))


@pytest.mark.parametrize("pairs", [True, False])
def test_output_windows_against_the_input(cvs, orc, pairs):
    """out.full_window larger than, smaller than and offset against cur.current_window: rows above and below the output count,
    and so do columns left and right of it"""
    cw = (2, -3, 2 + 129, -3 + 20)
    prev, cur, nxt = _pictures(77, cw, 0 if pairs else 1)
    for out_full in [(cw[0] - 4, cw[1] - 3, cw[2] + 5, cw[3] + 2), (cw[0] + 4, cw[1] + 3, cw[2] - 6, cw[3] - 5), (cw[0] + 3, cw[1] + 4, cw[2] - 5, cw[3] - 4),
                     (cw[0] + 60, cw[1] + 9, cw[2] + 30, cw[3] + 9), (cw[0] - 20, cw[1] - 10, cw[0] + 62, cw[1] + 8), (cw[0] + 7, cw[1] + 5, cw[0] + 7, cw[1] + 5),
                     (cw[2] + 1, cw[1], cw[2] + 9, cw[3])]:
        for field in (0, 1):
            _check(cvs, orc, out_full, cur, prev, nxt, field, "out %r cur %r field %d" % (out_full, cw, field))


@pytest.mark.parametrize("pairs", [True, False])
def test_neighbour_windows_that_cover_part_of_cur(cvs, orc, pairs):
    """the set of counting samples changes along a row and down a column; a neighbour in a buffer of its own geometry"""
    cw = (1, 0, 1 + 140, 25)
    prev, cur, nxt = _pictures(78, cw, 1 if pairs else 0)
    for side in ("left", "right", "top", "bottom"):
        for by in (1, 2, 9, 70 if side in ("left", "right") else 13):
            for field in (0, 1):
                _check(cvs, orc, cur[1], cur, _shrunk(prev, side, by), nxt, field, "prev cut %s by %d, field %d" % (side, by, field))
                _check(cvs, orc, cur[1], cur, _shrunk(prev, side, by), _shrunk(nxt, {"left": "top", "right": "bottom", "top": "right", "bottom": "left"}[side], by),
                       field, "prev cut %s and next cut another way by %d, field %d" % (side, by, field))
                _check(cvs, orc, cur[1], cur, _shrunk(prev, side, by), None, field, "only prev, cut %s by %d, field %d" % (side, by, field))
    # neighbours that lie elsewhere: overlapping a corner, and nowhere near
    for dx, dy in ((100, 10), (-135, -22), (141, 0), (0, 26), (500, 500)):
        _check(cvs, orc, cur[1], cur, _moved(prev, dx, dy), nxt, 0, "prev moved by (%d, %d)" % (dx, dy))
        _check(cvs, orc, cur[1], cur, _moved(prev, dx, dy), None, 1, "only prev, moved by (%d, %d)" % (dx, dy))


@pytest.mark.parametrize("pairs", [True, False])
def test_which_neighbours_are_given(cvs, orc, pairs):
    cw = (0, -1, 129, 17)
    prev, cur, nxt = _pictures(79, cw, 0 if pairs else 1)
    empty = lambda f: (f[0], f[1], None)
    for field in (0, 1):
        for what, args, kw in [("prev only", (prev, None), {}), ("next only", (None, nxt), {}), ("neither", (None, None), {}),
                               ("prev empty", (empty(prev), nxt), {}), ("next empty", (prev, empty(nxt)), {}), ("both empty", (empty(prev), empty(nxt)), {}),
                               ("NULL and empty", (None, empty(nxt)), {}), ("prev is next", (prev, None), {"shared": "neighbours"}),
                               ("prev is cur", (None, nxt), {"shared": "cur"}), ("prev is cur, no next", (None, None), {"shared": "cur"})]:
            _check(cvs, orc, cur[1], cur, args[0], args[1], field, "%s, field %d" % (what, field), **kw)


@pytest.mark.parametrize("threshold,softness", [(THRESHOLD, 0.0), (-1.0, SOFTNESS), (-1.0, 0.0), (0.0, SOFTNESS), (0.0, 0.0), (131072.0, SOFTNESS), (131072.0, 0.0),
                                                (THRESHOLD, 1e-42), (THRESHOLD, 3e38)])
def test_thresholds_and_softness(cvs, orc, threshold, softness):
    for width, pad in ((129, 1), (62, 1)):
        cw = (0, 0, width - 1, 16)
        prev, cur, nxt = _pictures(80 + width, cw, pad)
        for field in (0, 1):
            _check(cvs, orc, cur[1], cur, prev, nxt, field, "%dx17 threshold %g softness %g field %d" % (width, threshold, softness, field), threshold, softness)


def test_one_video_frame(cvs, orc):
    cw = (0, 0, 719, 479)
    prev, cur, nxt = _pictures(81, cw)
    k = _check(cvs, orc, cw, cur, prev, nxt, 1, "720x480")
    assert min(dm.classes(k)) >= 0.2


@pytest.mark.parametrize("width,height", [(1, 4194305), (131073, 3)])
def test_tall_and_wide_windows(cvs, orc, width, height):
    """more rows of workgroups than a grid holds (the launcher folds them into longer segments), and a row of more than 2^16
    columns"""
    cw = (0, 0, width - 1, height - 1)
    prev, cur, nxt = _pictures(82, cw, specials=height < 100)
    _check(cvs, orc, cw, cur, prev, nxt, 0 if height > 100 else 1, "%dx%d" % (width, height))


def test_refusals(cvs):
    """every refusal of the contract: -1, its message, an empty window and an unwritten output"""
    full = (0, 0, 15, 15)
    lim = _lib.MAX_COORD
    sentinel = np.broadcast_to(SENTINEL, (16, 16, 4)).copy()
    out = DeviceFrame.from_host(HostFrame(full, np.uint16, sentinel))
    a, b, c = (DeviceFrame.from_host(HostFrame(full, np.uint16, sentinel, full)) for _ in range(3))
    ok = _lib.deinterlace_adaptive(0, 0.05, 0.1)
    nan, inf = float("nan"), float("inf")
    entry = cvs.cvs_deinterlace_adaptive_f16_dev
    box = _lib.box2i.of

    def alias(frame, data, fullw=full, cur=full):
        return _lib.rgba_frame_f16(data, box(*fullw), box(*cur))

    cases = [("need", lambda: entry(out.ref(), a.ref(), None, c.ref(), C.byref(ok), None)),
             ("need", lambda: entry(out.ref(), a.ref(), b.ref(), c.ref(), None, None))]
    cases += [("field", lambda f=f: entry(out.ref(), a.ref(), b.ref(), c.ref(), C.byref(_lib.deinterlace_adaptive(f)), None)) for f in (2, -1)]
    cases += [("flags", lambda f=f: entry(out.ref(), a.ref(), b.ref(), c.ref(), C.byref(_lib.deinterlace_adaptive(0, flags=f)), None)) for f in (1, -1, 0x100)]
    cases += [("threshold", lambda t=t: entry(out.ref(), a.ref(), b.ref(), c.ref(), C.byref(_lib.deinterlace_adaptive(0, t, 0.1)), None)) for t in (nan, inf, -inf)]
    cases += [("softness", lambda t=t: entry(out.ref(), a.ref(), b.ref(), c.ref(), C.byref(_lib.deinterlace_adaptive(0, 0.05, t)), None)) for t in (nan, inf, -inf, -0.5)]
    # (another frame struct over the output's buffer: the output's own struct has an empty window from the first line on)
    cases += [("cannot be one of the inputs", lambda: entry(out.ref(), C.byref(alias(a, out.ptr)), b.ref(), c.ref(), C.byref(ok), None)),
              ("cannot be one of the inputs", lambda: entry(out.ref(), a.ref(), C.byref(alias(b, out.ptr)), c.ref(), C.byref(ok), None)),
              ("cannot be one of the inputs", lambda: entry(out.ref(), a.ref(), b.ref(), C.byref(alias(c, out.ptr)), C.byref(ok), None)),
              ("cannot be one of the inputs", lambda: entry(out.ref(), None, out.ref(), None, C.byref(ok), None))]
    for k in range(3):
        frames = [a.ref(), b.ref(), c.ref()]
        frames[k] = C.byref(alias(None, (a, b, c)[k].ptr, full, (0, 0, 16, 15)))
        cases.append(("outside its buffer", lambda frames=frames: entry(out.ref(), frames[0], frames[1], frames[2], C.byref(ok), None)))
        for fullw, cur in (((lim - 14, 0, lim + 1, 15), (lim - 14, 0, lim, 15)), ((0, -lim - 1, 15, -lim + 14), (0, -lim, 15, -lim + 14)),
                           ((0, 0, 2 ** 31 - 1, 15), full), ((-2 ** 31, 0, 15, 15), full)):
            frames = [a.ref(), b.ref(), c.ref()]
            frames[k] = C.byref(alias(None, (a, b, c)[k].ptr, fullw, cur))
            cases.append(("beyond", lambda frames=frames: entry(out.ref(), frames[0], frames[1], frames[2], C.byref(ok), None)))
    try:
        for word, call in cases:
            out.c.current_window = out.c.full_window
            cvs.cvs_clear_last_error()
            assert call() == -1, word
            assert "cvs_deinterlace_adaptive_f16_dev" in _lib.last_error() and word in _lib.last_error(), (word, _lib.last_error())
            assert out.current_window.is_empty(), word
        far = alias(None, out.ptr, (lim - 14, 0, lim + 1, 15), (0, 0, 15, 15))
        cvs.cvs_clear_last_error()
        assert entry(C.byref(far), a.ref(), b.ref(), c.ref(), C.byref(ok), None) == -1 and "beyond" in _lib.last_error() and far.current_window.is_empty()
        cvs.cvs_clear_last_error()
        assert entry(None, a.ref(), b.ref(), c.ref(), C.byref(ok), None) == -1 and "need" in _lib.last_error()
        _lib.check(cvs.cvs_stream_sync(None), "sync")
        assert np.array_equal(out.download().array, sentinel), "a refused call wrote"
        # an absent neighbour may share the output's buffer: it is never read
        gone = alias(None, out.ptr, full, (0, 0, -1, -1))
        assert entry(out.ref(), C.byref(gone), b.ref(), None, C.byref(ok), None) == 0 and out.current_window.tuple() == full
    finally:
        for f in (out, a, b, c):
            f.free()


# ---------------------------------------------------------------- identities that need no model

def _call(cvs, out_full, frames, order, p):
    (rc, got, window), _ = _run(cvs, _entry(cvs, p, order), out_full, frames)
    assert rc == 0, _lib.last_error()
    return got, window


def _field_to_frame(cvs, out_full, cur, field):
    (rc, got, window), _ = _run(cvs, lambda o, i: cvs.cvs_field_to_frame_f16_dev(o.ref(), i.ref(), field, None), out_full, [cur])
    assert rc == 0, _lib.last_error()
    return got, window


@pytest.mark.parametrize("pairs", [True, False])
def test_identities_with_field_to_frame_as_the_yardstick(cvs, pairs):
    cw = (-2, -1, 140, 35)
    prev, cur, nxt = _pictures(90, cw, 1 if pairs else 0)
    out_full = (cw[0] - 1, cw[1] + 2, cw[2] - 3, cw[3] + 2)
    soft = _lib.deinterlace_adaptive
    for field in (0, 1):
        yard = _field_to_frame(cvs, out_full, cur, field)
        for what, frames, order, p in [("no neighbours", [cur], [None, 0, None], soft(field, THRESHOLD, SOFTNESS)),
                                       ("never static", [cur, prev, nxt], [1, 0, 2], soft(field, -1.0, 0.0)),
                                       ("never static, one neighbour", [cur, nxt], [None, 0, 1], soft(field, -1.0, SOFTNESS))]:
            got = _call(cvs, out_full, frames, order, p)
            assert got[1] == yard[1], (what, field)
            # (the kept rows and everything outside the window code for code; a mean of two NaNs may carry either's payload)
            _compare(got[0], yard[0], _rows_mask(out_full, yard[1], lambda y: (y & 1) == field), "%s, field %d" % (what, field))
        a = _call(cvs, out_full, [cur, prev, nxt], [1, 0, 2], soft(field, THRESHOLD, SOFTNESS))
        b = _call(cvs, out_full, [cur, prev, nxt], [2, 0, 1], soft(field, THRESHOLD, SOFTNESS))
        assert a[1] == b[1] and np.array_equal(a[0], b[0]), "prev and next swapped, field %d" % field
        # tiles equal the whole: split at an even row, an odd row and a column
        whole, window = _call(cvs, cw, [cur, prev, nxt], [1, 0, 2], soft(field, THRESHOLD, SOFTNESS))
        assert window == cw
        for tiles in ([(cw[0], cw[1], cw[2], 9), (cw[0], 10, cw[2], cw[3])], [(cw[0], cw[1], cw[2], 10), (cw[0], 11, cw[2], cw[3])],
                      [(cw[0], cw[1], 60, cw[3]), (61, cw[1], cw[2], cw[3])], [(cw[0], cw[1], 61, cw[3]), (62, cw[1], cw[2], cw[3])]):
            for tile in tiles:
                part, window = _call(cvs, tile, [cur, prev, nxt], [1, 0, 2], soft(field, THRESHOLD, SOFTNESS))
                assert window == tile and np.array_equal(part, fm.crop(whole, cw, tile)), (tile, field)
    # a still picture of finite pixels comes back code for code (a NaN difference counts as motion: inf - inf)
    prev, cur, nxt = _pictures(91, cw, 1 if pairs else 0, specials=False)
    for field in (0, 1):
        got, window = _call(cvs, cw, [cur], [0, 0, 0], soft(field, 0.0, 0.0))
        assert window == cw and np.array_equal(got, fm.crop(cur[0], cur[1], cw)), field
