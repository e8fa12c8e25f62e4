"""Field conversions on the GPU, bit for bit against the numpy model of the contract (tests/fields_model.py, DESIGN.md "Field
conversions"): the three device entries on seeded frames with a band of special halfs, at video sizes, odd sizes and random
window configurations, in both arithmetic flavours; the five nodes in round trips that need no model, under tiled pulls, in a
footage chain behind the MPEG-2 import edge, with absent sources, under concurrent set_source and in a long run that must give
its device memory back.  Copied pixels are compared code for code; computed ones with the sign of zero and NaN payloads folded,
as the parity tests do (tests/util.py canon_f16)."""
import ctypes as C
import threading

import numpy as np
import pytest

from canvas_amd import _lib
from canvas_amd.abi import GET_FRAME_F16, HostFrame, video_frame_source_funcs, video_source
from canvas_amd.device import DeviceFrame
from tests import fields_model as fm
from tests.mpeg2_reconstruct_model import reconstruct_model
from tests.util import canon_f16

pytestmark = pytest.mark.gpu

SENTINEL = np.array([0x7E17, 0x1234, 0xFBCD, 0x0001], np.uint16)
SPECIALS = np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x03FF, 0x83FF, 0x0400, 0x7BFF, 0xFBFF, 0x7C00, 0xFC00,
                     0x7E00, 0xFE00, 0x7C01, 0x7DFF, 0xFC01, 0x7FFF, 0xFFFF, 0x3C00, 0xBC00], np.uint16)
FLAVOURS = [("separate", _lib.ARITH_SEPARATE), ("contracted", _lib.ARITH_CONTRACTED)]


def _box(full):
    return (full[3] - full[1] + 1, full[2] - full[0] + 1)


def _pixels(rng, full, layer=0):
    """The project's synthetic layer where the size allows, random in-range halfs otherwise, with a band of special halfs:
    three rows of them a third of the way down (so that specials meet specials vertically) and a scatter elsewhere."""
    from canvas_amd import synth
    h, w = _box(full)
    if w >= 16 and h >= 16:
        codes = synth.layer_pixels(w, h, layer, int(rng.integers(0, 4)), opaque_base=False).copy()
    else:
        codes = rng.integers(0, 0x3C01, (h, w, 4), dtype=np.uint16)
    top = h // 3
    band = codes[top:top + 3]
    band[...] = SPECIALS[rng.integers(0, len(SPECIALS), band.shape)]
    scatter = rng.uniform(size=codes.shape) < 0.02
    codes[scatter] = SPECIALS[rng.integers(0, len(SPECIALS), int(scatter.sum()))]
    return codes


def _window(frame):
    w = frame.current_window
    return None if w.is_empty() else w.tuple()


def _empty_box(win):
    return (0, 0, -1, -1) if win is None else win


def _run(cvs, call, out_full, inputs):
    """call(out, *inputs as device frames) into an output buffer over out_full pre-filled with SENTINEL, in both flavours:
    (rc, codes, window), the same from both."""
    before = np.broadcast_to(SENTINEL, _box(out_full) + (4,)).copy()
    results = []
    for name, mode in FLAVOURS:
        out = DeviceFrame.from_host(HostFrame(out_full, np.uint16, before))
        devs = [DeviceFrame.from_host(HostFrame(full, np.uint16, array, _empty_box(cur))) for array, full, cur in inputs]
        prev = cvs.cvs_set_arithmetic(mode)
        try:
            rc = call(out, *devs)
            _lib.check(cvs.cvs_stream_sync(None), "sync")
        finally:
            cvs.cvs_set_arithmetic(prev if prev >= 0 else _lib.ARITH_SEPARATE)
        results.append((rc, out.download().array, _window(out)))
        for d, (array, _, _) in zip(devs, inputs):
            assert np.array_equal(d.download().array, array), "an input was written"
            d.free()
        out.free()
    assert results[0][0] == results[1][0] and results[0][2] == results[1][2]
    assert np.array_equal(results[0][1], results[1][1]), "the two arithmetic flavours differ"
    return results[0], before


def _compare(got, want, exact, what):
    """exact: mask of pixels that are copies (compared code for code); the others fold -0 and NaN payloads."""
    g = np.where(exact[..., None], got, canon_f16(got))
    w = np.where(exact[..., None], want, canon_f16(want))
    if not np.array_equal(g, w):
        bad = np.argwhere((g != w).any(axis=-1))
        y, x = bad[0]
        raise AssertionError("%s: %d pixels differ; first at buffer row %d column %d: got %s want %s" % (
            what, len(bad), y, x, [hex(v) for v in got[y, x]], [hex(v) for v in want[y, x]]))


def _rows_mask(out_full, window, rows_exact):
    """Everything outside `window` exact (it must keep what it held); inside it, the rows rows_exact(y) says."""
    h, w = _box(out_full)
    mask = np.ones((h, w), bool)
    if window is not None:
        for y in range(window[1], window[3] + 1):
            if not rows_exact(y):
                mask[y - out_full[1], window[0] - out_full[0]:window[2] - out_full[0] + 1] = False
    return mask


def _check_field(cvs, orc, out_full, in_frame, field, what):
    (rc, got, window), before = _run(cvs, lambda o, i: cvs.cvs_field_to_frame_f16_dev(o.ref(), i.ref(), field, None), out_full, [in_frame])
    assert rc == 0, "%s: %s" % (what, _lib.last_error())
    want, want_window = fm.expected_one_input(before, out_full, in_frame, lambda cur, y0: fm.field_to_frame(cur, y0, field, orc.float_to_half))
    assert window == want_window, "%s: window %r, want %r" % (what, window, want_window)
    _compare(got, want, _rows_mask(out_full, window, lambda y: (y & 1) == field), what)


def _check_soften(cvs, orc, out_full, in_frame, what):
    (rc, got, window), before = _run(cvs, lambda o, i: cvs.cvs_soften_fields_f16_dev(o.ref(), i.ref(), None), out_full, [in_frame])
    assert rc == 0, "%s: %s" % (what, _lib.last_error())
    want, want_window = fm.expected_one_input(before, out_full, in_frame, lambda cur, y0: fm.soften(cur, orc.float_to_half))
    assert window == want_window, "%s: window %r, want %r" % (what, window, want_window)
    _compare(got, want, _rows_mask(out_full, window, lambda y: False), what)


def _check_interlace(cvs, out_full, even, odd, what, same=False):
    if same:
        call = lambda o, e: cvs.cvs_interlace_fields_f16_dev(o.ref(), e.ref(), e.ref(), None)
        (rc, got, window), before = _run(cvs, call, out_full, [even])
        odd = even
    else:
        call = lambda o, e, d: cvs.cvs_interlace_fields_f16_dev(o.ref(), e.ref(), d.ref(), None)
        (rc, got, window), before = _run(cvs, call, out_full, [even, odd])
    assert rc == 0, "%s: %s" % (what, _lib.last_error())
    want, want_window = fm.expected_interlace(before, out_full, even, odd)
    assert window == want_window, "%s: window %r, want %r" % (what, window, want_window)
    assert np.array_equal(got, want), what


SIZES = [(64, 36), (720, 480), (1920, 1080), (1, 1), (1, 7), (33, 2), (5, 5)]


@pytest.mark.parametrize("width,height", SIZES)
def test_entries_whole_frames(cvs, orc, width, height):
    rng = np.random.default_rng(width * 31 + height)
    for y0 in (0, -1):
        full = (0, y0, width - 1, y0 + height - 1)
        frame = (_pixels(rng, full), full, full)
        other = (_pixels(rng, full, 1), full, full)
        for field in (0, 1):
            _check_field(cvs, orc, full, frame, field, "field_to_frame %dx%d y0 %d field %d" % (width, height, y0, field))
        _check_soften(cvs, orc, full, frame, "soften %dx%d y0 %d" % (width, height, y0))
        _check_interlace(cvs, full, frame, other, "interlace %dx%d y0 %d" % (width, height, y0))


def _sub_box(rng, full, kind):
    x0, y0, x1, y1 = full
    if kind == "whole":
        return full
    if kind == "row":
        y = int(rng.integers(y0, y1 + 1))
        return (x0, y, x1, y)
    if kind == "column":
        x = int(rng.integers(x0, x1 + 1))
        return (x, y0, x, y1)
    ax, bx = sorted(int(v) for v in rng.integers(x0, x1 + 1, 2))
    ay, by = sorted(int(v) for v in rng.integers(y0, y1 + 1, 2))
    return (ax, ay, bx, by)


def _configurations(seed, count=48):
    """(out_full, in_full, in_current): shifted and negative origins, outputs partly or wholly outside the input's window,
    one-row and one-column windows, odd and even left edges and pitches (both access widths)."""
    rng = np.random.default_rng(seed)
    kinds = ["whole", "row", "column", "any", "any", "any"]
    for n in range(count):
        w, h = int(rng.integers(1, 150)), int(rng.integers(1, 40))
        fx, fy = int(rng.integers(-40, 40)), int(rng.integers(-40, 40))
        in_full = (fx, fy, fx + w - 1, fy + h - 1)
        in_cur = _sub_box(rng, in_full, kinds[n % len(kinds)])
        if n % 8 == 7:                                           # wholly outside the input's current window
            out_full = (in_cur[2] + 1, in_cur[1], in_cur[2] + 9, in_cur[3])
        elif n % 8 == 6:                                         # the same buffer geometry as the input
            out_full = in_full
        else:
            ow, oh = int(rng.integers(1, 150)), int(rng.integers(1, 40))
            ox, oy = in_cur[0] + int(rng.integers(-ow, in_cur[2] - in_cur[0] + 2)), in_cur[1] + int(rng.integers(-oh, in_cur[3] - in_cur[1] + 2))
            out_full = (ox, oy, ox + ow - 1, oy + oh - 1)
        yield rng, out_full, in_full, in_cur


def test_field_to_frame_windows(cvs, orc):
    n = 0
    for rng, out_full, in_full, in_cur in _configurations(101):
        frame = (_pixels(rng, in_full), in_full, in_cur)
        for field in (0, 1):
            _check_field(cvs, orc, out_full, frame, field, "out %r in %r cur %r field %d" % (out_full, in_full, in_cur, field))
        n += 1
    assert n >= 40
    empty = (_pixels(np.random.default_rng(1), (0, 0, 7, 7)), (0, 0, 7, 7), None)
    _check_field(cvs, orc, (0, 0, 7, 7), empty, 0, "empty input")


def test_soften_windows(cvs, orc):
    n = 0
    for rng, out_full, in_full, in_cur in _configurations(202):
        _check_soften(cvs, orc, out_full, (_pixels(rng, in_full), in_full, in_cur), "out %r in %r cur %r" % (out_full, in_full, in_cur))
        n += 1
    assert n >= 40
    empty = (_pixels(np.random.default_rng(1), (0, 0, 7, 7)), (0, 0, 7, 7), None)
    _check_soften(cvs, orc, (0, 0, 7, 7), empty, "empty input")


def test_interlace_windows(cvs):
    n = 0
    for rng, out_full, even_full, even_cur in _configurations(303):
        w, h = int(rng.integers(1, 150)), int(rng.integers(1, 40))
        fx, fy = out_full[0] + int(rng.integers(-30, 30)), out_full[1] + int(rng.integers(-20, 20))
        odd_full = (fx, fy, fx + w - 1, fy + h - 1)
        odd_cur = None if n % 9 == 8 else _sub_box(rng, odd_full, ["any", "whole", "row", "column"][n % 4])
        even = (_pixels(rng, even_full), even_full, None if n % 11 == 10 else even_cur)
        odd = (_pixels(rng, odd_full, 1), odd_full, odd_cur)
        _check_interlace(cvs, out_full, even, odd, "out %r even %r/%r odd %r/%r" % (out_full, even_full, even[2], odd_full, odd_cur))
        if n % 5 == 0:
            _check_interlace(cvs, out_full, even, None, "out %r, one frame on both fields %r/%r" % (out_full, even_full, even[2]), same=True)
        n += 1
    assert n >= 40
    full = (0, 0, 7, 7)
    empty = (_pixels(np.random.default_rng(1), full), full, None)
    _check_interlace(cvs, full, empty, empty, "both inputs empty")


def test_entries_refuse_on_the_device(cvs):
    full = (0, 0, 15, 15)
    out, a = DeviceFrame(full, np.uint16), DeviceFrame(full, np.uint16)
    try:
        for call in (lambda: cvs.cvs_field_to_frame_f16_dev(out.ref(), a.ref(), 2, None), lambda: cvs.cvs_field_to_frame_f16_dev(out.ref(), out.ref(), 0, None),
                     lambda: cvs.cvs_soften_fields_f16_dev(out.ref(), out.ref(), None), lambda: cvs.cvs_interlace_fields_f16_dev(out.ref(), a.ref(), out.ref(), None)):
            out.c.current_window = out.c.full_window
            cvs.cvs_clear_last_error()
            assert call() == -1 and _lib.last_error() and out.current_window.is_empty()
        assert cvs.cvs_field_to_frame_f16_dev(out.ref(), a.ref(), 1, None) == 0 and out.current_window.tuple() == full
    finally:
        out.free(); a.free()


# ---------------------------------------------------------------- the nodes

@pytest.fixture(scope="module")
def process(cvs):
    from fluggo.media import process
    return process


@pytest.fixture(scope="module")
def bt():
    from fluggo.media import basetypes
    return basetypes


RASTER = (0, -2, 45, 28)             # the tape's pictures: 46 columns, rows -2 .. 28


class Tape:
    """A foreign half-native source (host slot only): frame i is a seeded raster over RASTER whose every frame and row differ."""

    def __init__(self, raster=RASTER):
        self.raster = raster
        self._callback = GET_FRAME_F16(self._fill)
        self._funcs = video_frame_source_funcs(0, self._callback, C.cast(None, type(video_frame_source_funcs().get_frame_32)), None)
        C.pythonapi.PyCapsule_New.restype = C.py_object
        C.pythonapi.PyCapsule_New.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p]
        self._video_frame_source_funcs = C.pythonapi.PyCapsule_New(C.addressof(self._funcs), b"_video_frame_source_funcs", None)

    def picture(self, index):
        rng = np.random.default_rng(1000 + index)
        h, w = _box(self.raster)
        codes = rng.integers(0x0001, 0x3C01, (h, w, 4), dtype=np.uint16)
        codes[..., 3] = 0x3C00
        codes[:, :, 2] = (np.arange(h, dtype=np.uint16) + np.uint16(64 * (index % 500) + 0x2000))[:, None]      # a stamp per frame and row
        return codes

    def _fill(self, obj, index, fp):
        f = fp.contents
        full = f.full_window.tuple()
        part = fm.intersect(full, self.raster)
        if part is None or f.full_window.is_empty():
            f.current_window.min.x, f.current_window.min.y, f.current_window.max.x, f.current_window.max.y = 0, 0, -1, -1
            return
        h, w = _box(full)
        arr = np.ctypeslib.as_array(C.cast(f.data, C.POINTER(C.c_uint16)), shape=(h, w, 4))
        fm.crop(arr, full, part)[...] = fm.crop(self.picture(index), self.raster, part)
        f.current_window.min.x, f.current_window.min.y, f.current_window.max.x, f.current_window.max.y = part


def _pull(node, index, full):
    """The node's f16 pull through the C entry a plugin host uses: (codes over `full`, current window or None)."""
    lib = _lib.load()
    C.pythonapi.PyCapsule_GetPointer.restype = C.c_void_p
    C.pythonapi.PyCapsule_GetPointer.argtypes = [C.py_object, C.c_char_p]
    funcs = C.cast(C.pythonapi.PyCapsule_GetPointer(node._video_frame_source_funcs, b"_video_frame_source_funcs"), C.POINTER(video_frame_source_funcs))
    source = video_source(id(node), funcs)
    frame = HostFrame(full, np.uint16)
    lib.video_get_frame_f16(C.byref(source), index, frame.ref())
    return frame.array, _window(frame)


def _same_inside(got, full, window, want, want_full):
    return np.array_equal(fm.crop(got, full, window), fm.crop(want, want_full, window))


@pytest.mark.parametrize("parity", [0, 1])
def test_bob_interlace_of_bob_deinterlace_is_the_source(process, parity):
    tape = Tape()
    node = process.BobInterlaceFilter(process.BobDeinterlaceFilter(tape, parity), parity)
    for full in [(-3, -5, 50, 31), (0, -2, 45, 28), (1, 1, 33, 20), (7, -1, 7, 9)]:
        for i in (-3, -1, 0, 1, 6):
            got, window = _pull(node, i, full)
            assert window == fm.intersect(full, RASTER), (full, i)
            assert _same_inside(got, full, window, tape.picture(i), RASTER), (full, i)


@pytest.mark.parametrize("offset", [0, 1, 2, 3, 4])
def test_pulldown_removal_of_addition_is_the_source(process, offset):
    tape = Tape()
    node = process.Pulldown23RemovalFilter(process.Pulldown23AdditionFilter(tape, offset), offset)
    checked = 0
    for full in [(0, -2, 45, 28), (0, -4, 60, 12), (0, 3, 20, 17)]:          # min.x == 0: the removal's addressing quirk
        for j in range(-9, 12):
            if offset == 4 and (j & 3) == 0:
                continue                                                    # the removal's own offset-4 slip
            got, window = _pull(node, j, full)
            assert window == fm.intersect(full, RASTER), (full, j)
            assert _same_inside(got, full, window, tape.picture(j), RASTER), (full, j)
            checked += 1
    assert checked >= 45


def test_addition_node_weaves_the_frames_the_arithmetic_names(process, orc):
    tape = Tape()
    node = process.Pulldown23AdditionFilter(tape, 1)
    full = (-2, -3, 47, 30)
    for i in range(-6, 7):
        e, o = fm.pulldown23_add(1, i)
        got, window = _pull(node, i, full)
        frames = [(tape.picture(k), RASTER, RASTER) for k in (e, o)]
        assert window == RASTER
        assert np.array_equal(fm.crop(got, full, window), fm.interlace(frames[0], frames[1], window)), i


@pytest.mark.parametrize("kind", ["deinterlace0", "deinterlace1", "weave"])
def test_tiled_pulls_equal_the_pull_in_one_piece(process, orc, kind):
    tape = Tape()
    node = {"deinterlace0": lambda: process.DeinterlaceFilter(tape, 0), "deinterlace1": lambda: process.DeinterlaceFilter(tape, 1),
            "weave": lambda: process.WeaveInterlaceFilter(tape)}[kind]()
    full = (2, -2, 40, 27)
    whole, window = _pull(node, 3, full)
    assert window == full
    picture = (tape.picture(3), RASTER, RASTER)
    op = (lambda cur, y0: fm.soften(cur, orc.float_to_half)) if kind == "weave" else (lambda cur, y0: fm.field_to_frame(cur, y0, int(kind[-1]), orc.float_to_half))
    want, _ = fm.expected_one_input(np.zeros(_box(full) + (4,), np.uint16), full, picture, op)
    assert np.array_equal(canon_f16(whole), canon_f16(want)), "the node against the model"
    for split in (10, 11):                                       # an even and an odd first row of the bottom piece
        top_full, bottom_full = (full[0], full[1], full[2], split - 1), (full[0], split, full[2], full[3])
        top, tw = _pull(node, 3, top_full)
        bottom, bw = _pull(node, 3, bottom_full)
        assert (tw, bw) == (top_full, bottom_full)
        assert np.array_equal(np.concatenate([top, bottom], axis=0), whole), split


def _planes(rng, width, height):
    return [rng.integers(0, 256, s, dtype=np.uint8) for s in [(height, width), (height // 2, width // 2), (height // 2, width // 2)]]


def test_footage_chain(process, bt, orc):
    """CodedImageSource -> MPEG2ReconstructionFilter(interlaced) -> BobDeinterlaceFilter -> f16 pull, each stage against its
    model; then the same frames through a pull queue with two workers."""
    width, height = 64, 32
    rng = np.random.default_rng(9)
    frames = [_planes(rng, width, height) for _ in range(3)]

    class Footage(process.CodedImageSource):
        def get_frame(self, frame):
            return [process.CodedImage(bytearray(p.tobytes()), p.shape[1], p.shape[0]) for p in frames[frame % 3]]

    recon = process.MPEG2ReconstructionFilter(Footage(), size=(width, height), interlaced=True)
    bob = process.BobDeinterlaceFilter(recon, 0)
    table = orc.transfer_table(0)
    raster = (0, 0, width - 1, height - 1)
    full = (-2, -2, width + 1, height + 1)
    want = {}
    for i in range(6):
        picture = reconstruct_model(frames[(i >> 1) % 3], width, height, table, orc.float_to_half, True, "601")
        got, window = _pull(recon, i >> 1, full)
        assert window == raster and np.array_equal(fm.crop(got, full, raster), picture), "reconstruction, frame %d" % (i >> 1)
        want[i] = fm.field_to_frame(picture, 0, i & 1, orc.float_to_half)
        got, window = _pull(bob, i, full)
        assert window == raster, i
        assert np.array_equal(canon_f16(fm.crop(got, full, raster)), canon_f16(want[i])), "bob frame %d" % i

    q = process.VideoPullQueue(workers=2)
    done, seen, lock = threading.Event(), {}, threading.Lock()

    def callback(frame_index, frame, user_data):
        with lock:
            floats = want[frame_index].view(np.float16).astype(np.float64)
            w = frame.current_window
            ok = (w.min.x, w.min.y, w.max.x, w.max.y) == raster
            for y in range(0, height, 3):
                ok = ok and all(tuple(frame.pixel(x, y)) == tuple(floats[y, x]) for x in range(0, width, 5))
            seen[frame_index] = ok
            if len(seen) == 6:
                done.set()

    items = [q.enqueue(source=bob, frame_index=i, window=bt.box2i(*full), callback=callback, user_data=None) for i in range(6)]
    assert done.wait(60), "callbacks did not arrive"
    assert all(seen.values()), seen
    del items


def _nodes(process, source):
    return [process.DeinterlaceFilter(source), process.BobDeinterlaceFilter(source, 1), process.WeaveInterlaceFilter(source),
            process.BobInterlaceFilter(source), process.Pulldown23AdditionFilter(source, 2)]


def test_empty_and_absent_sources_give_empty_windows(process, bt):
    window = bt.box2i(-4, -4, 19, 11)
    for source in (None, process.EmptyVideoSource()):
        for node in _nodes(process, source):
            for i in (-2, 0, 1, 2, 3):
                assert node.get_frame_f16(i, window).current_window.empty(), (type(node).__name__, i)
                assert node.get_frame_f32(i, window).current_window.empty(), (type(node).__name__, i)
    far = bt.box2i(500, 500, 520, 510)                             # a request the source has nothing in
    for node in _nodes(process, Tape()):
        assert node.get_frame_f16(1, far).current_window.empty(), type(node).__name__


def test_set_source_under_concurrent_pulls(process, bt):
    """Pull-queue workers read each node (reader side of its lock, no GIL) while the main thread keeps replacing its source
    (writer side): every pull ends, with the whole window or -- source absent at that moment -- an empty one."""
    window = bt.box2i(0, -2, 45, 28)
    solid = process.SolidColorVideoSource((0.25, 0.5, 0.75, 1.0), bt.box2i(-8, -8, 90, 60))
    for node in _nodes(process, solid):
        q = process.VideoPullQueue(workers=3)
        total, got, all_done = 300, [], threading.Event()

        def callback(frame_index, frame, user_data):
            w = frame.current_window
            got.append(w.empty() or w == window)
            if len(got) == total:
                all_done.set()

        def feeder():
            for i in range(total):
                q.enqueue(node, i % 7 - 3, window, callback, None)

        t = threading.Thread(target=feeder, daemon=True)
        t.start()
        writes = 0
        while not all_done.is_set() and writes < 100000:
            node.set_source(None if writes % 2 == 0 else solid)
            writes += 1
        assert all_done.wait(60), "%s: %d of %d pulls came back after %d writes" % (type(node).__name__, len(got), total, writes)
        t.join(30)
        assert all(got), type(node).__name__
        node.set_source(solid)
        assert node.get_frame_f16(1, window).current_window == window


def test_long_run_gives_device_memory_back(cvs, process, bt):
    def free_bytes():
        f, t = C.c_size_t(), C.c_size_t()
        _lib.check(cvs.cvs_stream_sync(None))
        cvs.cvs_pool_trim()
        _lib.check(cvs.cvs_mem_info(C.byref(f), C.byref(t)))
        return f.value

    source = process.SolidColorVideoSource(process.LerpFunc((0.0, 1.0, 0.25, 1.0), (1.0, 0.0, 0.75, 1.0), 64.0), bt.box2i(-3, -3, 70, 50))
    graph = process.Pulldown23AdditionFilter(process.DeinterlaceFilter(process.BobInterlaceFilter(
        process.BobDeinterlaceFilter(process.WeaveInterlaceFilter(source), 1), 0), 1), 3)
    window = bt.box2i(0, 0, 63, 35)

    def pulls(count):
        for i in range(count):
            assert not graph.get_frame_f16(i % 97 - 20, window).current_window.empty()

    pulls(50)
    start = free_bytes()
    pulls(2000)
    assert free_bytes() == start
