"""Video scopes on the GPU (DESIGN.md "Scopes"): counts and pictures against tests/scope_model.py, with ==.

The bytes the model counts are downloaded from the EXISTING display edge (cvs_frame_to_bytes_dev, RGBA8, for the gamma-0.45
ramp; cvs_frame_to_rgba8_intent_dev for the widget's) on the same device frame: what is measured is what is exported or shown,
and the test restates no ramp.  Every table is pre-filled with 0xFF before the call, so a counter the call does not write, or
does not zero, shows."""
import ctypes as C

import numpy as np
import pytest

import oracle
from canvas_amd import _lib
from canvas_amd.abi import HostFrame, box2i
from canvas_amd.device import DeviceFrame
from tests import scope_model as sm
from tests.entry_cases import all_codes
from tests.models import f2h_rz_model
from tests.test_fields_gpu import RASTER, Tape, _pull
from tests.test_unsharp_gpu import _pull32

pytestmark = pytest.mark.gpu

SENTINEL16 = np.array([0x7E17, 0x1234, 0xFBCD, 0x0001], np.uint16)
KINDS = [sm.HISTOGRAM, sm.WAVEFORM, sm.PARADE, sm.VECTORSCOPE]
KIND_IDS = ["histogram", "waveform", "parade", "vectorscope"]
PICTURE_KINDS, PICTURE_IDS = KINDS[1:], KIND_IDS[1:]
EXPORT, WIDGET = (_lib.LUT_NONE, 0.0), (_lib.LUT_LINEAR_TO_SRGB, 1.25)


@pytest.fixture(scope="module")
def process(cvs):
    from fluggo.media import process
    return process


@pytest.fixture(scope="module")
def bt():
    from fluggo.media import basetypes
    return basetypes


@pytest.fixture(params=["separate", "contracted"])
def flavour(request, cvs):
    before = cvs.cvs_set_arithmetic(_lib.ARITH_CONTRACTED if request.param == "contracted" else _lib.ARITH_SEPARATE)
    yield request.param
    cvs.cvs_set_arithmetic(before if before >= 0 else _lib.ARITH_SEPARATE)


def _size(box):
    return (box[3] - box[1] + 1, box[2] - box[0] + 1)


def _display_bytes(cvs, frame, pre, intent):
    """(h, w, 4) bytes r, g, b, a of the device frame's current window from the display edge; None for an empty window."""
    cur = frame.current_window
    if cur.is_empty():
        return None
    h, w = _size(cur.tuple())
    dev = cvs.cvs_malloc(h * w * 4)
    try:
        if intent > 0:
            rc = cvs.cvs_frame_to_rgba8_intent_dev(dev, frame.ref(), pre, C.c_float(intent), None)
        else:
            rc = cvs.cvs_frame_to_bytes_dev(dev, frame.ref(), pre, _lib.DISPLAY_RGBA8, None)
        _lib.check(rc, "display edge")
        out = np.empty((h, w, 4), np.uint8)
        _lib.check(cvs.cvs_memcpy_d2h(out.ctypes.data, dev, out.nbytes, None), "d2h")
    finally:
        cvs.cvs_free(dev)
    return out


class DeviceTable:
    """Room for `counters` uint32 on the device, 0xFF in every byte until a call writes it."""

    def __init__(self, cvs, counters):
        self.cvs, self.counters = cvs, counters
        self.ptr = cvs.cvs_malloc(counters * 4)
        assert self.ptr
        self.fill(np.full(counters, 0xFFFFFFFF, np.uint32))

    def fill(self, values):
        values = np.ascontiguousarray(values, np.uint32)
        _lib.check(self.cvs.cvs_memcpy_h2d(self.ptr, values.ctypes.data, values.nbytes, None), "h2d")

    def read(self):
        _lib.check(self.cvs.cvs_stream_sync(None), "sync")
        out = np.empty(self.counters, np.uint32)
        _lib.check(self.cvs.cvs_memcpy_d2h(out.ctypes.data, self.ptr, out.nbytes, None), "d2h")
        return out

    def free(self):
        self.cvs.cvs_free(self.ptr)


def _counts(cvs, frame, kind, region, columns=256, display=EXPORT, skip=False):
    """One call of cvs_scope_counts_f16_dev into a table of 0xFF: the table it leaves."""
    p = _lib.scope(kind, region, columns=columns, pre_lut=display[0], rendering_intent=display[1], flags=_lib.SCOPE_SKIP_TRANSPARENT if skip else 0)
    table = DeviceTable(cvs, sm.count(kind, columns))
    try:
        assert cvs.cvs_scope_count(C.byref(p)) == table.counters
        _lib.check(cvs.cvs_scope_counts_f16_dev(table.ptr, frame.ref(), C.byref(p), None), "cvs_scope_counts_f16_dev")
        return table.read()
    finally:
        table.free()


def _same_table(got, want, what):
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError("%s: %d of %d counters differ, first at %d: %d, the model %d (sums %d, %d)" % (
            what, bad.size, got.size, bad[0], got[bad[0]], want[bad[0]], got.astype(np.int64).sum(), want.astype(np.int64).sum()))


def _check(cvs, frame, px, kind, region, columns=256, display=EXPORT, skip=False, what=""):
    cur = frame.current_window
    got = _counts(cvs, frame, kind, region, columns, display, skip)
    want = sm.table(kind, px, None if cur.is_empty() else cur.tuple(), region, columns, skip)
    _same_table(got, want, "%s kind %d region %r columns %d skip %r" % (what, kind, region, columns, skip))
    return got


def _random_codes(rng, h, w):
    """halfs from 0 to 1.0 and a little beyond, a few negative ones and specials: every byte level turns up"""
    codes = rng.integers(0, 0x3D00, (h, w, 4), dtype=np.uint16)
    odd = rng.uniform(size=codes.shape) < 0.03
    codes[odd] = rng.integers(0, 65536, int(odd.sum()), dtype=np.uint16)
    return codes


# ---------------------------------------------------------------- counts

@pytest.mark.parametrize("intent", [0.0, 1.25], ids=["gamma45", "intent1.25"])
@pytest.mark.parametrize("pre", [_lib.LUT_NONE, _lib.LUT_LINEAR_TO_REC709], ids=["none", "rec709"])
def test_every_kind_on_every_half_code(cvs, flavour, pre, intent):
    full = (0, 0, 63, 63)
    frame = DeviceFrame.from_host(all_codes(full, full))
    try:
        px = _display_bytes(cvs, frame, pre, intent)
        assert len(np.unique(px)) > 128
        for kind in KINDS:
            for skip in (False, True):
                got = _check(cvs, frame, px, kind, full, 64, (pre, intent), skip, flavour)
                assert got.sum() > 0
    finally:
        frame.free()


@pytest.mark.parametrize("height", [1, 5, 36])
@pytest.mark.parametrize("width", [1, 63, 64, 65, 129])
def test_lane_and_strip_tails(cvs, width, height):
    """A full window that starts at (-3, -2) with the current window ragged inside it; the region whole, partly outside the
    current window and wholly outside it (zeros)."""
    cur = (-2, -1, -2 + width - 1, -1 + height - 1)
    full = (-3, -2, cur[2] + 2, cur[3] + 1)
    h, w = _size(full)
    frame = DeviceFrame.from_host(HostFrame(full, np.uint16, _random_codes(np.random.default_rng(width * 100 + height), h, w), cur))
    try:
        px = _display_bytes(cvs, frame, *EXPORT)
        regions = [cur, (cur[0] + width // 3, cur[1] - 2, cur[2] + 5, cur[3]), (cur[0] - 4, cur[1] + height // 2, cur[2] - width // 2, cur[3] + 9),
                   (cur[2] + 1, cur[1], cur[2] + 9, cur[3]), (cur[0], cur[3] + 1, cur[2], cur[3] + 2)]
        for kind in KINDS:
            for region in regions:
                got = _check(cvs, frame, px, kind, region, 7, what="%dx%d" % (width, height))
                if sm.intersect(cur, region) is None:
                    assert not got.any()
        # an empty current window: a table of zeros
        frame.c.current_window = box2i.empty()
        for kind in KINDS:
            assert not _counts(cvs, frame, kind, cur, 7).any()
    finally:
        frame.free()


@pytest.mark.parametrize("kind", [sm.WAVEFORM, sm.PARADE], ids=["waveform", "parade"])
def test_column_mapping(cvs, kind):
    """columns 1, 7, the width, more than the width, and the most there is; 65 x 300 so that several workgroups share a strip;
    columns counted from region.min.x, which lies left of the window at negative coordinates."""
    for width, height in [(65, 300), (33, 9)]:
        cur = (-40, -7, -40 + width - 1, -7 + height - 1)
        frame = DeviceFrame.from_host(HostFrame(cur, np.uint16, _random_codes(np.random.default_rng(width), height, width), cur))
        try:
            px = _display_bytes(cvs, frame, *WIDGET)
            for region in [cur, (cur[0] - 5, cur[1], cur[2] + 3, cur[3]), (cur[0] + 2, cur[1] + 1, cur[2] - 1, cur[3])]:
                for columns in (1, 7, width, 100, 4096):
                    _check(cvs, frame, px, kind, region, columns, WIDGET, what="%dx%d" % (width, height))
        finally:
            frame.free()


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_a_flat_frame_and_one_pixel_that_differs(cvs, kind):
    """320 x 256 = 81 920 pixels in ONE counter: more than 16 bits hold, from several workgroups."""
    full = (0, 0, 319, 255)
    codes = np.broadcast_to(np.array([0x3800, 0x3400, 0x3000, 0x3C00], np.uint16), (256, 320, 4)).copy()
    for differing in (False, True):
        if differing:
            codes[200, 171] = (0x3000, 0x3A00, 0x2000, 0x0000)
        frame = DeviceFrame.from_host(HostFrame(full, np.uint16, codes, full))
        try:
            px = _display_bytes(cvs, frame, *EXPORT)
            got = _check(cvs, frame, px, kind, full, 1, what="flat" + (" but one" if differing else ""))
            assert got.max() == 81920 - (1 if differing else 0) and got.max() > 65535
            assert np.count_nonzero(got) == {sm.HISTOGRAM: 5, sm.WAVEFORM: 1, sm.PARADE: 3, sm.VECTORSCOPE: 1}[kind] * (2 if differing else 1)
        finally:
            frame.free()


def test_the_chroma_clamp(cvs):
    """Pure blue and pure red, bytes (0, 0, 255) and (255, 0, 0): Cb = 255 and Cr = 255, not 256."""
    full = (0, 0, 2, 0)
    codes = np.array([[[0, 0, 0x3C00, 0x3C00], [0x3C00, 0, 0, 0x3C00], [0x3C00, 0x3C00, 0x3C00, 0x3C00]]], np.uint16)
    frame = DeviceFrame.from_host(HostFrame(full, np.uint16, codes, full))
    try:
        px = _display_bytes(cvs, frame, *EXPORT)
        assert px[0, :, :3].tolist() == [[0, 0, 255], [255, 0, 0], [255, 255, 255]]
        got = _check(cvs, frame, px, sm.VECTORSCOPE, full).reshape(256, 256)
        cb_red = int(sm.chroma(np.int64(255), np.int64(0), np.int64(0))[0])
        assert got[116, 255] == 1 and got[255, cb_red] == 1 and got[128, 128] == 1 and got.sum() == 3
    finally:
        frame.free()


def test_skip_transparent_goes_by_the_alpha_byte(cvs):
    """A tiny positive alpha is a non-zero half that the ramp maps to byte 0: skipped.  A negative zero as well."""
    full = (0, 0, 7, 3)
    rng = np.random.default_rng(5)
    codes = _random_codes(rng, 4, 8)
    codes[..., 3] = np.array([0x0000, 0x0001, 0x0200, 0x8000, 0x3C00, 0x3800, 0x1000, 0x2400], np.uint16)
    frame = DeviceFrame.from_host(HostFrame(full, np.uint16, codes, full))
    try:
        px = _display_bytes(cvs, frame, *EXPORT)
        zero = px[..., 3] == 0
        assert (zero & (codes[..., 3] != 0)).any() and (~zero).any()
        for kind in KINDS:
            kept = _check(cvs, frame, px, kind, full, 8, skip=True)
            every = _check(cvs, frame, px, kind, full, 8, skip=False)
            rows = {sm.HISTOGRAM: 5, sm.WAVEFORM: 1, sm.PARADE: 3, sm.VECTORSCOPE: 1}[kind]
            assert kept.sum() == int((~zero).sum()) * rows and every.sum() == 32 * rows
    finally:
        frame.free()


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_two_calls_in_a_row_give_the_same_table(cvs, kind):
    full = (0, 0, 99, 40)
    frame = DeviceFrame.from_host(HostFrame(full, np.uint16, _random_codes(np.random.default_rng(9), 41, 100), full))
    p = _lib.scope(kind, full, columns=30)
    table = DeviceTable(cvs, sm.count(kind, 30))
    try:
        want = sm.table(kind, _display_bytes(cvs, frame, *EXPORT), full, full, 30)
        for _ in range(2):
            _lib.check(cvs.cvs_scope_counts_f16_dev(table.ptr, frame.ref(), C.byref(p), None))
            _same_table(table.read(), want, "repeated call")
        for _ in range(2):                              # and back to back, without a look in between
            _lib.check(cvs.cvs_scope_counts_f16_dev(table.ptr, frame.ref(), C.byref(p), None))
        _same_table(table.read(), want, "two calls back to back")
    finally:
        table.free()
        frame.free()


def test_a_recorded_scope_keeps_its_display_table(cvs):
    """display.c keeps 8 byte tables and rewrites an evicted slot in place: a graph that recorded a scope and did not hold the
    table it read would count another intent's bytes on replay (tests/test_graph_replay_gpu.py test_a_graph_holds_its_display_table,
    for the scopes)."""
    from tests.test_graph_replay_gpu import record
    full = (0, 0, 63, 63)
    frame = DeviceFrame.from_host(all_codes(full, full))
    stream = cvs.cvs_stream_create()
    p = _lib.scope(sm.HISTOGRAM, full, rendering_intent=2.0)
    table = DeviceTable(cvs, sm.count(sm.HISTOGRAM, 1))
    graph = None
    try:
        want = sm.table(sm.HISTOGRAM, _display_bytes(cvs, frame, _lib.LUT_NONE, 2.0), full, full)
        _lib.check(cvs.cvs_scope_counts_f16_dev(table.ptr, frame.ref(), C.byref(p), stream))        # warm: the table exists
        _lib.check(cvs.cvs_stream_sync(stream))
        _same_table(table.read(), want, "called directly")
        rc, graph = record(cvs, stream, lambda: cvs.cvs_scope_counts_f16_dev(table.ptr, frame.ref(), C.byref(p), stream))
        assert graph and rc == 0, _lib.last_error()
        others = [sm.table(sm.HISTOGRAM, _display_bytes(cvs, frame, _lib.LUT_NONE, 0.5 + 0.1 * k), full, full) for k in range(12)]    # twelve other tables: every free slot is rewritten
        assert any(not np.array_equal(o, want) for o in others)
        table.fill(np.full(table.counters, 0xFFFFFFFF, np.uint32))
        _lib.check(cvs.cvs_graph_launch(graph, stream), "cvs_graph_launch")
        _lib.check(cvs.cvs_stream_sync(stream))
        _same_table(table.read(), want, "replayed after the cache was churned")
    finally:
        cvs.cvs_stream_sync(stream)
        if graph:
            cvs.cvs_graph_destroy(graph)
        cvs.cvs_stream_destroy(stream)
        table.free()
        frame.free()


def test_the_host_entry(cvs):
    full, cur = (-3, -2, 70, 20), (1, 0, 66, 17)
    h, w = _size(full)
    host = HostFrame(full, np.uint16, _random_codes(np.random.default_rng(11), h, w), cur)
    ch, cw = _size(cur)
    px = np.empty((ch, cw, 4), np.uint8)
    _lib.check(cvs.video_frame_to_bytes(px.ctypes.data, host.ref(), _lib.LUT_NONE, _lib.DISPLAY_RGBA8))
    before = host.array.copy()
    for kind in KINDS:
        for region in [cur, (10, -5, 90, 9)]:
            p = _lib.scope(kind, region, columns=11)
            got = np.full(sm.count(kind, 11), 0xFFFFFFFF, np.uint32)
            _lib.check(cvs.video_scope_counts(got.ctypes.data, host.ref(), C.byref(p)), "video_scope_counts")
            _same_table(got, sm.table(kind, px, cur, region, 11), "host entry, kind %d" % kind)
    empty = HostFrame(full, np.uint16, before, (0, 0, -1, -1))
    got = np.full(sm.count(sm.HISTOGRAM, 1), 0xFFFFFFFF, np.uint32)
    _lib.check(cvs.video_scope_counts(got.ctypes.data, empty.ref(), C.byref(_lib.scope(sm.HISTOGRAM, cur))))
    assert not got.any() and np.array_equal(host.array, before) and host.current_window.tuple() == cur


# ---------------------------------------------------------------- pictures

def _render_counts(kind, columns):
    rng = np.random.default_rng(40 + kind)
    n = rng.integers(0, 40, sm.count(kind, columns)).astype(np.uint32)
    n[rng.uniform(size=n.size) < 0.3] = 0
    n[3], n[4], n[260] = 2 ** 32 - 1, 2 ** 24 + 1, 2 ** 32 - 1
    return n


@pytest.mark.parametrize("kind", PICTURE_KINDS, ids=PICTURE_IDS)
def test_render_against_the_model(cvs, kind):
    """Gains 0, 1/16, 1 and 3.5 over counters that include 2^32 - 1; the place at negative coordinates; targets that hold the
    whole picture, that clip it on each side, and that lie inside it; the parade's panels at 7 columns."""
    columns = 7
    counts = _render_counts(kind, columns)
    table = DeviceTable(cvs, counts.size)
    table.fill(counts)
    pw, ph = sm.picture_size(kind, columns)
    place = (-9, -20, -9 + pw - 1, -20 + ph - 1)
    targets = [(place[0] - 3, place[1] - 4, place[2] + 2, place[3] + 5), (place[0] + 2, place[1] - 1, place[2] + 4, place[3] + 1),
               (place[0] - 2, place[1] + 5, place[2] - 1, place[3] + 1), (place[0] - 1, place[1] - 2, place[2] + 1, place[3] - 7),
               (place[0] + 1, place[1] + 100, place[2] - 1, place[1] + 130), (place[2] + 1, place[1], place[2] + 4, place[3])]
    p = _lib.scope(kind, (0, 0, -1, -1), columns=columns)          # render reads nothing of the region
    try:
        for gain in (0.0, 1.0 / 16.0, 1.0, 3.5):
            want = sm.picture(kind, counts, columns, gain)
            for full in targets:
                h, w = _size(full)
                target = DeviceFrame.from_host(HostFrame(full, np.uint16, np.broadcast_to(SENTINEL16, (h, w, 4)).copy(), full))
                try:
                    _lib.check(cvs.cvs_scope_render_f16_dev(target.ref(), C.byref(box2i.of(*place)), table.ptr, C.byref(p), C.c_float(gain), None), "render")
                    _lib.check(cvs.cvs_stream_sync(None))
                    win = sm.intersect(place, full)
                    assert (None if target.current_window.is_empty() else target.current_window.tuple()) == win, (gain, full)
                    expect = np.broadcast_to(SENTINEL16, (h, w, 4)).copy()
                    if win is not None:
                        expect[win[1] - full[1]:win[3] - full[1] + 1, win[0] - full[0]:win[2] - full[0] + 1] = \
                            want[win[1] - place[1]:win[3] - place[1] + 1, win[0] - place[0]:win[2] - place[0] + 1]
                    got = target.download().array
                    assert np.array_equal(got, expect), "kind %d gain %g target %r: %d pixels differ" % (kind, gain, full, (got != expect).any(axis=-1).sum())
                finally:
                    target.free()
        assert np.array_equal(table.read(), counts)                 # the table is an input
    finally:
        table.free()


# ---------------------------------------------------------------- Python: source.get_scope and VideoScopeFilter

def _tape_bytes(cvs, tape, index, display):
    frame = DeviceFrame.from_host(HostFrame(RASTER, np.uint16, tape.picture(index), RASTER))
    try:
        return _display_bytes(cvs, frame, *display)
    finally:
        frame.free()


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_get_scope(cvs, process, bt, kind):
    tape = Tape()
    for display, name in ((EXPORT, "export"), (WIDGET, "widget")):
        px = _tape_bytes(cvs, tape, 2, display)
        for window in [RASTER, (-3, -5, 50, 31), (5, 3, 30, 12)]:
            raw, cur = tape_scope(process, bt, tape, 2, window, KIND_IDS[kind], columns=9, display=name)
            assert isinstance(raw, bytes) and len(raw) == 4 * sm.count(kind, 9)
            assert (cur.min.x, cur.min.y, cur.max.x, cur.max.y) == sm.intersect(RASTER, window)
            _same_table(np.frombuffer(raw, np.uint32), sm.table(kind, px, RASTER, window, 9), "get_scope %s %r" % (name, window))
    # beside the picture: nothing is defined there, the table holds zeros
    raw, cur = tape_scope(process, bt, tape, 2, (100, 100, 120, 110), KIND_IDS[kind])
    assert cur.max.x < cur.min.x and not np.frombuffer(raw, np.uint32).any() and len(raw) == 4 * sm.count(kind, 256)
    solid = process.SolidColorVideoSource((0.25, 0.5, 0.125, 1.0), bt.box2i(0, 0, 15, 7))
    raw, cur = solid.get_scope(0, bt.box2i(0, 0, 15, 7), KIND_IDS[kind], skip_transparent=True)
    assert np.frombuffer(raw, np.uint32).sum() == 128 * {sm.HISTOGRAM: 5, sm.WAVEFORM: 1, sm.PARADE: 3, sm.VECTORSCOPE: 1}[kind]


def tape_scope(process, bt, tape, index, window, kind, **kw):
    """get_scope is a method of every VideoSource: reach a foreign source through a node that passes it on unchanged."""
    node = process.VideoGainOffsetFilter(tape, 1.0, 0.0)
    return node.get_scope(index, bt.box2i(*window), kind, **kw)


def _node_picture(cvs, tape, index, kind, rect, columns, display, gain, skip=False):
    px = _tape_bytes(cvs, tape, index, display)
    counts = sm.table(kind, px, RASTER, rect, columns, skip)
    return sm.picture(kind, counts, columns, gain)


def _widen(codes):
    return np.ascontiguousarray(codes, np.uint16).view(np.float16).astype(np.float32)


@pytest.mark.parametrize("kind", PICTURE_KINDS, ids=PICTURE_IDS)
def test_node_pulled_as_f16_and_f32(cvs, process, bt, kind):
    tape = Tape()
    rect = (3, -1, 40, 25)
    node = process.VideoScopeFilter(tape, KIND_IDS[kind], bt.box2i(*rect), columns=16, display="widget", gain=0.25)
    want = _node_picture(cvs, tape, 1, kind, rect, 16, WIDGET, 0.25)
    pw, ph = sm.picture_size(kind, 16)
    place = (0, 0, pw - 1, ph - 1)
    for full in [(-3, -4, pw + 5, ph + 2), (2, 10, pw - 3, 200)]:
        win = sm.intersect(place, full)
        crop = want[win[1]:win[3] + 1, win[0]:win[2] + 1]
        got16, w16 = _pull(node, 1, full)
        got32, w32 = _pull32(node, 1, full)
        assert w16 == win and w32 == win
        inside = (slice(win[1] - full[1], win[3] - full[1] + 1), slice(win[0] - full[0], win[2] - full[0] + 1))
        assert np.array_equal(got16[inside], crop), ("f16", kind, full)
        assert np.array_equal(got32[inside].view(np.uint32), _widen(crop).view(np.uint32)), ("f32", kind, full)
    assert want[..., :3].any()
    node.skip_transparent = True
    node.display = "export"
    got16, _ = _pull(node, 1, place)
    assert np.array_equal(got16, _node_picture(cvs, tape, 1, kind, rect, 16, EXPORT, 0.25, True))
    node.set_source(None)
    assert _pull(node, 1, place)[1] is None and _pull32(node, 1, place)[1] is None


def test_gain_follows_a_frame_function(cvs, process, bt):
    tape = Tape()
    node = process.VideoScopeFilter(tape, "waveform", bt.box2i(*RASTER), columns=12, gain=process.LerpFunc((0.0,), (1.0,), 4.0))
    place = (0, 0, 11, 255)
    seen = []
    for index in range(4):
        got, win = _pull(node, index, place)
        assert win == place
        want = _node_picture(cvs, tape, index, sm.WAVEFORM, RASTER, 12, EXPORT, index / 4.0)
        assert np.array_equal(got, want), index
        seen.append(int((got[..., 0] != 0).sum()))
    assert seen[0] == 0 and seen[1] > 0
    node.gain = -1.0                                                 # the entry refuses: an empty window, and it says why
    cvs.cvs_clear_last_error()
    assert _pull(node, 1, place)[1] is None and "gain" in _lib.last_error()


def test_parade_picture_in_picture_over_a_solid(cvs, process, bt):
    """Under a VideoWorkspace: the opaque picture over a solid ground, pulled as f32 and as f16."""
    tape = Tape()
    full = (-4, -6, 59, 269)
    ground = (0.5, 0.25, 0.125, 1.0)
    ws = process.VideoWorkspace()
    ws.add(source=process.SolidColorVideoSource(ground, bt.box2i(*full)), x=0, length=10, z=0, offset=0)
    ws.add(source=process.VideoScopeFilter(tape, "parade", bt.box2i(*RASTER), columns=16, gain=0.5), x=0, length=10, z=1, offset=0)
    h, w = _size(full)
    lower = np.broadcast_to(np.array(ground, np.float32), (h, w, 4)).copy()
    place = (0, 0, 47, 255)
    upper = _widen(_node_picture(cvs, tape, 3, sm.PARADE, RASTER, 16, EXPORT, 0.5))
    acc = HostFrame(full, np.float32, lower.copy(), full)
    oracle.lib().orc_mix_over_f32(acc.ref(), HostFrame(place, np.float32, upper, place).ref(), C.c_float(1.0))
    assert acc.current_window.tuple() == full
    want = acc.array
    assert np.array_equal(want[6:262, 4:52], upper)                  # opaque: the picture covers the ground
    got32, w32 = _pull32(ws, 3, full)
    got16, w16 = _pull(ws, 3, full)
    assert w32 == full and w16 == full
    assert np.array_equal(got32.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got16, f2h_rz_model(want).astype(np.uint16).reshape(got16.shape))
