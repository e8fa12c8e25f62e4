"""VideoCornerPinFilter on the GPU, bit for bit against the model composed by hand: tests/perspective_model.py under the route and
window rules of tests/graph_model.py (a Pin node kind defined here), the CPU oracle's over for the workspace.  Whole pulls and
tiles, both formats, both arithmetic flavours; corners driven by frame functions; a blur above the pin; a keyed layer pinned over
a ground.  A pull promises nothing outside its current window, so both sides are set to zero there.  No tolerance anywhere."""
import ctypes as C
import math

import numpy as np
import pytest

import oracle
from canvas_amd import _lib
from canvas_amd.abi import HostFrame
from tests import graph_model as gm
from tests import perspective_model as pm
from tests.models import f2h_rz_model
from tests.test_fields_gpu import _pull
from tests.test_key_gpu import _same
from tests.test_unsharp_gpu import _in_flavour, _pull32, _tiles

pytestmark = pytest.mark.gpu

FLAVOURS = [("gcc", _lib.ARITH_SEPARATE), ("fma", _lib.ARITH_CONTRACTED)]
FULL = (-3, -5, 50, 31)
RASTER = gm.RASTER
KEYSTONE = ((9.0, 1.5), (35.5, 1.5), (47.25, 27.0), (-1.5, 27.0))
GENERAL = ((4.25, -2.5), (44.0, 3.75), (39.5, 26.125), (-1.75, 19.5))
MIRRORED = tuple(GENERAL[k] for k in (1, 0, 3, 2))
IDENTITY = tuple(pm.rect_quad(pm.outer(RASTER)))


@pytest.fixture(scope="module")
def process(cvs):
    from fluggo.media import process
    return process


@pytest.fixture(scope="module")
def bt():
    from fluggo.media import basetypes
    return basetypes


class Pin(gm.Node):
    """VideoCornerPinFilter: asks for source_window(p, window) clipped to source_rect; reports the quad's bounding box
    [floor(min) - 1, ceil(max) + 1] in the window, transparent where the entry wrote nothing"""
    filter = True

    def __init__(self, source, source_rect, corners, filter="bilinear"):
        self.sources, self.source_rect, self.corners, self.filter_name = (source,), tuple(source_rect), corners, filter

    def quad(self, index):
        return [tuple(gm._f(v) for v in gm.value(c, index)[:2]) for c in self.corners]

    def coefficients(self, index):
        return pm.from_quad(pm.outer(self.source_rect), self.quad(index))

    def render(self, index, full, fmt):
        before = np.zeros(gm._box(full) + (4,), np.uint16 if fmt == gm.F16 else np.float32)
        p = self.coefficients(index)
        if p is None:
            return before, None
        filt = pm.BILINEAR if self.filter_name == "bilinear" else pm.NEAREST
        need = pm.intersect(pm.source_window(p, full), self.source_rect)
        if need is not None:
            src, scur = gm.pull(self.sources[0], index, need, fmt)
            before, _win = pm.expected(before, full, src, need, scur, p, filt)
        quad = self.quad(index)
        xs, ys = [q[0] for q in quad], [q[1] for q in quad]
        bbox = (math.floor(min(xs)) - 1, math.floor(min(ys)) - 1, math.ceil(max(xs)) + 1, math.ceil(max(ys)) + 1)
        return before, pm.intersect(bbox, full)


def _real(process, bt, pin, source):
    corners = tuple(gm._real(process, bt, c) for c in pin.corners)
    return process.VideoCornerPinFilter(source, bt.box2i(*pin.source_rect), corners, pin.filter_name)


def _pulled(node, index, full, half):
    pixels, win = (_pull if half else _pull32)(node, index, full)
    return gm._canvas(pixels, full, win)


def _check_whole_and_tiles(graph, node, index, full, what):
    """Both pulls over `full` equal the model's, window and pixels; the pull over each tile is the crop of the whole pull."""
    for half in (True, False):
        label = "%s frame %d %s window %r" % (what, index, "f16" if half else "f32", full)
        want, wwin = gm.pull(graph, index, full, gm.F16 if half else gm.F32)
        got, win = _pulled(node, index, full, half)
        assert win == wwin, "%s: window %r, the model's %r" % (label, win, wwin)
        _same(got, want, half, label)
        for tile in _tiles(full):
            tgot, twin = _pulled(node, index, tile, half)
            assert twin == (None if win is None else pm.intersect(win, tile)), "%s tile %r: window %r of %r" % (label, tile, twin, win)
            assert tgot.tobytes() == np.ascontiguousarray(pm.crop(got, full, tile)).tobytes(), "%s: tile %r is not the crop of the whole pull" % (label, tile)


@pytest.mark.parametrize("fname", ["nearest", "bilinear"])
def test_tiles_equal_the_whole_pull_and_both_equal_the_model(cvs, process, bt, fname):
    """Over a half-native tape (the f16 pull goes through the f16 entry) and over a keyed tape (drawn in f32, truncated)."""
    for s, (name, rect, corners) in enumerate((("identity", RASTER, IDENTITY), ("keystone", RASTER, KEYSTONE), ("general", RASTER, GENERAL),
                                               ("general mirrored, part of the source", (8, 3, 37, 22), MIRRORED))):
        for keyed in (False, True):
            tape = gm.Tape(RASTER, 40 + s)
            source = gm.Key(tape, gm.TAPE_KEY, 0.0625, 0.5, 0.0, 0.0) if keyed else tape
            graph = Pin(source, rect, corners, fname)
            node = _real(process, bt, graph, gm.build(process, bt, source))
            assert node.coefficients_at(2) == graph.coefficients(2)
            for flavour, mode in FLAVOURS:
                with _in_flavour(cvs, flavour, mode):
                    _check_whole_and_tiles(graph, node, 2, FULL, "%s %s %s %s" % (name, fname, "keyed" if keyed else "tape", flavour))


def test_a_blurred_pinned_layer_keeps_its_halo_in_a_tile(cvs, process, bt):
    """The window the pin reports does not depend on the tile it is pulled in, so the blur above it, which writes nothing outside
    its source's window, has the same halo in a tile as in the whole pull (tests/test_node_graphs_gpu.py
    test_a_blurred_turned_layer_keeps_its_halo_in_a_tile has the history)."""
    tape = gm.Tape(RASTER, 19)
    corners = ((14.5, 2.25), (43.0, -1.5), (47.5, 24.0), (10.25, 19.5))
    graph = gm.Blur(Pin(tape, RASTER, corners), "gauss13")
    pin = _real(process, bt, graph.sources[0], gm.build(process, bt, tape))
    node = process.VideoBlurFilter(pin, tuple(float(t) for t in gm.TAPS["gauss13"]))
    with _in_flavour(cvs, *FLAVOURS[0]):
        _check_whole_and_tiles(graph, node, 2, FULL, "blur(pin(tape))")
        for half in (True, False):
            whole, win = _pulled(node, 2, FULL, half)
            assert win == (9, -3, 49, 25)                                       # the quad's bounding box and its margin
            # the halo above the quad's top edge, inside that margin, in the tile whose pull reaches little of the source
            tile = _tiles(FULL)[1]
            got, twin = _pulled(node, 2, tile, half)
            assert twin == pm.intersect(win, tile) and got.tobytes() == np.ascontiguousarray(pm.crop(whole, FULL, tile)).tobytes()
            assert (pm.crop(whole, FULL, (36, -3, 42, -3))[..., 3] != 0).any()


def test_corners_driven_by_frame_functions(cvs, process, bt):
    lerp = gm.Lerp
    corners = (lerp((0.0, 0.0), (8.0, 4.0), 4.0), (44.5, -1.0), lerp((45.0, 28.0), (37.0, 22.0), 4.0), lerp((0.5, 27.0), (-2.5, 30.0), 4.0))
    tape = gm.Tape(RASTER, 23)
    graph = Pin(tape, RASTER, corners)
    node = _real(process, bt, graph, gm.build(process, bt, tape))
    seen = set()
    with _in_flavour(cvs, *FLAVOURS[0]):
        for index in range(5):
            got = node.coefficients_at(index)
            assert got == graph.coefficients(index) and got is not None
            seen.add(got)
            for half in (True, False):
                want, wwin = gm.pull(graph, index, FULL, gm.F16 if half else gm.F32)
                pixels, win = _pulled(node, index, FULL, half)
                assert win == wwin and win is not None
                _same(pixels, want, half, "frame %d %s" % (index, "f16" if half else "f32"))
    assert len(seen) == 5


def test_a_degenerate_quad_gives_an_empty_window_and_no_exception(cvs, process, bt):
    tape = gm.Tape(RASTER, 29)
    real = gm.build(process, bt, tape)
    rect = bt.box2i(*RASTER)
    node = process.VideoCornerPinFilter(real, rect, KEYSTONE)
    assert _pull(node, 1, FULL)[1] is not None
    for name, corners in (("bow-tie", ((0, 0), (40, 0), (0, 25), (40, 25))), ("concave", ((0, 0), (40, 0), (12, 8), (0, 25))),
                          ("a line", ((0, 0), (10, 10), (20, 20), (30, 30))), ("a point", ((5, 5),) * 4)):
        node.corners = corners
        assert node.corners == corners
        assert node.coefficients_at(1) is None, name
        assert _pull(node, 1, FULL)[1] is None and _pull32(node, 1, FULL)[1] is None, name
    # folding in mid-animation: convex at frame 0, crossed at frame 4
    node.corners = (process.LerpFunc((0.0, 0.0), (40.0, 0.0), 4.0), process.LerpFunc((40.0, 0.0), (0.0, 0.0), 4.0), (40.0, 25.0), (0.0, 25.0))
    assert node.coefficients_at(0) is not None and node.coefficients_at(4) is None and node.coefficients_at(2) is None
    assert _pull(node, 0, FULL)[1] is not None and _pull(node, 4, FULL)[1] is None and _pull32(node, 2, FULL)[1] is None
    # a refused value leaves the old one
    before = node.corners
    for bad in (((0, 0), (1, 1), (2, 2)), 7, ((0, 0), (1, 1), (2, 2), "x"), ((0, 0), (1, 1), (2, 2), (float("nan"), 0))):
        with pytest.raises((TypeError, ValueError)):
            node.corners = bad
    assert node.corners == before
    with pytest.raises((TypeError, ValueError)):
        node.source_rect = (1, 2)
    assert node.source_rect == rect
    with pytest.raises(ValueError):
        node.filter = "bicubic"
    assert node.filter == "bilinear"
    node.filter = "nearest"
    assert node.filter == "nearest"
    # nothing of the tape in source_rect, no source at all
    node.corners = KEYSTONE
    node.source_rect = bt.box2i(100, 100, 120, 120)
    for half in (True, False):
        pixels, win = _pulled(node, 1, FULL, half)
        assert win == (-3, 0, 49, 28) and not pixels.any()              # the quad's box, transparent
    node.source_rect = rect
    node.set_source(None)
    cvs.cvs_clear_last_error()
    assert _pull(node, 1, FULL)[1] is None and _pull32(node, 1, FULL)[1] is None
    assert "cvs_perspective" in _lib.last_error()


@pytest.mark.parametrize("flavour,mode", FLAVOURS)
def test_a_pinned_keyed_layer_over_a_ground_in_a_workspace(cvs, process, bt, flavour, mode):
    """The workspace pulls the node as f32 and blends it over the solid at mix 1.0: the model's layer, then the oracle's over."""
    with _in_flavour(cvs, flavour, mode):
        tape = gm.Tape(RASTER, 31)
        keyed = gm.Key(tape, gm.TAPE_KEY, 0.0625, 0.5, 0.0, 0.0)
        full = RASTER
        corners = ((12.5, 6.0), (36.0, 8.5), (40.25, 24.0), (9.0, 21.5))
        graph = Pin(keyed, RASTER, corners)
        node = _real(process, bt, graph, gm.build(process, bt, keyed))
        ground = (0.9, 0.1, 0.3, 0.75)
        ws = process.VideoWorkspace()
        ws.add(source=process.SolidColorVideoSource(ground, bt.box2i(*full)), x=0, length=10, z=0, offset=0)
        ws.add(source=node, x=0, length=10, z=1, offset=0)
        lower = np.broadcast_to(np.array(ground, np.float32), gm._box(full) + (4,)).copy()
        upper, win = gm.pull(graph, 3, full, gm.F32)
        alpha = upper[..., 3]
        assert win is not None and win != full and ((alpha > 0) & (alpha < 1)).any() and (pm.crop(alpha, full, win) == 0).any()
        # the reference's over picks its `left` frame by comparing the lower window's min.x with the upper's min.y (video_mix.c:265):
        # the layer sits where that picks the geometrically left one, as tests/models.py over_model asks
        assert full[0] < win[1] and full[0] < win[0] and win[2] < full[2]
        acc = HostFrame(full, np.float32, lower.copy(), full)
        oracle.lib().orc_mix_over_f32(acc.ref(), HostFrame(full, np.float32, upper, win).ref(), C.c_float(1.0))
        assert acc.current_window.tuple() == full
        got32, w32 = _pull32(ws, 3, full)
        got16, w16 = _pull(ws, 3, full)
        assert w32 == full and w16 == full
        _same(got32, acc.array, False, "workspace f32 " + flavour)
        _same(got16, f2h_rz_model(acc.array), True, "workspace f16 " + flavour)
