"""The Catmull-Rom filter of the two warps on the GPU, bit for bit against the numpy model (tests/cubic_model.py; DESIGN.md
"Catmull-Rom warps"), every call under both cvs_set_arithmetic settings with identical codes required, for f16 and f32 frames.
Every operation of the contract is a correctly rounded IEEE f32 operation, a comparison, a minimum or maximum, or an exact
conversion, so there is no tolerance anywhere: one differing code fails.  What is folded before comparing (tests/util.py
canon_f16 / canon_f32) is the sign of zero and the payload of a NaN.  Target pixels outside the window must keep a sentinel,
inputs must come back unwritten.  No frame is larger than 65 x 33: the tile is 32 x 8, so 31, 33 and 65 columns and 1, 2, 7, 8, 9
and 33 rows sit either side of one and two tiles and take several.  Then the two nodes with filter="catmull-rom": whole pulls and
tiles in both formats against the model composed by the rules of tests/graph_model.py, a blur above a turned and above a pinned
layer, and pulls over a workspace against the CPU oracle's over."""
import ctypes as C
import math

import numpy as np
import pytest

import oracle
from canvas_amd import _lib
from canvas_amd.abi import HostFrame
from canvas_amd.device import DeviceFrame
from tests import cubic_cases as cc
from tests import cubic_model as cm
from tests import fields_model as fm
from tests import graph_model as gm
from tests import perspective_cases as pc
from tests import perspective_model as pm
from tests import transform_model as tm
from tests.models import f2h_rz_model
from tests.test_fields_gpu import _pull
from tests.test_key_gpu import FLAVOURS, SENTINEL16, SENTINEL32, _box, _same
from tests.test_perspective_node_gpu import FULL, GENERAL, KEYSTONE, RASTER, Pin, _check_whole_and_tiles, _pulled
from tests.test_perspective_node_gpu import _real as _real_pin
from tests.test_transform_gpu import _pixels
from tests.test_unsharp_gpu import _in_flavour, _pull32, _tiles

pytestmark = pytest.mark.gpu

CUBIC = _lib.TRANSFORM_CATMULL_ROM
WIDTHS, HEIGHTS = [31, 33, 65], (1, 2, 7, 8, 9, 33)
NARROW = [(1, 1), (1, 5), (5, 1), (2, 2), (3, 3)]                    # sources narrower than the filter's support


def _once(cvs, entry, params, half, tfull, sfull, pixels):
    """One call on fresh device frames, the source's window its whole buffer -> (return code, target buffer, window or None)."""
    dtype, sentinel = (np.uint16, SENTINEL16) if half else (np.float32, SENTINEL32)
    before = np.broadcast_to(sentinel, _box(tfull) + (4,)).copy()
    source = DeviceFrame.from_host(HostFrame(sfull, dtype, pixels, sfull))
    target = DeviceFrame.from_host(HostFrame(tfull, dtype, before))
    try:
        rc = entry(target.ref(), source.ref(), C.byref(params), None)
        _lib.check(cvs.cvs_stream_sync(None), "sync")
        got = target.download().array
        window = None if target.current_window.is_empty() else target.current_window.tuple()
        assert source.download().array.tobytes() == np.ascontiguousarray(pixels).tobytes(), "the input was written"
    finally:
        source.free(); target.free()
    return rc, got, window


def _check(cvs, warp, geometry, half, tfull, sfull, pixels, what):
    """The call under both arithmetic settings: the model's codes, the model's window, and the same bytes from both."""
    before = np.broadcast_to(SENTINEL16 if half else SENTINEL32, _box(tfull) + (4,)).copy()
    if warp == "transform":
        entry, params = (cvs.cvs_transform_f16_dev if half else cvs.cvs_transform_f32_dev), _lib.transform(geometry, CUBIC)
        want, win = cm.transform_expected(before, tfull, pixels, sfull, sfull, geometry)
    else:
        entry, params = (cvs.cvs_perspective_f16_dev if half else cvs.cvs_perspective_f32_dev), _lib.perspective(*geometry, filter=CUBIC)
        want, win = cm.perspective_expected(before, tfull, pixels, sfull, sfull, geometry)
    results = []
    for flavour, mode in FLAVOURS:
        with _in_flavour(cvs, flavour, mode):
            rc, got, window = _once(cvs, entry, params, half, tfull, sfull, pixels)
        label = "%s %s %s %s" % (warp, what, "f16" if half else "f32", flavour)
        assert rc == 0, "%s: %s" % (label, _lib.last_error())
        assert window == win, "%s: window %r, want %r" % (label, window, win)
        _same(got, want, half, label)
        results.append(got)
    assert results[0].tobytes() == results[1].tobytes(), what + ": the two arithmetic settings give different bytes"
    return results[0], win


def _source_of(tw, th):
    """Smaller than the target, its window its whole buffer: a clamped tap sits on the allocation's first and last pixel"""
    return (3, 1, tw - 6, th - 2) if th >= 3 else (3, 0, tw - 6, th - 1)


def _quad_cases(cvs, tw, th, sfull):
    """(name, the model's triple) of the three quads of tests/perspective_cases.py; one that is not strictly convex at this
    height has nothing to draw, which the library must say too"""
    out = []
    for name, quad in pc.quads(tw, th, pm.outer(sfull)):
        p = pm.from_quad(pm.outer(sfull), quad)
        r = (C.c_double * 4)(*pm.outer(sfull))
        q = ((C.c_double * 2) * 4)(*[(C.c_double * 2)(float(a), float(b)) for a, b in quad])
        made = _lib.perspective()
        rc = cvs.cvs_perspective_from_quad(r, q, CUBIC, C.byref(made))
        if p is None:
            assert rc == 1, (name, tw, th)
            continue
        assert rc == 0 and (tuple(float(v) for v in made.h), tuple(made.target_origin), tuple(made.source_origin)) == p and made.filter == CUBIC
        out.append((name, p))
    return out


@pytest.mark.parametrize("width", WIDTHS)
def test_the_kernels_are_the_model_bit_for_bit(cvs, width):
    rng = np.random.default_rng(2700 + width)
    drawn = 0
    for height in HEIGHTS:
        tfull = (0, 0, width - 1, height - 1)
        sfull = _source_of(width, height)
        frames = {True: _pixels(rng, sfull, True), False: _pixels(rng, sfull, False)}
        for half in (True, False):
            for name, m in cc.affine_maps(width, height, sfull):
                _check(cvs, "transform", m, half, tfull, sfull, frames[half], "%dx%d %s" % (width, height, name))
            for name, p in _quad_cases(cvs, width, height, sfull):
                _check(cvs, "perspective", p, half, tfull, sfull, frames[half], "%dx%d %s" % (width, height, name))
                drawn += 1
    assert drawn >= 2 * (3 * 4 + 1)                                  # every quad from 7 rows up, the shift at every height


@pytest.mark.parametrize("sw,sh", NARROW)
def test_sources_narrower_than_the_support(cvs, sw, sh):
    """Every tap row or column clamps onto the source's few pixels; nothing outside the allocation is read (the arena harness
    holds the same calls to that with guards)."""
    rng = np.random.default_rng(100 * sw + sh)
    tw, th = 33, 9
    tfull = (0, 0, tw - 1, th - 1)
    sfull = (14, 3, 14 + sw - 1, 3 + sh - 1)
    for half in (True, False):
        pixels = _pixels(rng, sfull, half)
        for name, m in cc.affine_maps(tw, th, sfull) + [("enlarged sixfold", tm.from_parts(anchor=(14, 3), position=(9.25, 1.5), scale=(6, 2.5), rotation=10.0))]:
            _check(cvs, "transform", m, half, tfull, sfull, pixels, "source %dx%d %s" % (sw, sh, name))
        for name, p in _quad_cases(cvs, tw, th, sfull):
            _check(cvs, "perspective", p, half, tfull, sfull, pixels, "source %dx%d %s" % (sw, sh, name))


def test_exact_maps_are_permutations(cvs):
    """Identity, an integer shift, the mirrors and the right-angle rotations move codes, special ones included: asserted against
    numpy's own rot90 and slices, not only against the model."""
    rng = np.random.default_rng(94)
    for w, h in ((33, 9), (65, 33), (7, 40), (1, 1)):
        S = (0, 0, w - 1, h - 1)
        turned = (0, 0, h - 1, w - 1)
        for half in (True, False):
            s = _pixels(rng, S, half)
            bits = (lambda a: a) if half else (lambda a: np.ascontiguousarray(a).view(np.uint32))
            for name, tfull, parts, want in (
                    ("identity", S, {}, s), ("shift", (5, -3, w + 4, h - 4), dict(position=(5, -3)), s),
                    ("mirror x", S, dict(scale=(-1, 1), position=(w - 1, 0)), s[:, ::-1]), ("mirror y", S, dict(scale=(1, -1), position=(0, h - 1)), s[::-1]),
                    ("90", turned, dict(rotation=90, position=(h - 1, 0)), np.rot90(s, -1)), ("180", S, dict(rotation=180, position=(w - 1, h - 1)), np.rot90(s, 2)),
                    ("270", turned, dict(rotation=270, position=(0, w - 1)), np.rot90(s, 1))):
                got, win = _check(cvs, "transform", tm.from_parts(**parts), half, tfull, S, s, "%dx%d %s" % (w, h, name))
                assert win == tfull
                assert np.array_equal(bits(got), bits(np.ascontiguousarray(want))), (w, h, name, half)


def test_an_opaque_flat_layer_and_an_alpha_checker(cvs):
    """The clamp rule on the device: a flat opaque layer turned by 30 degrees and under a keystone is exactly its colour and
    exactly opaque wherever it is drawn from inside; a one-pixel alpha checker with wild colours stays inside the source's range."""
    rng = np.random.default_rng(95)
    tw, th = 65, 33
    tfull, sfull = (0, 0, tw - 1, th - 1), (3, 1, tw - 6, th - 2)
    color = np.array([0.1, 0.6, 0.15, 1.0], np.float32)
    maps = [("transform", cc.affine_maps(tw, th, sfull)[1][1]), ("perspective", pm.from_quad(pm.outer(sfull), pc.quads(tw, th, pm.outer(sfull))[1][1]))]
    for half in (True, False):
        flat = np.broadcast_to(f2h_rz_model(color) if half else color, _box(sfull) + (4,)).copy()
        wild = rng.uniform(-1e4, 1e4, _box(sfull) + (4,)).astype(np.float32)
        yy, xx = np.mgrid[0:wild.shape[0], 0:wild.shape[1]]
        wild[..., 3] = (xx + yy) & 1
        wild = f2h_rz_model(wild) if half else wild
        for warp, geometry in maps:
            got, win = _check(cvs, warp, geometry, half, tfull, sfull, flat, "flat")
            wide = tm.widen(got) if half else got
            inside = tm.crop(wide, tfull, win)
            opaque = inside[..., 3] == 1
            assert opaque.sum() > 500 and (inside[opaque] == (tm.widen(flat) if half else flat)[0, 0]).all()
            assert inside[..., 3].max() == 1 and inside[..., 3].min() == 0
            solid = inside[..., 3] > 0
            assert (inside[solid][:, :3] == (tm.widen(flat) if half else flat)[0, 0][:3]).all()      # the rim keeps the colour exactly
            got, win = _check(cvs, warp, geometry, half, tfull, sfull, wild, "checker")
            inside, src = tm.crop(tm.widen(got) if half else got, tfull, win), (tm.widen(wild) if half else wild)
            drawn = inside[..., 3] > 0
            assert drawn.sum() > 500 and np.isfinite(inside).all()
            for ch in range(3):
                assert inside[..., ch][drawn].min() >= src[..., ch][src[..., 3] > 0].min() and inside[..., ch][drawn].max() <= src[..., ch][src[..., 3] > 0].max()
            assert inside[..., 3].min() >= 0 and inside[..., 3].max() <= 1


# ---------------------------------------------------------------- the nodes

@pytest.fixture(scope="module")
def process(cvs):
    from fluggo.media import process
    return process


@pytest.fixture(scope="module")
def bt():
    from fluggo.media import basetypes
    return basetypes


class CubicTransform(gm.Transform):
    """VideoTransformFilter with filter="catmull-rom": gm.Transform with the windows and the pixels of tests/cubic_model.py"""

    def __init__(self, source, source_rect, anchor=(0.0, 0.0), scale=(1.0, 1.0), rotation=0.0, position=(0.0, 0.0)):
        gm.Transform.__init__(self, source, source_rect, anchor, scale, rotation, position, "catmull-rom")

    def render(self, index, full, fmt):
        before = np.zeros(gm._box(full) + (4,), np.uint16 if fmt == gm.F16 else np.float32)
        m = self.coefficients(index)
        if m is None:
            return before, None
        need = cm.intersect(cm.transform_source_window(m, full), self.source_rect)
        win = None
        if need is not None:
            src, scur = gm.pull(self.sources[0], index, need, fmt)
            before, win = cm.transform_expected(before, full, src, need, scur, m)
        return before, fm.bounding(win, cm.transform_target_window(m, self.source_rect, full))


class CubicPin(Pin):
    """VideoCornerPinFilter with filter="catmull-rom": the Pin of tests/test_perspective_node_gpu.py likewise"""

    def __init__(self, source, source_rect, corners):
        Pin.__init__(self, source, source_rect, corners, "catmull-rom")

    def render(self, index, full, fmt):
        before = np.zeros(gm._box(full) + (4,), np.uint16 if fmt == gm.F16 else np.float32)
        p = self.coefficients(index)
        if p is None:
            return before, None
        need = cm.intersect(cm.perspective_source_window(p, full), self.source_rect)
        if need is not None:
            src, scur = gm.pull(self.sources[0], index, need, fmt)
            before, _win = cm.perspective_expected(before, full, src, need, scur, p)
        quad = self.quad(index)
        xs, ys = [q[0] for q in quad], [q[1] for q in quad]
        bbox = (math.floor(min(xs)) - 1, math.floor(min(ys)) - 1, math.ceil(max(xs)) + 1, math.ceil(max(ys)) + 1)
        return before, cm.intersect(bbox, full)


def _built(process, bt, graph):
    """The real node of a graph whose top is a cubic warp over anything tests/graph_model.py builds"""
    below = gm.build(process, bt, graph.sources[0])
    if isinstance(graph, CubicPin):
        return _real_pin(process, bt, graph, below)
    r = lambda p: gm._real(process, bt, p)          # noqa: E731
    return process.VideoTransformFilter(below, bt.box2i(*graph.source_rect), r(graph.anchor), r(graph.scale), r(graph.rotation), r(graph.position), "catmull-rom")


def _layers(keyed_too=True):
    out = []
    for s, (name, make) in enumerate((
            ("turned 30 degrees", lambda src: CubicTransform(src, RASTER, (23.0, 13.0), (1.25, 0.75), 30.0, (20.0, 12.0))),
            ("part of the source, mirrored and turned", lambda src: CubicTransform(src, (8, 3, 37, 22), (8.0, 3.0), (-1.0, 1.0), 90.0, (30.0, 2.0))),
            ("shifted by a fraction", lambda src: CubicTransform(src, RASTER, position=(0.5, 0.25))),
            ("keystone", lambda src: CubicPin(src, RASTER, KEYSTONE)), ("general quad", lambda src: CubicPin(src, RASTER, GENERAL)),
            ("general quad, part of the source", lambda src: CubicPin(src, (8, 3, 37, 22), GENERAL)))):
        for keyed in ((False, True) if keyed_too else (False,)):
            tape = gm.Tape(RASTER, 60 + s)
            out.append(("%s, %s" % (name, "keyed" if keyed else "tape"), make(gm.Key(tape, gm.TAPE_KEY, 0.0625, 0.5, 0.0, 0.0) if keyed else tape)))
    return out


@pytest.mark.parametrize("what,graph", _layers(), ids=[l[0] for l in _layers()])
def test_tiles_equal_the_whole_pull_and_both_equal_the_model(cvs, process, bt, what, graph):
    """Over a half-native tape the f16 pull goes through the f16 entry (the device slot's own format); over a keyed tape it is
    drawn in f32 and truncated.  Host and device slot: _pull and _pull32 download what the device frame holds."""
    node = _built(process, bt, graph)
    assert node.filter == "catmull-rom"
    for flavour, mode in FLAVOURS:
        with _in_flavour(cvs, flavour, mode):
            _check_whole_and_tiles(graph, node, 2, FULL, "%s %s" % (what, flavour))


@pytest.mark.parametrize("kind", ["transform", "pin"])
def test_a_blurred_cubic_layer_keeps_its_halo_in_a_tile(cvs, process, bt, kind):
    """The window a warp node reports does not depend on the tile it is pulled in -- with this filter too, whose target window
    reaches one pixel further -- so the blur above it has the same halo in a tile as in the whole pull (DESIGN.md "Affine
    transform" has the history)."""
    tape = gm.Tape(RASTER, 19)
    if kind == "transform":
        layer = CubicTransform(tape, RASTER, (22.5, 11.5), (1.375, 1.0), 16.5, (16.5, 16.25))
    else:
        layer = CubicPin(tape, RASTER, ((14.5, 2.25), (43.0, -1.5), (47.5, 24.0), (10.25, 19.5)))
    graph = gm.Blur(layer, "gauss13")
    node = process.VideoBlurFilter(_built(process, bt, layer), tuple(float(t) for t in gm.TAPS["gauss13"]))
    for flavour, mode in FLAVOURS:
        with _in_flavour(cvs, flavour, mode):
            _check_whole_and_tiles(graph, node, 2, FULL, "blur(%s(tape)) %s" % (kind, flavour))
            for half in (True, False):
                whole, win = _pulled(node, 2, FULL, half)
                tile = _tiles(FULL)[1]
                got, twin = _pulled(node, 2, tile, half)
                assert win is not None and twin == pm.intersect(win, tile)
                assert got.tobytes() == np.ascontiguousarray(pm.crop(whole, FULL, tile)).tobytes()


@pytest.mark.parametrize("flavour,mode", FLAVOURS)
@pytest.mark.parametrize("kind", ["transform", "pin"])
def test_a_cubic_layer_over_a_ground_in_a_workspace(cvs, process, bt, kind, flavour, mode):
    """The workspace pulls the node as f32 and blends it over the solid at mix 1.0: the model's layer, then the oracle's over."""
    with _in_flavour(cvs, flavour, mode):
        tape = gm.Tape(RASTER, 31)
        full = RASTER
        if kind == "transform":
            graph = CubicTransform(tape, RASTER, (23.0, 13.0), (0.5, 0.5), 30.0, (22.0, 17.0))
        else:
            graph = CubicPin(gm.Key(tape, gm.TAPE_KEY, 0.0625, 0.5, 0.0, 0.0), RASTER, ((12.5, 6.0), (36.0, 8.5), (40.25, 24.0), (9.0, 21.5)))
        node = _built(process, bt, graph)
        ground = (0.9, 0.1, 0.3, 0.75)
        ws = process.VideoWorkspace()
        ws.add(source=process.SolidColorVideoSource(ground, bt.box2i(*full)), x=0, length=10, z=0, offset=0)
        ws.add(source=node, x=0, length=10, z=1, offset=0)
        lower = np.broadcast_to(np.array(ground, np.float32), gm._box(full) + (4,)).copy()
        upper, win = gm.pull(graph, 3, full, gm.F32)
        alpha = upper[..., 3]
        assert win is not None and win != full and ((alpha > 0) & (alpha < 1)).any()
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
