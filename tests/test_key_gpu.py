"""The chroma key on the GPU, bit for bit against the numpy model (tests/key_model.py; DESIGN.md "Chroma key"), every entry
case under both cvs_set_arithmetic settings with identical codes required.  Every operation of the contract is a correctly
rounded IEEE f32 operation or an exact conversion, so there is no tolerance anywhere: one differing code fails.  What is folded
before comparing (tests/util.py canon_f16 / canon_f32) is the sign of zero and the payload of a NaN, which x86 and gfx950 choose
differently.  Target pixels outside the window must keep a sentinel, inputs must come back unwritten."""
import ctypes as C

import numpy as np
import pytest

import oracle
from canvas_amd import _lib
from canvas_amd.abi import HostFrame
from canvas_amd.device import DeviceFrame
from tests import key_model as km
from tests.models import f2h_rz_model, over_model
from tests.test_fields_gpu import SPECIALS, Tape, _pull
from tests.test_unsharp_gpu import RASTER, _in_flavour, _pull32, _tiles
from tests.util import canon_f16, canon_f32

pytestmark = pytest.mark.gpu

FLAVOURS = [("gcc", _lib.ARITH_SEPARATE), ("fma", _lib.ARITH_CONTRACTED)]
SENTINEL16 = np.array([0x7E17, 0x1234, 0xFBCD, 0x0001], np.uint16)
SENTINEL32 = np.array([1234.5, -7.25, 3.0e-5, 0.4375], np.float32)
SHOT = dict(key=km.GREEN, tolerance=0.08, softness=0.25, spill=0.8, spill_range=0.4, show_matte=False)
# a few settings that between them take every branch: soft and hard edge, spill with and without a range, none, clamped, matte
SETTINGS = [
    SHOT,
    dict(key=km.GREEN, tolerance=0.15, softness=0.0, spill=0.0, spill_range=0.0, show_matte=False),
    dict(key=km.GREEN, tolerance=0.05, softness=0.5, spill=1.5, spill_range=0.0, show_matte=False),
    dict(key=(0.9, -0.1, 1.2), tolerance=0.0, softness=0.1, spill=0.5, spill_range=0.3, show_matte=True),
]


def _box(full):
    return (full[3] - full[1] + 1, full[2] - full[0] + 1)


def _pixels32(rng, full, key=km.GREEN, extremes=True):
    """f32 RGBA over `full`: the synthetic shot where the size allows, colours scattered round the key otherwise (so the ramps
    are live either way), then a scatter of the pixels the contract singles out: the key colour itself, colours below 0 and
    above 1, +-Inf and NaN channels, and (extremes) magnitudes that send the square root down its scaling branches."""
    h, w = _box(full)
    if w >= 16 and h >= 16:
        s = km.green_screen(w, h, int(rng.integers(0, 1000)), key)
        s[..., 3] = rng.uniform(0, 1, (h, w)).astype(np.float32)
    else:
        s = (np.array(tuple(key[:3]) + (0.5,), np.float32) + rng.uniform(-0.4, 0.4, (h, w, 4)).astype(np.float32)).astype(np.float32)
    pool = [np.array(tuple(key[:3]) + (1.0,), np.float32), np.array(tuple(key[:3]) + (0.25,), np.float32),
            np.array([-0.5, 1.5, -0.25, 1.0], np.float32), np.array([2.0, 3.5, 1.25, 0.5], np.float32),
            np.array([np.inf, 0.5, 0.5, 1.0], np.float32), np.array([0.5, -np.inf, 0.5, 0.5], np.float32),
            np.array([0.5, 0.5, np.nan, 0.75], np.float32), np.array([0.25, 0.5, 0.75, np.nan], np.float32),
            np.array([0.25, 0.5, 0.75, np.inf], np.float32), np.array([0.0, -0.0, 0.0, -0.0], np.float32)]
    if extremes:
        pool += [np.array([1e-30, 3e-30, -2e-30, 1.0], np.float32), np.array([1e-42, 0.0, 2e-44, 1.0], np.float32),
                 np.array([1e-20, 1e-21, 3e-20, 0.5], np.float32), np.array([1e18, -3e18, 2e17, 1.0], np.float32),
                 np.array([3e38, 1e38, -3e38, 0.5], np.float32), np.array([6e4, 1e-7, 6.5e4, 1.0], np.float32)]
    hit = rng.uniform(size=(h, w)) < 0.08
    s[hit] = np.stack(pool)[rng.integers(0, len(pool), int(hit.sum()))]
    return s


def _pixels16(rng, full, key=km.GREEN):
    """The same as half codes, with the special halfs of test_fields_gpu.py (signalling NaNs, subnormals, the largest finite
    half, both zeros) scattered over all four channels."""
    codes = f2h_rz_model(_pixels32(rng, full, key, extremes=False))
    scatter = rng.uniform(size=codes.shape) < 0.03
    codes[scatter] = SPECIALS[rng.integers(0, len(SPECIALS), int(scatter.sum()))]
    return codes


def _params(p):
    return _lib.chroma_key((C.c_float * 3)(*p["key"][:3]), p["tolerance"], p["softness"], p["spill"], p["spill_range"],
                           _lib.KEY_SHOW_MATTE if p["show_matte"] else 0)


def _entry(cvs, half):
    return cvs.cvs_chroma_key_f16_dev if half else cvs.cvs_chroma_key_f32_dev


def _same(got, want, half, what):
    g, w = (canon_f16(got), canon_f16(want)) if half else (canon_f32(got), canon_f32(want))
    g, w = g.reshape(got.shape), w.reshape(want.shape)
    if not np.array_equal(g, w):
        raw = (lambda a: a) if half else (lambda a: np.ascontiguousarray(a).view(np.uint32))
        bad = np.argwhere((g != w).any(axis=-1))
        y, x = bad[0]
        raise AssertionError("%s: %d pixels differ; first at buffer row %d column %d: got %s want %s" % (
            what, len(bad), y, x, [hex(int(v)) for v in raw(got)[y, x]], [hex(int(v)) for v in raw(want)[y, x]]))


def _key_once(cvs, half, tfull, sfull, scur, pixels, p):
    """One out-of-place call on fresh device frames -> (target buffer, window or None)."""
    dtype, sentinel = (np.uint16, SENTINEL16) if half else (np.float32, SENTINEL32)
    before = np.broadcast_to(sentinel, _box(tfull) + (4,)).copy()
    source = DeviceFrame.from_host(HostFrame(sfull, dtype, pixels, (0, 0, -1, -1) if scur is None else scur))
    target = DeviceFrame.from_host(HostFrame(tfull, dtype, before))
    try:
        rc = _entry(cvs, half)(target.ref(), source.ref(), C.byref(_params(p)), None)
        _lib.check(cvs.cvs_stream_sync(None), "sync")
        assert rc == 0, _lib.last_error()
        got = target.download().array
        window = None if target.current_window.is_empty() else target.current_window.tuple()
        assert source.download().array.tobytes() == np.ascontiguousarray(pixels).tobytes(), "the input was written"
    finally:
        source.free(); target.free()
    return got, window, before


def _check(cvs, half, tfull, sfull, scur, pixels, p, what):
    """The call under both arithmetic settings: the model's codes, the model's window, and the same codes from both."""
    results = []
    for flavour, mode in FLAVOURS:
        with _in_flavour(cvs, flavour, mode):
            got, window, before = _key_once(cvs, half, tfull, sfull, scur, pixels, p)
        want, win = km.expected(before, tfull, pixels, sfull, scur, **p)
        label = "%s %s %s" % (what, "f16" if half else "f32", flavour)
        assert window == win, "%s: window %r, want %r" % (label, window, win)
        _same(got, want, half, label)
        results.append(got)
    assert results[0].tobytes() == results[1].tobytes(), what + ": the two arithmetic settings give different codes"
    return results[0]


def _geometries(w, h):
    """(name, source full, source current or None, target full)"""
    full = (0, 0, w - 1, h - 1)
    odd = (1, 1 if h > 2 else 0, w - 2 if w > 3 else w - 1, h - 1)              # an odd left edge: off the pair grid
    even = (2 if w > 4 else 0, 0, w - 1 if w < 3 else w - 2, h - 1 if h < 3 else h - 2)   # an even one, an odd right edge
    shifted = (w // 3, -(h // 2) - 1, w // 3 + w - 1, h - (h // 2) - 1)         # the target reaches beyond the source on two sides
    negative = (-w - 3, -h - 2, -4, -3)                                          # the whole plane left of and above the origin
    bigger = (-5, -3, w + 6, h + 2)                                              # a source buffer larger than the target
    inside = (3 if w > 8 else 0, 2 if h > 6 else 0, w - 3 if w > 8 else w - 1, h - 2 if h > 6 else h - 1)
    return [("whole", full, full, full), ("odd left edge", full, odd, full), ("even left edge", full, even, full),
            ("partly outside", full, full, shifted), ("negative plane", negative, negative, (negative[0] + 1, negative[1], negative[2] + 2, negative[3] + 1)),
            ("source larger", bigger, bigger, full), ("source smaller", bigger, inside, bigger), ("odd target base", full, full, (1, 0, w + 1, h - 1)),
            ("disjoint", full, full, (w + 5, 0, 2 * w + 4, h - 1)), ("empty source", full, None, full)]


@pytest.mark.parametrize("width,height", [(333, 71), (64, 36), (17, 9), (130, 3), (2, 5), (1, 1), (1, 7), (5, 1)])
def test_sizes_and_windows(cvs, width, height):
    """Odd widths, one-pixel-wide frames and a 1 x 1 frame; windows on odd and even left edges, so that both the pair and the
    one-pixel form run and pairs are cut on either side; source windows smaller than, larger than and offset against the
    target's buffer; negative plane coordinates; no pixels at all."""
    rng = np.random.default_rng(width * 131 + height)
    for gname, sfull, scur, tfull in _geometries(width, height):
        for half in (True, False):
            pixels = _pixels16(rng, sfull) if half else _pixels32(rng, sfull)
            for i, p in enumerate(SETTINGS):
                _check(cvs, half, tfull, sfull, scur, pixels, p, "%dx%d %s setting %d" % (width, height, gname, i))


@pytest.mark.parametrize("show_matte", [False, True])
def test_parameter_grid(cvs, show_matte):
    rng = np.random.default_rng(21)
    full = (-7, -3, 88, 50)
    frames = {True: _pixels16(rng, full), False: _pixels32(rng, full)}
    for tolerance in (0.0, 0.06, 0.2):
        for softness in (0.0, 0.1, 0.5):
            for spill in (0.0, 0.5, 1.0, 1.5):
                for spill_range in (0.0, 0.3):
                    p = dict(key=km.GREEN, tolerance=tolerance, softness=softness, spill=spill, spill_range=spill_range, show_matte=show_matte)
                    for half in (True, False):
                        got = _check(cvs, half, full, full, full, frames[half], p, "grid %r" % (p,))
                        if spill == 1.5:                               # the clamp: what spill 1 gives
                            one = _key_once(cvs, half, full, full, full, frames[half], dict(p, spill=1.0))[0]
                            assert got.tobytes() == one.tobytes(), p


def test_distance_exactly_at_tolerance(cvs):
    """tolerance set to the very distance of pixels in the frame: the hard edge removes them, the soft ramp starts at them,
    and one code less keeps them."""
    rng = np.random.default_rng(9)
    full = (0, 0, 47, 30)
    for half in (True, False):
        pixels = _pixels16(rng, full) if half else _pixels32(rng, full)
        chosen = np.array([0.25, 0.625, 0.125, 0.875], np.float32)
        planted = rng.uniform(size=_box(full)) < 0.2
        pixels[planted] = f2h_rz_model(chosen) if half else chosen
        d = float(km.distance(chosen[None, None], km.GREEN)[0, 0])
        below = float(np.nextafter(np.float32(d), np.float32(0)))
        assert 0 < below < d
        for tolerance in (d, below):
            for softness, spill_range in ((0.0, 0.0), (0.25, 0.5)):
                p = dict(key=km.GREEN, tolerance=tolerance, softness=softness, spill=0.75, spill_range=spill_range, show_matte=False)
                got = _check(cvs, half, full, full, full, pixels, p, "at tolerance %r" % (p,))
                alpha = got[..., 3][planted]
                if tolerance == d:
                    assert (alpha == 0).all()                          # removed by the hard edge, at the foot of the ramp
                elif softness == 0.0 or not half:                      # (one code up the ramp is below the smallest half)
                    assert (alpha != 0).all()


def test_in_place_equals_out_of_place(cvs):
    rng = np.random.default_rng(33)
    for full, cur in (((0, 0, 200, 40), (0, 0, 200, 40)), ((-3, -2, 96, 37), (0, 1, 91, 30)), ((0, 0, 0, 5), (0, 1, 0, 4))):
        for half in (True, False):
            dtype = np.uint16 if half else np.float32
            pixels = _pixels16(rng, full) if half else _pixels32(rng, full)
            for p in SETTINGS:
                apart, window, _ = _key_once(cvs, half, full, full, cur, pixels, p)
                frame = DeviceFrame.from_host(HostFrame(full, dtype, pixels, cur))
                try:
                    assert _entry(cvs, half)(frame.ref(), frame.ref(), C.byref(_params(p)), None) == 0, _lib.last_error()
                    _lib.check(cvs.cvs_stream_sync(None), "sync")
                    assert frame.current_window.tuple() == window == cur
                    got = frame.download().array
                finally:
                    frame.free()
                assert km.crop(got, full, cur).tobytes() == km.crop(apart, full, cur).tobytes(), (full, half, p)
                outside = np.ones(_box(full), bool)
                km.crop(outside, full, cur)[...] = False
                assert np.array_equal(got[outside].view(np.uint8), np.ascontiguousarray(pixels)[outside].view(np.uint8))     # left as it was


@pytest.mark.timeout(1500)
def test_full_size_frame(cvs):
    """3840 x 2160 compared whole: f16 with the despill, f16 in the matte view, f32 with the despill."""
    full = (0, 0, 3839, 2159)
    rng = np.random.default_rng(4)
    codes = _pixels16(rng, full)
    _check(cvs, True, full, full, full, codes, SHOT, "4K")
    _check(cvs, True, full, full, full, codes, dict(SHOT, show_matte=True, softness=0.0), "4K matte")
    _check(cvs, False, full, full, full, _pixels32(rng, full), SHOT, "4K")


def test_entries_refuse_on_the_device(cvs):
    """With a device present the refusals are the contract's own (not the missing device's), and nothing is written."""
    full = (0, 0, 15, 7)
    for half in (True, False):
        dtype, sentinel = (np.uint16, SENTINEL16) if half else (np.float32, SENTINEL32)
        before = np.broadcast_to(sentinel, _box(full) + (4,)).copy()
        source = DeviceFrame.from_host(HostFrame(full, dtype, before, full))
        target = DeviceFrame.from_host(HostFrame(full, dtype, before))
        try:
            for bad in (dict(tolerance=-0.1), dict(softness=float("nan")), dict(spill_range=float("inf")), dict(key=(0.0, float("nan"), 0.0))):
                cvs.cvs_clear_last_error()
                target.c.current_window = target.c.full_window
                assert _entry(cvs, half)(target.ref(), source.ref(), C.byref(_params(dict(SHOT, **bad))), None) == -1, bad
                assert "finite" in _lib.last_error() and target.current_window.is_empty(), bad
            _lib.check(cvs.cvs_stream_sync(None), "sync")
            assert target.download().array.tobytes() == before.tobytes()
        finally:
            source.free(); target.free()


# ---------------------------------------------------------------- the node

@pytest.fixture(scope="module")
def process(cvs):
    from fluggo.media import process
    return process


@pytest.fixture(scope="module")
def bt():
    from fluggo.media import basetypes
    return basetypes


TAPE_KEY = (0.25, 0.5, 0.03)


def _node_args(p):
    return (tuple(p["key"][:3]) + (1.0,), p["tolerance"], p["softness"], p["spill"], p["spill_range"], p["show_matte"])


def _entry_result(cvs, half, full, sfull, pixels, p):
    got, window, _ = _key_once(cvs, half, full, sfull, sfull, pixels, p)
    return got, window


def test_node_pulls_equal_the_entry_and_tiles_equal_the_whole(cvs, process):
    tape = Tape()
    full = (-3, -5, 50, 31)
    for p in [dict(SHOT, key=TAPE_KEY), dict(SHOT, key=TAPE_KEY, show_matte=True, softness=0.0), dict(SHOT, key=TAPE_KEY, spill=0.0)]:
        node = process.VideoChromaKeyFilter(tape, *_node_args(p))
        codes = tape.picture(2)
        want16, win16 = _entry_result(cvs, True, full, RASTER, codes, p)
        want32, win32 = _entry_result(cvs, False, full, RASTER, km.widen(codes), p)
        got16, w16 = _pull(node, 2, full)
        got32, w32 = _pull32(node, 2, full)
        assert w16 == win16 == RASTER and w32 == win32 == RASTER
        assert km.crop(got16, full, RASTER).tobytes() == km.crop(want16, full, RASTER).tobytes(), p
        assert km.crop(got32, full, RASTER).tobytes() == km.crop(want32, full, RASTER).tobytes(), p
        _same(km.crop(got16, full, RASTER), km.key_pixels(codes, **p), True, "f16 pull against the model")
        _same(km.crop(got32, full, RASTER), km.key_pixels(km.widen(codes), **p), False, "f32 pull against the model")
        alpha = km.crop(got32, full, RASTER)[..., 3]
        if p["softness"] > 0:
            assert ((alpha > 0) & (alpha < 1)).any() and (alpha == 1).any()      # the tape's pixels lie on the ramp and beyond it
        for tile in _tiles(full):
            t16, tw16 = _pull(node, 2, tile)
            t32, tw32 = _pull32(node, 2, tile)
            tw = km.intersect(tile, RASTER)
            assert tw16 == tw and tw32 == tw, (tile, tw16, tw32)
            assert np.array_equal(km.crop(t16, tile, tw), km.crop(got16, full, tw)), ("f16 tile", tile)
            assert np.array_equal(km.crop(t32, tile, tw).view(np.uint32), km.crop(got32, full, tw).view(np.uint32)), ("f32 tile", tile)


def test_node_over_a_device_source_pulled_as_f16(cvs, process, bt):
    """A source that is not half-native (a solid colour): the f16 pull is the f32 render truncated."""
    color, box, full = (0.1, 0.6, 0.15, 0.875), (5, 4, 40, 30), (0, 0, 63, 47)
    p = dict(SHOT, tolerance=0.01, softness=0.2)
    node = process.VideoChromaKeyFilter(process.SolidColorVideoSource(color, bt.box2i(*box)), *_node_args(p))
    s = np.broadcast_to(np.array(color, np.float32), _box(box) + (4,)).copy()
    want = km.key_f32(s, **p)
    got32, w32 = _pull32(node, 0, full)
    got16, w16 = _pull(node, 0, full)
    assert w32 == box and w16 == box
    _same(km.crop(got32, full, box), want, False, "solid f32")
    _same(km.crop(got16, full, box), f2h_rz_model(want), True, "solid f16")
    assert 0 < float(want[0, 0, 3]) < 0.875


def test_parameters_follow_frame_functions(cvs, process):
    tape = Tape()
    lerp = process.LerpFunc
    node = process.VideoChromaKeyFilter(tape, key=lerp((0.25, 0.5, 0.0, 1.0), (0.25, 0.0, 0.5, 1.0), 2.0), tolerance=lerp((0.0,), (0.25,), 2.0),
                                        softness=lerp((0.5,), (0.0,), 2.0), spill=lerp((0.0,), (2.0,), 2.0), spill_range=lerp((0.0,), (0.5,), 2.0))
    for index in range(3):
        p = dict(key=(0.25, 0.5 - 0.25 * index, 0.25 * index), tolerance=0.125 * index, softness=0.5 - 0.25 * index, spill=1.0 * index,
                 spill_range=0.25 * index, show_matte=False)
        codes = tape.picture(index)
        got16, w16 = _pull(node, index, RASTER)
        got32, w32 = _pull32(node, index, RASTER)
        assert w16 == RASTER and w32 == RASTER
        _same(got16, km.key_pixels(codes, **p), True, "lerp frame %d" % index)
        _same(got32, km.key_pixels(km.widen(codes), **p), False, "lerp frame %d" % index)
    # a frame function that yields a negative tolerance: the entry refuses, the node gives an empty window and says why
    node.tolerance = lerp((0.5,), (-0.5,), 2.0)
    cvs.cvs_clear_last_error()
    assert _pull(node, 2, RASTER)[1] is None and "finite" in _lib.last_error()
    assert _pull32(node, 2, RASTER)[1] is None
    assert _pull(node, 0, RASTER)[1] == RASTER
    node.set_source(None)
    assert _pull(node, 0, RASTER)[1] is None and _pull32(node, 0, RASTER)[1] is None


@pytest.mark.parametrize("flavour,mode", FLAVOURS)
def test_keyed_layer_over_a_solid_in_a_workspace(cvs, process, bt, flavour, mode):
    """The workspace pulls the node as f32 (nothing rounded before the over) and blends it over the solid at mix 1.0: the
    model's key, then the over -- tests/models.py over_model in the separate flavour (and the gcc oracle's over must agree
    with it), the contracting oracle build's over in the contracted one, which over_model does not state."""
    with _in_flavour(cvs, flavour, mode):
        tape = Tape()
        full = RASTER
        p = dict(SHOT, key=TAPE_KEY)
        ground = (0.9, 0.1, 0.3, 0.75)
        ws = process.VideoWorkspace()
        ws.add(source=process.SolidColorVideoSource(ground, bt.box2i(*full)), x=0, length=10, z=0, offset=0)
        ws.add(source=process.VideoChromaKeyFilter(tape, *_node_args(p)), x=0, length=10, z=1, offset=0)
        lower = np.broadcast_to(np.array(ground, np.float32), _box(full) + (4,)).copy()
        upper = km.key_f32(km.widen(tape.picture(3)), **p)
        assert ((upper[..., 3] > 0) & (upper[..., 3] < 1)).any()
        acc = HostFrame(full, np.float32, lower.copy(), full)
        oracle.lib().orc_mix_over_f32(acc.ref(), HostFrame(full, np.float32, upper, full).ref(), C.c_float(1.0))
        assert acc.current_window.tuple() == full
        if flavour == "gcc":
            want, wwin = over_model(lower, full, upper, full, full, 1.0)
            assert tuple(wwin) == full
            _same(acc.array, want, False, "the oracle's over against over_model")
        else:
            want = acc.array
        got32, w32 = _pull32(ws, 3, full)
        got16, w16 = _pull(ws, 3, full)
        assert w32 == full and w16 == full
        _same(got32, want, False, "workspace f32 " + flavour)
        _same(got16, f2h_rz_model(want), True, "workspace f16 " + flavour)
