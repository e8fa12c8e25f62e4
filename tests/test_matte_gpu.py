"""The matte refine on the GPU, bit for bit against the numpy model (tests/matte_model.py; DESIGN.md "Matte refine"), every
entry case under both cvs_set_arithmetic settings with identical codes required.  Every operation of the contract is a correctly
rounded IEEE f32 operation, a comparison or an exact conversion, so there is no tolerance anywhere: one differing code fails.
What is folded before comparing (tests/util.py canon_f16 / canon_f32) is the sign of zero, which the contract leaves open for a
minimum or maximum, and the payload of a NaN.  Target pixels outside the window must keep a sentinel, inputs must come back
unwritten.  No frame is larger than 200 x 70; the tile is 128 x 32 (64 x 32 for windows up to 64 columns), so 129 and 200
columns and 33 and 40 rows take more than one workgroup each way."""
import ctypes as C

import numpy as np
import pytest

from canvas_amd import _lib
from canvas_amd.abi import HostFrame
from canvas_amd.device import DeviceFrame
from tests import key_model as km
from tests import matte_model as mm
from tests.models import f2h_rz_model
from tests.test_fields_gpu import SPECIALS, Tape, _pull
from tests.test_key_gpu import FLAVOURS, SENTINEL16, SENTINEL32, SHOT, _box, _geometries, _same
from tests.test_unsharp_gpu import RASTER, _in_flavour, _pull32

pytestmark = pytest.mark.gpu

GAUSS9 = [float(t) for t in np.float32(np.exp(-0.5 * (np.arange(-4, 5) / 1.5) ** 2) / np.exp(-0.5 * (np.arange(-4, 5) / 1.5) ** 2).sum())]
ROUGH25 = [float(t) for t in np.float32(np.random.default_rng(77).uniform(-0.1, 0.25, 25))]
ROUGH25[3], ROUGH25[12], ROUGH25[20] = -0.0625, 0.0, -0.03125          # unnormalised, with negative taps and a zero tap
FEATHERS = [None, [1.0], [0.25, 0.5, 0.25], GAUSS9, ROUGH25]
CHOKES = [-16, -2, -1, 0, 1, 2, 16]
LEVELS = [(0.0, 1.0), (0.1, 0.9), (0.5, 0.500001)]
TAPS5 = [0.0625, 0.25, 0.375, 0.25, 0.0625]
ODD_ALPHAS = np.array([np.nan, np.inf, -np.inf, 1e-40, -1e-42, 6e-8, 0.0, -0.0, -0.25, 1.5, 37.0, -3.0e38], np.float32)


def _alpha(rng, h, w, kind):
    if kind == "disc":
        return mm.soft_disc(w, h)
    if kind == "keyed":                                              # what the keyer makes of its synthetic shot
        shot = km.green_screen(w, h, int(rng.integers(0, 1000)))
        return km.key_f32(shot, **SHOT)[..., 3]
    return rng.uniform(0, 1, (h, w)).astype(np.float32)


def _pixels(rng, full, half, kind="noise"):
    """RGBA over `full` in the format asked for: random colours, the alpha plane named, then about 3 % of the alphas replaced by
    NaN, +-Inf, subnormals, +-0 and values outside [0, 1]; half frames also get the special half codes of test_fields_gpu.py
    (signalling NaNs, subnormals, the largest finite half, both zeros) in all four channels."""
    h, w = _box(full)
    s = rng.uniform(-0.25, 1.25, (h, w, 4)).astype(np.float32)
    s[..., 3] = _alpha(rng, h, w, kind)
    hit = rng.uniform(size=(h, w)) < 0.03
    s[..., 3][hit] = ODD_ALPHAS[rng.integers(0, len(ODD_ALPHAS), int(hit.sum()))]
    if not half:
        s[..., :3][rng.uniform(size=(h, w, 3)) < 0.01] = np.nan       # colour must come back code for code
        return s
    codes = f2h_rz_model(s)
    scatter = rng.uniform(size=codes.shape) < 0.03
    codes[scatter] = SPECIALS[rng.integers(0, len(SPECIALS), int(scatter.sum()))]
    return codes


def _params(p):
    return _lib.matte(p.get("choke", 0), p.get("feather"), p.get("black", 0.0), p.get("white", 1.0), p.get("show_matte", False))


def _entry(cvs, half):
    return cvs.cvs_matte_refine_f16_dev if half else cvs.cvs_matte_refine_f32_dev


def _refine_once(cvs, half, tfull, sfull, scur, pixels, p):
    """One call on fresh device frames -> (target buffer, window or None, the target beforehand)."""
    dtype, sentinel = (np.uint16, SENTINEL16) if half else (np.float32, SENTINEL32)
    before = np.broadcast_to(sentinel, _box(tfull) + (4,)).copy()
    source = DeviceFrame.from_host(HostFrame(sfull, dtype, pixels, (0, 0, -1, -1) if scur is None else scur))
    target = DeviceFrame.from_host(HostFrame(tfull, dtype, before))
    try:
        m = _params(p)
        rc = _entry(cvs, half)(target.ref(), source.ref(), C.byref(m), None)
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
    want, win = mm.expected(np.broadcast_to(SENTINEL16 if half else SENTINEL32, _box(tfull) + (4,)).copy(), tfull, pixels, sfull, scur, **p)
    results = []
    for flavour, mode in FLAVOURS:
        with _in_flavour(cvs, flavour, mode):
            got, window, _ = _refine_once(cvs, half, tfull, sfull, scur, pixels, p)
        label = "%s %s %s" % (what, "f16" if half else "f32", flavour)
        assert window == win, "%s: window %r, want %r" % (label, window, win)
        _same(got, want, half, label)
        results.append(got)
    assert results[0].tobytes() == results[1].tobytes(), what + ": the two arithmetic settings give different codes"
    return results[0]


def _whole(cvs, width, height, p, rng, what, kind="noise"):
    full = (0, 0, width - 1, height - 1)
    for half in (True, False):
        _check(cvs, half, full, full, full, _pixels(rng, full, half, kind), p, "%dx%d %s %r" % (width, height, what, p))


@pytest.mark.parametrize("width", [1, 2, 63, 64, 65, 129, 200])
def test_widths_and_heights(cvs, width):
    """Either side of a 64-lane strip, of the 64-column and the 128-column tile and of the pair form; heights 1, 2, 2r and
    2r + 1 for r = 2 and r = 16, and 40 (two tiles down)."""
    rng = np.random.default_rng(width)
    settings = {1: dict(choke=1, feather=[0.25, 0.5, 0.25]), 2: dict(choke=-1, feather=GAUSS9, black=0.1, white=0.9),
                4: dict(choke=2, feather=TAPS5), 5: dict(choke=-2, feather=TAPS5, show_matte=True),
                32: dict(choke=16, feather=GAUSS9), 33: dict(choke=-16, feather=ROUGH25, black=0.1, white=0.9),
                40: dict(choke=2, feather=GAUSS9, black=0.1, white=0.9)}
    for height, p in settings.items():
        _whole(cvs, width, height, p, rng, "whole frame")
    _whole(cvs, width, 40, dict(choke=16, feather=ROUGH25), rng, "largest halo")
    _whole(cvs, width, 40, dict(), rng, "identity")


@pytest.mark.parametrize("choke", CHOKES)
def test_parameter_grid(cvs, choke):
    """choke x feather x levels, the matte view on every other combination; 131 x 37: two tiles across, two down."""
    rng = np.random.default_rng(100 + choke)
    full = (-5, -3, 125, 33)
    frames = {True: _pixels(rng, full, True), False: _pixels(rng, full, False)}
    n = 0
    for feather in FEATHERS:
        for black, white in LEVELS:
            for half in (True, False):
                n += 1
                p = dict(choke=choke, feather=feather, black=black, white=white, show_matte=bool(n & 1) ^ half)
                _check(cvs, half, full, full, full, frames[half], p, "grid %r" % (p,))


@pytest.mark.parametrize("show_matte", [False, True])
def test_windows_smaller_than_the_neighbourhood(cvs, show_matte):
    rng = np.random.default_rng(5)
    for width, height in ((5, 3), (3, 5), (1, 1)):
        for choke in (16, -16):
            _whole(cvs, width, height, dict(choke=choke, feather=ROUGH25, show_matte=show_matte), rng, "tiny")
    # a constant matte stays constant: nothing erodes in from the border
    full = (0, 0, 70, 20)
    flat = np.full(_box(full) + (4,), 0.625, np.float32)
    for choke in (16, -16, 3):
        got = _check(cvs, False, full, full, full, flat, dict(choke=choke), "flat")
        assert (got[..., 3] == np.float32(0.625)).all()


def test_geometries(cvs):
    """Every geometry of the keyer's tests at 65 x 37: odd and even left edges, a target reaching beyond the source, the negative
    plane, a source larger and smaller than the target (whose window then sees neighbours outside it), disjoint, no source."""
    rng = np.random.default_rng(65 * 37)
    for gname, sfull, scur, tfull in _geometries(65, 37):
        for half in (True, False):
            pixels = _pixels(rng, sfull, half)
            for p in (dict(choke=2, feather=TAPS5), dict(choke=-2, feather=TAPS5, black=0.1, white=0.9, show_matte=True)):
                _check(cvs, half, tfull, sfull, scur, pixels, p, "65x37 %s" % gname)
    # a target strictly inside a larger source window: the crop of the whole, not the refine of the crop
    sfull, tfull = (0, 0, 199, 69), (37, 11, 171, 58)
    for half in (True, False):
        pixels = _pixels(rng, sfull, half)
        p = dict(choke=3, feather=GAUSS9)
        got = _check(cvs, half, tfull, sfull, sfull, pixels, p, "inner target")
        assert not np.array_equal(got, mm.refine_pixels(mm.crop(pixels, sfull, tfull), **p))


@pytest.mark.parametrize("kind", ["disc", "keyed", "noise"])
def test_alpha_planes(cvs, kind):
    rng = np.random.default_rng(len(kind))
    for p in (dict(choke=1), dict(choke=2, feather=GAUSS9), dict(choke=-1, feather=[0.25, 0.5, 0.25], black=0.1, white=0.9),
              dict(choke=0, feather=GAUSS9, black=0.5, white=0.500001, show_matte=True)):
        _whole(cvs, 200, 70, p, rng, kind, kind)


def test_same_buffer_is_refused_and_unchanged(cvs):
    full = (0, 0, 40, 20)
    rng = np.random.default_rng(8)
    for half in (True, False):
        dtype = np.uint16 if half else np.float32
        pixels = _pixels(rng, full, half)
        frame = DeviceFrame.from_host(HostFrame(full, dtype, pixels, full))
        try:
            cvs.cvs_clear_last_error()
            m = _params(dict(choke=1, feather=TAPS5))
            assert _entry(cvs, half)(frame.ref(), frame.ref(), C.byref(m), None) == -1
            assert "in place" in _lib.last_error() and frame.current_window.is_empty()
            for bad in (dict(choke=17), dict(feather=[0.5, 0.5]), dict(black=0.5, white=0.5)):
                other = DeviceFrame.from_host(HostFrame(full, dtype, pixels))
                try:
                    other.c.current_window = other.c.full_window
                    frame.c.current_window = frame.c.full_window
                    assert _entry(cvs, half)(other.ref(), frame.ref(), C.byref(_params(bad)), None) == -1, bad
                    assert other.current_window.is_empty()
                    _lib.check(cvs.cvs_stream_sync(None), "sync")
                    assert other.download().array.tobytes() == np.ascontiguousarray(pixels).tobytes()
                finally:
                    other.free()
            _lib.check(cvs.cvs_stream_sync(None), "sync")
            assert frame.download().array.tobytes() == np.ascontiguousarray(pixels).tobytes()
        finally:
            frame.free()


# ---------------------------------------------------------------- the node

@pytest.fixture(scope="module")
def process(cvs):
    from fluggo.media import process
    return process


KEY = dict(SHOT, key=(0.25, 0.5, 0.03))


def _key_by_hand(cvs, half, window, codes):
    """The keyer's entry over `window` on the tape's picture -> (buffer over window, its current window)"""
    dtype = np.uint16 if half else np.float32
    source = DeviceFrame.from_host(HostFrame(RASTER, dtype, codes if half else km.widen(codes), RASTER))
    target = DeviceFrame.from_host(HostFrame(window, dtype, np.zeros(_box(window) + (4,), dtype)))
    try:
        key = _lib.chroma_key((C.c_float * 3)(*KEY["key"]), KEY["tolerance"], KEY["softness"], KEY["spill"], KEY["spill_range"], 0)
        assert (cvs.cvs_chroma_key_f16_dev if half else cvs.cvs_chroma_key_f32_dev)(target.ref(), source.ref(), C.byref(key), None) == 0, _lib.last_error()
        _lib.check(cvs.cvs_stream_sync(None), "sync")
        return target.download().array, target.current_window.tuple()
    finally:
        source.free(); target.free()


def test_node_over_the_keyer_equals_the_two_entries_by_hand(cvs, process):
    """Windows inside the tape's raster and reaching beyond it: the node pulls its source over the window grown by |choke| + c,
    so the entries by hand key that grown window and refine it into the window asked for."""
    tape = Tape()
    p = dict(choke=1, feather=TAPS5, black=0.05, white=0.95)
    keyed = process.VideoChromaKeyFilter(tape, tuple(KEY["key"]) + (1.0,), KEY["tolerance"], KEY["softness"], KEY["spill"], KEY["spill_range"])
    node = process.VideoMatteFilter(keyed, p["choke"], p["feather"], p["black"], p["white"])
    codes = tape.picture(4)
    for full in ((10, 3, 30, 20), (-3, -5, 50, 31), (20, 10, 45, 28)):
        grown = (full[0] - 3, full[1] - 3, full[2] + 3, full[3] + 3)
        keyed32, kwin = _key_by_hand(cvs, False, grown, codes)
        assert kwin == km.intersect(grown, RASTER)
        want32, win, _ = _refine_once(cvs, False, full, grown, kwin, keyed32, p)
        assert win == km.intersect(full, RASTER)
        got32, w32 = _pull32(node, 4, full)
        got16, w16 = _pull(node, 4, full)
        assert w32 == win and w16 == win
        assert km.crop(got32, full, win).tobytes() == km.crop(want32, full, win).tobytes(), full
        assert km.crop(got16, full, win).tobytes() == f2h_rz_model(km.crop(want32, full, win)).tobytes(), full
        # and against the model: the refine of the model's key over the whole raster, cropped
        model = mm.crop(mm.refine_pixels(km.key_f32(km.widen(codes), **KEY), **p), RASTER, win)
        _same(km.crop(got32, full, win), model, False, "node against the models %r" % (full,))
    # straight over the half-native tape, pulled as f16: the f16 entry, one launch
    direct = process.VideoMatteFilter(tape, -2, GAUSS9, show_matte=True)
    for full in ((10, 3, 30, 20), (-3, -5, 50, 31)):
        win = km.intersect(full, RASTER)
        got16, w16 = _pull(direct, 4, full)
        assert w16 == win
        _same(km.crop(got16, full, win), mm.crop(mm.refine_pixels(codes, -2, GAUSS9, show_matte=True), RASTER, win), True, "direct f16 pull")


def test_node_parameters_follow_frame_functions_and_refusals_give_empty_windows(cvs, process):
    tape = Tape()
    lerp = process.LerpFunc
    node = process.VideoMatteFilter(tape, choke=lerp((-2.0,), (2.0,), 2.0), feather=TAPS5, black=lerp((0.0,), (0.5,), 2.0), white=lerp((1.0,), (0.75,), 2.0))
    for index in range(3):
        p = dict(choke=-2 + 2 * index, feather=TAPS5, black=0.25 * index, white=1.0 - 0.125 * index)
        codes = tape.picture(index)
        got16, w16 = _pull(node, index, RASTER)
        got32, w32 = _pull32(node, index, RASTER)
        assert w16 == RASTER and w32 == RASTER
        _same(got16, mm.refine_pixels(codes, **p), True, "lerp frame %d" % index)
        _same(got32, mm.refine_pixels(km.widen(codes), **p), False, "lerp frame %d" % index)
    node.choke = lerp((0.0,), (80.0,), 2.0)                         # 40 at frame 1: the entry refuses, the node says why
    cvs.cvs_clear_last_error()
    assert _pull(node, 1, RASTER)[1] is None and "choke" in _lib.last_error()
    assert _pull32(node, 1, RASTER)[1] is None
    assert _pull(node, 0, RASTER)[1] == RASTER
    node.choke = 1
    node.white = 0.0                                                 # white <= black
    assert _pull(node, 0, RASTER)[1] is None and _pull32(node, 0, RASTER)[1] is None
    node.white = 1.0
    assert _pull(node, 0, RASTER)[1] == RASTER
    node.set_source(None)
    assert _pull(node, 0, RASTER)[1] is None and _pull32(node, 0, RASTER)[1] is None
