"""The affine transform on the GPU, bit for bit against the numpy model (tests/transform_model.py; DESIGN.md "Affine transform"),
every entry case under both cvs_set_arithmetic settings with identical codes required, for f16 and f32 frames and both filters.
Every operation of the contract is a correctly rounded IEEE f32 operation, a comparison or an exact conversion, so there is no
tolerance anywhere: one differing code fails.  What is folded before comparing (tests/util.py canon_f16 / canon_f32) is the sign
of zero and the payload of a NaN.  Target pixels outside the window must keep a sentinel, inputs must come back unwritten.  No
frame is larger than 200 x 70; the tile is 32 x 8, so widths 31, 32, 33, 63, 64, 65 and heights 7, 8, 9 sit either side of one
and two tiles, and 129, 200 and 33 take several."""
import ctypes as C
import threading

import numpy as np
import pytest

import oracle
from canvas_amd import _lib
from canvas_amd.abi import HostFrame
from canvas_amd.device import DeviceFrame
from tests import transform_model as tm
from tests.models import f2h_rz_model
from tests.test_fields_gpu import SPECIALS, Tape, _pull
from tests.test_key_gpu import FLAVOURS, SENTINEL16, SENTINEL32, _box, _same
from tests.test_unsharp_gpu import RASTER, _in_flavour, _pull32, _tiles

pytestmark = pytest.mark.gpu

FILTERS = [("nearest", tm.NEAREST), ("bilinear", tm.BILINEAR)]
ODD = np.array([np.nan, np.inf, -np.inf, 1e-40, -1e-42, 6e-8, 0.0, -0.0, 0.0, -0.25, 1.5, 37.0, -3.0e38], np.float32)


def _pixels(rng, full, half, specials=True):
    """RGBA over `full` in the format asked for: random colours, alphas in [0, 1], then about 3 % of the pixels get a channel
    replaced by NaN, +-Inf, subnormals, +-0, alpha 0 or a value outside [0, 1]; half frames also get the special half codes of
    test_fields_gpu.py (signalling NaNs, subnormals, the largest finite half, both zeros) in all four channels."""
    h, w = _box(full)
    s = rng.uniform(-0.25, 1.25, (h, w, 4)).astype(np.float32)
    s[..., 3] = rng.uniform(0.0, 1.0, (h, w)).astype(np.float32)
    if specials:
        hit = rng.uniform(size=(h, w, 4)) < np.array([0.005, 0.005, 0.005, 0.02])
        s[hit] = ODD[rng.integers(0, len(ODD), int(hit.sum()))]
    if not half:
        return s
    codes = f2h_rz_model(s)
    if specials:
        scatter = rng.uniform(size=codes.shape) < 0.01
        codes[scatter] = SPECIALS[rng.integers(0, len(SPECIALS), int(scatter.sum()))]
    return codes


def _entry(cvs, half):
    return cvs.cvs_transform_f16_dev if half else cvs.cvs_transform_f32_dev


def _once(cvs, half, tfull, sfull, scur, pixels, m, filt, stream=None):
    """One call on fresh device frames -> (target buffer, window or None)."""
    dtype, sentinel = (np.uint16, SENTINEL16) if half else (np.float32, SENTINEL32)
    before = np.broadcast_to(sentinel, _box(tfull) + (4,)).copy()
    source = DeviceFrame.from_host(HostFrame(sfull, dtype, pixels, (0, 0, -1, -1) if scur is None else scur))
    target = DeviceFrame.from_host(HostFrame(tfull, dtype, before))
    try:
        rc = _entry(cvs, half)(target.ref(), source.ref(), C.byref(_lib.transform(m, filt)), stream)
        _lib.check(cvs.cvs_stream_sync(stream), "sync")
        assert rc == 0, _lib.last_error()
        got = target.download().array
        window = None if target.current_window.is_empty() else target.current_window.tuple()
        assert source.download().array.tobytes() == np.ascontiguousarray(pixels).tobytes(), "the input was written"
    finally:
        source.free(); target.free()
    return got, window


def _expected(half, tfull, sfull, scur, pixels, m, filt):
    before = np.broadcast_to(SENTINEL16 if half else SENTINEL32, _box(tfull) + (4,)).copy()
    return tm.expected(before, tfull, pixels, sfull, scur, m, filt)


def _check(cvs, half, tfull, sfull, scur, pixels, m, filt, what):
    """The call under both arithmetic settings: the model's codes, the model's window, and the same codes from both."""
    want, win = _expected(half, tfull, sfull, scur, pixels, m, filt)
    results = []
    for flavour, mode in FLAVOURS:
        with _in_flavour(cvs, flavour, mode):
            got, window = _once(cvs, half, tfull, sfull, scur, pixels, m, filt)
        label = "%s %s %s %s" % (what, "f16" if half else "f32", "bilinear" if filt else "nearest", flavour)
        assert window == win, "%s: window %r, want %r" % (label, window, win)
        _same(got, want, half, label)
        results.append(got)
    assert results[0].tobytes() == results[1].tobytes(), what + ": the two arithmetic settings give different codes"
    return results[0], win


def _layer_transforms(S):
    """(name, coefficients) of the transforms every size is put through, about the centre of S where that means something"""
    w, h = S[2] - S[0] + 1, S[3] - S[1] + 1
    cx, cy = S[0] + (w - 1) / 2.0, S[1] + (h - 1) / 2.0
    mid = dict(anchor=(cx, cy), position=(cx, cy))
    cases = [("identity", {}), ("shift 3 -2", dict(position=(3, -2))), ("shift 0.5 0.25", dict(position=(0.5, 0.25))),
             ("90", dict(rotation=90, anchor=(S[0], S[1]), position=(S[0] + h - 1, S[1]))),
             ("180", dict(rotation=180, anchor=(S[0], S[1]), position=(S[2], S[3]))),
             ("270", dict(rotation=270, anchor=(S[0], S[1]), position=(S[0], S[1] + w - 1))),
             ("mirror", dict(scale=(-1, 1), anchor=(S[0], S[1]), position=(S[2], S[1]))),
             ("30", dict(mid, rotation=30)), ("-17.5 scaled", dict(mid, rotation=-17.5, scale=(1.5, 0.75))),
             ("half size", dict(mid, scale=(0.5, 0.5))), ("double size", dict(mid, scale=(2, 2))),
             ("flipped and turned", dict(mid, rotation=40, scale=(-1.25, 0.8)))]
    return [(name, tm.from_parts(**parts)) for name, parts in cases]


@pytest.mark.parametrize("width", [1, 2, 31, 32, 33, 63, 64, 65, 129, 200])
def test_widths_and_heights(cvs, width):
    """Every transform in both filters and both formats at heights 1, 2, 7, 8, 9 and 33; the target is the source's own
    rectangle, so the window written is as wide as the frame wherever the layer covers it."""
    rng = np.random.default_rng(width)
    for height in (1, 2, 7, 8, 9, 33):
        full = (0, 0, width - 1, height - 1)
        frames = {True: _pixels(rng, full, True), False: _pixels(rng, full, False)}
        for name, m in _layer_transforms(full):
            for fname, filt in FILTERS:
                for half in (True, False):
                    _check(cvs, half, full, full, full, frames[half], m, filt, "%dx%d %s" % (width, height, name))


@pytest.mark.parametrize("fname,filt", FILTERS)
def test_exact_maps_are_permutations(cvs, fname, filt):
    """Identity, an integer shift, the mirrors and the right-angle rotations move codes, special ones included: asserted against
    numpy's own rot90 and slices, not only against the model."""
    rng = np.random.default_rng(90 + filt)
    for w, h in ((33, 9), (64, 8), (65, 33), (7, 70), (1, 1)):
        S = (0, 0, w - 1, h - 1)
        turned = (0, 0, h - 1, w - 1)
        for half in (True, False):
            s = _pixels(rng, S, half)
            bits = (lambda a: a) if half else (lambda a: np.ascontiguousarray(a).view(np.uint32))
            for name, tfull, parts, want in (
                    ("identity", S, {}, s), ("shift", (5, -3, w + 4, h - 4), dict(position=(5, -3)), s),
                    ("mirror x", S, dict(scale=(-1, 1), position=(w - 1, 0)), s[:, ::-1]), ("mirror y", S, dict(scale=(1, -1), position=(0, h - 1)), s[::-1]),
                    ("90", turned, dict(rotation=90, position=(h - 1, 0)), np.rot90(s, -1)), ("180", S, dict(rotation=180, position=(w - 1, h - 1)), np.rot90(s, 2)),
                    ("270", turned, dict(rotation=270, position=(0, w - 1)), np.rot90(s, 1)), ("-90", turned, dict(rotation=-90, position=(0, w - 1)), np.rot90(s, 1)),
                    ("450 about a corner", turned, dict(rotation=450, anchor=(0, h - 1), position=(0, 0)), np.rot90(s, -1))):
                got, win = _check(cvs, half, tfull, S, S, s, tm.from_parts(**parts), filt, "%dx%d %s" % (w, h, name))
                assert win == tfull
                assert np.array_equal(bits(got), bits(np.ascontiguousarray(want))), (w, h, name, half)


def test_source_windows_inside_their_buffers(cvs):
    """S smaller than and offset inside its buffer, in the negative plane: taps outside S are dropped although the buffer holds
    pixels there (poisoned with NaN colours and alpha 1 here, so that a tap taken from them would show)."""
    rng = np.random.default_rng(41)
    sfull = (-90, -40, -11, 9)
    for scur in ((-71, -33, -20, 2), (-90, -40, -11, 9), (-50, -10, -50, -10), (-89, -39, -12, -39)):
        for half in (True, False):
            pixels = _pixels(rng, sfull, half)
            poison = np.array([0x7E00, 0x7E00, 0x7E00, 0x3C00], np.uint16) if half else np.array([np.nan, np.nan, np.nan, 1.0], np.float32)
            keep = tm.crop(pixels, sfull, scur).copy()
            pixels[...] = poison
            tm.crop(pixels, sfull, scur)[...] = keep
            cx, cy = (scur[0] + scur[2]) / 2.0, (scur[1] + scur[3]) / 2.0
            for name, parts in (("identity", {}), ("shift", dict(position=(0.5, 0.25))), ("turned", dict(anchor=(cx, cy), position=(cx + 2, cy - 1), rotation=30)),
                                ("moved to the positive plane", dict(anchor=(cx, cy), position=(40, 20), rotation=-17.5, scale=(1.5, 0.75)))):
                tfull = (-10, -5, 90, 45) if name.startswith("moved") else (-95, -45, -5, 14)
                for fname, filt in FILTERS:
                    got, win = _check(cvs, half, tfull, sfull, scur, pixels, tm.from_parts(**parts), filt, "S %r %s" % (scur, name))
                    assert win is not None


def test_targets_cropped_larger_and_disjoint(cvs):
    rng = np.random.default_rng(43)
    S = (0, 0, 64, 36)
    m30 = tm.from_parts(anchor=(32, 18), position=(32, 18), rotation=30)
    for half in (True, False):
        pixels = _pixels(rng, S, half)
        for fname, filt in FILTERS:
            # a crop: the target strictly inside the layer, every pixel of it written
            got, win = _check(cvs, half, (20, 10, 44, 26), S, S, pixels, m30, filt, "crop")
            assert win == (20, 10, 44, 26)
            # larger than the image: zeros inside the window beyond the layer, the sentinel outside the window
            tfull = (-60, -16, 130, 53)
            got, win = _check(cvs, half, tfull, S, S, pixels, m30, filt, "larger")
            assert win is not None and win != tfull and win[0] > tfull[0] and win[2] < tfull[2]
            inside = tm.crop(got, tfull, win)
            assert not inside[0, 0].any() and not inside[-1, -1].any()      # the window's corners lie beyond the turned layer
            sentinel = SENTINEL16 if half else SENTINEL32
            assert (got[0, 0] == sentinel).all() and (got[-1, -1] == sentinel).all()
            # disjoint: nothing to draw, rc 0, an empty window, nothing written
            got, win = _check(cvs, half, (200, 0, 260, 36), S, S, pixels, m30, filt, "disjoint")
            assert win is None and (got == sentinel).all()
            # no source window at all
            got, win = _check(cvs, half, S, S, None, pixels, m30, filt, "empty source")
            assert win is None and (got == sentinel).all()


def test_transparent_regions_give_exact_zeros(cvs):
    """Where all four taps have alpha 0 the colour is exactly 0, whatever colour the transparent pixels carry."""
    rng = np.random.default_rng(47)
    S = (0, 0, 69, 39)
    m = tm.from_parts(anchor=(35, 20), position=(35, 20), rotation=30)
    for half in (True, False):
        pixels = _pixels(rng, S, half, specials=False)
        pixels[10:30, 20:55, 3] = 0
        got, win = _check(cvs, half, S, S, S, pixels, m, tm.BILINEAR, "hole")
        u, v = tm.source_coords(m, S)
        i, j = np.floor(u), np.floor(v)
        deep = (i >= 20) & (i + 1 <= 54) & (j >= 10) & (j + 1 <= 29)
        assert deep.sum() > 300 and not got[deep].any()
        edge = tm.widen(got)[..., 3] if half else got[..., 3]
        assert ((edge > 0) & (edge < 1)).any()


def test_two_streams_from_two_threads(cvs):
    """Two calls on two streams from two threads give the single-threaded answer."""
    rng = np.random.default_rng(53)
    S = (0, 0, 199, 69)
    jobs = [(True, _pixels(rng, S, True), tm.from_parts(anchor=(100, 35), position=(100, 35), rotation=30), tm.BILINEAR),
            (False, _pixels(rng, S, False), tm.from_parts(anchor=(100, 35), position=(90, 30), rotation=-17.5, scale=(1.5, 0.75)), tm.BILINEAR)]
    alone = [_once(cvs, half, S, S, S, pixels, m, filt) for half, pixels, m, filt in jobs]
    results, errors = [None, None], []

    def work(k):
        try:
            stream = cvs.cvs_stream_create()
            try:
                half, pixels, m, filt = jobs[k]
                for _ in range(4):
                    results[k] = _once(cvs, half, S, S, S, pixels, m, filt, stream)
            finally:
                cvs.cvs_stream_destroy(stream)
        except BaseException as e:                                   # noqa: BLE001
            errors.append(e)
    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for k in range(2):
        assert results[k][1] == alone[k][1] and results[k][0].tobytes() == alone[k][0].tobytes(), k
        want, win = _expected(jobs[k][0], S, S, S, jobs[k][1], jobs[k][2], jobs[k][3])
        _same(results[k][0], want, jobs[k][0], "thread %d" % k)


def test_refusals_write_nothing(cvs):
    full = (0, 0, 40, 20)
    rng = np.random.default_rng(8)
    for half in (True, False):
        dtype = np.uint16 if half else np.float32
        pixels = _pixels(rng, full, half)
        frame = DeviceFrame.from_host(HostFrame(full, dtype, pixels, full))
        try:
            cvs.cvs_clear_last_error()
            assert _entry(cvs, half)(frame.ref(), frame.ref(), C.byref(_lib.transform()), None) == -1
            assert "in place" in _lib.last_error() and frame.current_window.is_empty()
            for m, filt in (((1, 2, 0, 2, 4, 0), 1), ((1, 0, 0, 0, 1, 0), 2), ((float("nan"), 0, 0, 0, 1, 0), 0)):
                other = DeviceFrame.from_host(HostFrame(full, dtype, pixels))
                try:
                    other.c.current_window = other.c.full_window
                    frame.c.current_window = frame.c.full_window
                    assert _entry(cvs, half)(other.ref(), frame.ref(), C.byref(_lib.transform(m, filt)), None) == -1, (m, filt)
                    assert other.current_window.is_empty()
                    _lib.check(cvs.cvs_stream_sync(None), "sync")
                    assert other.download().array.tobytes() == np.ascontiguousarray(pixels).tobytes()
                finally:
                    other.free()
        finally:
            frame.free()


# ---------------------------------------------------------------- the node

@pytest.fixture(scope="module")
def process(cvs):
    from fluggo.media import process
    return process


@pytest.fixture(scope="module")
def bt():
    from fluggo.media import basetypes
    return basetypes


def _canvas(buffer, full, win):
    """The pulled buffer with everything outside its current window set to zero (a pull promises nothing there)"""
    out = np.zeros_like(buffer)
    if win is not None:
        tm.crop(out, full, win)[...] = tm.crop(buffer, full, win)
    return out


def _node_model(pixels, raster, rect, m, filt, full):
    """What a pull over `full` gives: the source holds `pixels` over `raster`, the node pulls it over the window the taps need,
    clipped to source_rect, and reports where source_rect lands in `full` (transparent black where the entry wrote nothing), so
    that the window does not depend on the tile -> (pixels over full, zero outside the window; the window)"""
    need = tm.intersect(tm.source_window(m, full), rect)
    S = None if need is None else tm.intersect(need, raster)
    out, win = tm.expected(np.zeros(_box(full) + (4,), pixels.dtype), full, pixels, raster, S, m, filt)
    layer = tm.target_window(m, filt, rect, full)
    if win is not None and layer is not None:
        layer = (min(win[0], layer[0]), min(win[1], layer[1]), max(win[2], layer[2]), max(win[3], layer[3]))
    return out, (win if layer is None else layer)


def _as_f32(parts):
    """The parts as the node reads them: every number an f32"""
    return {k: tuple(float(np.float32(c)) for c in v) if isinstance(v, tuple) else float(np.float32(v)) for k, v in parts.items()}


def _check_pulls(node, index, full, codes, raster, rect, filt, what, half_native=True):
    """Both pulls against the model fed with inverse_at(index); returns the two canvases."""
    m = node.inverse_at(index)
    want32, win = _node_model(tm.widen(codes), raster, rect, m, filt, full)
    got32, w32 = _pull32(node, index, full)
    got16, w16 = _pull(node, index, full)
    assert w32 == win and w16 == win, (what, w32, w16, win)
    c32, c16 = _canvas(got32, full, w32), _canvas(got16, full, w16)
    _same(c32, want32, False, what + " f32 pull")
    # a half-native source is warped in half codes by the f16 entry; any other is drawn in f32 and truncated
    want16 = _node_model(codes, raster, rect, m, filt, full)[0] if half_native else f2h_rz_model(want32)
    _same(c16, want16, True, what + " f16 pull")
    return c16, c32, win


@pytest.mark.parametrize("fname,filt", FILTERS)
def test_node_over_a_tape_and_tiles_equal_the_whole(cvs, process, bt, fname, filt):
    tape = Tape()
    full = (-3, -5, 50, 31)
    for rect, parts in ((RASTER, dict(anchor=(23, 13), scale=(1.25, 0.8), rotation=30.0, position=(20, 12))),
                        ((8, 3, 37, 22), dict(anchor=(8, 3), scale=(-1, 1), rotation=90.0, position=(30, 2))),      # source_rect bounds what is pulled
                        (RASTER, dict()), (RASTER, dict(position=(0.5, 0.25)))):
        node = process.VideoTransformFilter(tape, bt.box2i(*rect), filter=fname, **parts)
        assert node.inverse_at(2) == tm.from_parts(**_as_f32(parts))
        codes = tape.picture(2)
        c16, c32, win = _check_pulls(node, 2, full, codes, RASTER, rect, filt, "tape %r" % (parts,))
        assert win is not None
        for tile in _tiles(full):
            t16, t32, twin = _check_pulls(node, 2, tile, codes, RASTER, rect, filt, "tile %r of %r" % (tile, parts))
            assert np.array_equal(t16, tm.crop(c16, full, tile)), ("f16 tile", tile, parts)
            assert np.array_equal(t32.view(np.uint32), np.ascontiguousarray(tm.crop(c32, full, tile)).view(np.uint32)), ("f32 tile", tile, parts)


def test_node_follows_frame_functions_over_several_frames(cvs, process, bt):
    tape = Tape()
    lerp = process.LerpFunc
    node = process.VideoTransformFilter(tape, bt.box2i(*RASTER), anchor=(23, 13), position=lerp((23.0, 13.0), (27.0, 9.0), 4.0), rotation=lerp((0.0,), (120.0,), 4.0),
                                        scale=lerp((1.0, 1.0), (0.5, 2.0), 4.0))
    seen = set()
    for index in range(5):
        m = node.inverse_at(index)
        assert m == tm.from_parts((23, 13), (1.0 - 0.125 * index, 1.0 + 0.25 * index), 30.0 * index, (23.0 + index, 13.0 - index))
        seen.add(m)
        _check_pulls(node, index, RASTER, tape.picture(index), RASTER, RASTER, tm.BILINEAR, "frame %d" % index)
    assert len(seen) == 5
    assert node.inverse_at(0) == (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)      # frame 0 is the identity: it went through the kernel like the rest
    # degenerate, refused and absent: empty windows, no exception
    node.scale = lerp((1.0, 1.0), (0.0, 1.0), 4.0)
    assert node.inverse_at(4) is None and _pull(node, 4, RASTER)[1] is None and _pull32(node, 4, RASTER)[1] is None
    assert _pull(node, 2, RASTER)[1] is not None
    node.scale = (1, 1)
    node.source_rect = bt.box2i(100, 100, 120, 120)                  # nothing of the tape in it
    assert _pull(node, 1, RASTER)[1] is None and _pull32(node, 1, RASTER)[1] is None
    node.source_rect = bt.box2i(*RASTER)
    assert _pull(node, 1, RASTER)[1] is not None
    node.set_source(None)
    cvs.cvs_clear_last_error()
    assert _pull(node, 1, RASTER)[1] is None and _pull32(node, 1, RASTER)[1] is None
    assert "cvs_transform" in _lib.last_error()


def test_node_over_a_solid_source(cvs, process, bt):
    """A source that is not half-native: the f16 pull is the f32 render truncated.  The layer's edge keeps the colour."""
    color, box, full = (0.1, 0.6, 0.15, 0.875), (5, 4, 40, 30), (0, 0, 63, 47)
    rect = (8, 6, 36, 26)
    solid = np.broadcast_to(np.array(color, np.float32), _box(box) + (4,)).copy()
    for fname, filt in FILTERS:
        node = process.VideoTransformFilter(process.SolidColorVideoSource(color, bt.box2i(*box)), bt.box2i(*rect), (22, 16), (1.25, 1.25), 30.0, (30, 22), fname)
        m = node.inverse_at(0)
        want32, win = _node_model(solid, box, rect, m, filt, full)
        got32, w32 = _pull32(node, 0, full)
        got16, w16 = _pull(node, 0, full)
        assert w32 == win and w16 == win and win is not None
        _same(_canvas(got32, full, w32), want32, False, "solid f32 " + fname)
        _same(_canvas(got16, full, w16), f2h_rz_model(want32), True, "solid f16 " + fname)
        alpha = want32[..., 3]
        rim = (alpha > 0) & (alpha < np.float32(0.875))
        assert (rim.any() if filt else not rim.any())
        # along the rim alpha falls off and the colour stays within rounding of the layer's (2 ulp: the constant-frame bound)
        for ch in range(3):
            off = np.abs(want32[..., ch][alpha > 0].astype(np.float64) - float(np.float32(color[ch]))) / float(np.spacing(np.float32(color[ch])))
            assert off.max() <= 4, (ch, off.max())


@pytest.mark.parametrize("flavour,mode", FLAVOURS)
def test_rotated_layer_over_a_solid_in_a_workspace(cvs, process, bt, flavour, mode):
    """The workspace pulls the node as f32 and blends it over the solid at mix 1.0: the model's layer, then the oracle's over."""
    with _in_flavour(cvs, flavour, mode):
        tape = Tape()
        full = RASTER
        ground = (0.9, 0.1, 0.3, 0.75)
        node = process.VideoTransformFilter(tape, bt.box2i(*RASTER), (23, 13), (0.5, 0.5), 30.0, (22, 17))
        ws = process.VideoWorkspace()
        ws.add(source=process.SolidColorVideoSource(ground, bt.box2i(*full)), x=0, length=10, z=0, offset=0)
        ws.add(source=node, x=0, length=10, z=1, offset=0)
        lower = np.broadcast_to(np.array(ground, np.float32), _box(full) + (4,)).copy()
        upper, win = _node_model(tm.widen(tape.picture(3)), RASTER, RASTER, node.inverse_at(3), tm.BILINEAR, full)
        assert win is not None and win != full and ((upper[..., 3] > 0) & (upper[..., 3] < 1)).any()
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
