"""The corner pin on the GPU, bit for bit against the numpy model (tests/perspective_model.py; DESIGN.md "Corner pin"), every entry
case under both cvs_set_arithmetic settings with identical codes required, for f16 and f32 frames and both filters.  Every
operation of the contract is a correctly rounded IEEE f32 operation, a comparison or an exact conversion, so there is no tolerance
anywhere: one differing code fails.  What is folded before comparing (tests/util.py canon_f16 / canon_f32) is the sign of zero.
Target pixels outside the window must keep a sentinel, inputs must come back unwritten.  The tile is 32 x 8, so widths 31, 33 and
65 and heights 7 and 9 sit either side of one and two tiles; one window is taller than a launch's grid."""
import ctypes as C

import numpy as np
import pytest

from canvas_amd import _lib
from canvas_amd.abi import HostFrame
from canvas_amd.device import DeviceFrame
from tests import perspective_model as pm
from tests import transform_model as tm
from tests.models import f2h_rz_model
from tests.test_key_gpu import FLAVOURS, SENTINEL16, SENTINEL32, _box, _same
from tests.test_unsharp_gpu import _in_flavour

pytestmark = pytest.mark.gpu

FILTERS = [("nearest", pm.NEAREST), ("bilinear", pm.BILINEAR)]
F32 = np.float32


def _pixels(rng, full, half):
    """Finite RGBA over `full` in the format asked for: colours in [-0.25, 1.25], alphas in (0, 1], a third of the pixels with
    alpha 0 (their colours kept)."""
    h, w = _box(full)
    s = rng.uniform(-0.25, 1.25, (h, w, 4)).astype(F32)
    s[..., 3] = rng.uniform(0.05, 1.0, (h, w)).astype(F32)
    s[..., 3][rng.uniform(size=(h, w)) < 1.0 / 3.0] = 0
    return f2h_rz_model(s) if half else s


def _entry(cvs, half):
    return cvs.cvs_perspective_f16_dev if half else cvs.cvs_perspective_f32_dev


def _once(cvs, half, tfull, sfull, scur, pixels, p, filt, entry=None, params=None):
    """One call on fresh device frames -> (target buffer, window or None)."""
    dtype, sentinel = (np.uint16, SENTINEL16) if half else (np.float32, SENTINEL32)
    before = np.broadcast_to(sentinel, _box(tfull) + (4,)).copy()
    source = DeviceFrame.from_host(HostFrame(sfull, dtype, pixels, (0, 0, -1, -1) if scur is None else scur))
    target = DeviceFrame.from_host(HostFrame(tfull, dtype, before))
    try:
        params = _lib.perspective(*p, filter=filt) if params is None else params
        rc = (entry or _entry(cvs, half))(target.ref(), source.ref(), C.byref(params), None)
        _lib.check(cvs.cvs_stream_sync(None), "sync")
        assert rc == 0, _lib.last_error()
        got = target.download().array
        window = None if target.current_window.is_empty() else target.current_window.tuple()
        assert source.download().array.tobytes() == np.ascontiguousarray(pixels).tobytes(), "the input was written"
    finally:
        source.free(); target.free()
    return got, window


def _expected(half, tfull, sfull, scur, pixels, p, filt):
    before = np.broadcast_to(SENTINEL16 if half else SENTINEL32, _box(tfull) + (4,)).copy()
    return pm.expected(before, tfull, pixels, sfull, scur, p, filt)


def _check(cvs, half, tfull, sfull, scur, pixels, p, filt, what, flavours=FLAVOURS):
    """The call under both arithmetic settings: the model's codes, the model's window, and the same codes from both."""
    want, win = _expected(half, tfull, sfull, scur, pixels, p, filt)
    results = []
    for flavour, mode in flavours:
        with _in_flavour(cvs, flavour, mode):
            got, window = _once(cvs, half, tfull, sfull, scur, pixels, p, filt)
        label = "%s %s %s %s" % (what, "f16" if half else "f32", "bilinear" if filt else "nearest", flavour)
        assert window == win, "%s: window %r, want %r" % (label, window, win)
        _same(got, want, half, label)
        results.append(got)
    assert results[0].tobytes() == results[-1].tobytes(), what + ": the two arithmetic settings give different codes"
    return results[0], win


def _move(b, d):
    return (b[0] + d[0], b[1] + d[1], b[2] + d[0], b[3] + d[1])


def _quads(S, tfull):
    """(name, quad): where the outer corners of S land in a target of tfull's size at tfull's place"""
    rect = pm.outer(S)
    corners = pm.rect_quad(rect)
    x0, y0 = tfull[0] - 0.5, tfull[1] - 0.5
    w, h = float(tfull[2] - tfull[0] + 1), float(tfull[3] - tfull[1] + 1)
    sw, sh = rect[2] - rect[0], rect[3] - rect[1]
    quarter = [(x0 + 2 + sh, y0 + 1), (x0 + 2 + sh, y0 + 1 + sw), (x0 + 2, y0 + 1 + sw), (x0 + 2, y0 + 1)]     # TL, TR, BR, BL turned by 90 degrees
    keystone = [(x0 + 0.2 * w, y0 + 1), (x0 + 0.8 * w, y0 + 1), (x0 + w, y0 + h - 1), (x0, y0 + h - 1)]          # top edge 0.6 of the bottom
    general = [(x0 + 0.11 * w, y0 + 0.3), (x0 + 0.93 * w, y0 + 1.4), (x0 + 0.78 * w, y0 + h - 0.8), (x0 + 0.02 * w + 1.0, y0 + h - 2.1)]
    return [("identity", corners), ("shift", [(x + 2, y - 1) for x, y in corners]), ("mirror", [corners[k] for k in (1, 0, 3, 2)]), ("90", quarter),
            ("half-pixel shift", [(x + 0.5, y + 0.5) for x, y in corners]), ("keystone", keystone), ("general", general),
            ("general mirrored", [general[k] for k in (1, 0, 3, 2)])]


@pytest.mark.parametrize("tw", [31, 33, 65])
@pytest.mark.parametrize("where", [(0, 0), (-101, -57)], ids=["origin", "odd-negative"])
def test_sizes_quads_formats_and_filters(cvs, tw, where):
    """Targets of 31, 33 and 65 columns x 7 and 9 rows, a source smaller than the target, at the origin and with every frame --
    and so both origins of the map -- moved to odd negative coordinates."""
    rng = np.random.default_rng(tw)
    odd = 0
    for th in (7, 9):
        tfull = _move((0, 0, tw - 1, th - 1), where)
        sfull = _move((3, 1, tw - 6, th - 2), where)
        frames = {True: _pixels(rng, sfull, True), False: _pixels(rng, sfull, False)}
        for name, quad in _quads(sfull, tfull):
            p = pm.from_quad(pm.outer(sfull), quad)
            assert p is not None, name
            if where != (0, 0):
                assert max(p[1] + p[2]) < 0
                odd += sum(v & 1 for v in p[1] + p[2])
            for fname, filt in FILTERS:
                for half in (True, False):
                    got, win = _check(cvs, half, tfull, sfull, sfull, frames[half], p, filt, "%dx%d %s" % (tw, th, name))
                    assert win is not None
    assert where == (0, 0) or odd > 8


@pytest.mark.parametrize("fname,filt", FILTERS)
def test_exact_maps_are_permutations(cvs, fname, filt):
    """Identity, an integer shift, a mirror and a quarter turn come out of from_quad as exact coefficients and move codes:
    asserted against numpy's own slices and rot90, not only against the model."""
    rng = np.random.default_rng(90 + filt)
    for w, h in ((33, 9), (65, 7), (1, 1)):
        S = (0, 0, w - 1, h - 1)
        turned = (0, 0, h - 1, w - 1)
        c = pm.rect_quad(pm.outer(S))
        quarter = [(h - 0.5, -0.5), (h - 0.5, w - 0.5), (-0.5, w - 0.5), (-0.5, -0.5)]
        for half in (True, False):
            s = _pixels(rng, S, half)
            bits = (lambda a: a) if half else (lambda a: np.ascontiguousarray(a).view(np.uint32))
            for name, tfull, quad, want in (("identity", S, c, s), ("shift", (5, -3, w + 4, h - 4), [(x + 5, y - 3) for x, y in c], s),
                                            ("mirror x", S, [c[k] for k in (1, 0, 3, 2)], s[:, ::-1]), ("mirror y", S, [c[k] for k in (3, 2, 1, 0)], s[::-1]),
                                            ("90", turned, quarter, np.rot90(s, -1))):
                p = pm.from_quad(pm.outer(S), quad)
                assert p[0][6:] == (0.0, 0.0, 1.0)
                got, win = _check(cvs, half, tfull, S, S, s, p, filt, "%dx%d %s" % (w, h, name))
                assert win == tfull
                assert np.array_equal(bits(got), bits(np.ascontiguousarray(want))), (w, h, name, half)


def test_source_windows_inside_their_buffers(cvs):
    """S a strict sub-window of a buffer with an odd base column, down to 1 x 1 and 2 x 1: taps outside S are dropped although the
    buffer holds pixels there (colour 1000 and alpha 1 here, so that a tap taken from them would show)."""
    rng = np.random.default_rng(41)
    sfull = (-91, -41, -12, 8)
    tfull = (-95, -45, -5, 14)
    for scur in ((-71, -33, -20, 2), (-50, -10, -50, -10), (-89, -39, -88, -39)):
        for half in (True, False):
            pixels = _pixels(rng, sfull, half)
            poison = f2h_rz_model(np.array([1000, 1000, 1000, 1], F32)) if half else np.array([1000, 1000, 1000, 1], F32)
            keep = pm.crop(pixels, sfull, scur).copy()
            pixels[...] = poison
            pm.crop(pixels, sfull, scur)[...] = keep
            rect = pm.outer(scur)
            cx, cy, w, h = (rect[0] + rect[2]) / 2, (rect[1] + rect[3]) / 2, rect[2] - rect[0], rect[3] - rect[1]
            grown = [(cx - 0.9 * w - 3, cy - 0.6 * h - 2), (cx + 0.7 * w + 2, cy - 0.8 * h - 3), (cx + 1.1 * w + 4, cy + 0.9 * h + 3), (cx - 0.6 * w - 2, cy + 0.7 * h + 2)]
            for name, quad in (("identity", pm.rect_quad(rect)), ("half-pixel shift", [(x + 0.5, y + 0.25) for x, y in pm.rect_quad(rect)]), ("general", grown)):
                p = pm.from_quad(rect, quad)
                for fname, filt in FILTERS:
                    got, win = _check(cvs, half, tfull, sfull, scur, pixels, p, filt, "S %r %s" % (scur, name))
                    assert win is not None
                    written = pm.crop(got, tfull, win)
                    assert not ((pm.widen(written) if half else written)[..., :3] > 100).any(), "a tap was taken outside S"
            # no source window at all, and a target the picture misses
            got, win = _check(cvs, half, tfull, sfull, None, pixels, p, pm.BILINEAR, "empty source")
            assert win is None and (got == (SENTINEL16 if half else SENTINEL32)).all()
            got, win = _check(cvs, half, (200, 0, 260, 36), sfull, scur, pixels, p, pm.BILINEAR, "disjoint")
            assert win is None and (got == (SENTINEL16 if half else SENTINEL32)).all()


def test_affine_coefficients_with_zero_origins_give_the_transforms_bytes(cvs):
    """h6 = h7 = 0, h8 = 1 and both origins (0, 0): w is exactly 1, u = nu, and the entry is cvs_transform byte for byte, window
    included, on the same frames."""
    rng = np.random.default_rng(43)
    for tfull, S in (((0, 0, 64, 36), (0, 0, 64, 36)), ((-20, -9, 44, 8), (3, 1, 33, 7))):
        cx, cy = (S[0] + S[2]) / 2.0, (S[1] + S[3]) / 2.0
        for parts in ({}, dict(position=(0.5, 0.25)), dict(anchor=(cx, cy), position=(cx, cy), rotation=30), dict(anchor=(cx, cy), position=(cx + 3, cy - 2), rotation=-17.5, scale=(1.5, -0.75)),
                      dict(anchor=(cx, cy), position=(cx, cy), scale=(0.5, 0.5))):
            m = tm.from_parts(**parts)
            for half in (True, False):
                pixels = _pixels(rng, S, half)
                for fname, filt in FILTERS:
                    p = (m + (0.0, 0.0, 1.0), (0, 0), (0, 0))
                    got, win = _check(cvs, half, tfull, S, S, pixels, p, filt, "affine %r" % (parts,))
                    other, owin = _once(cvs, half, tfull, S, S, pixels, None, filt, entry=cvs.cvs_transform_f16_dev if half else cvs.cvs_transform_f32_dev,
                                        params=_lib.transform(m, filt))
                    assert win == owin and got.tobytes() == other.tobytes(), (parts, half, fname)


def test_nothing_is_drawn_on_or_beyond_the_vanishing_line(cvs):
    """h = (1,0,0, 0,1,0, 0.1,0,1): w = 1 + 0.1 x is 0 at x = -10 and negative beyond, where u = x / w is positive again -- without
    the w > 0 rule (-30, -4) would sample (15, 2) and the layer appear a second time."""
    h = tuple(float(F32(v)) for v in (1, 0, 0, 0, 1, 0, 0.1, 0, 1))
    p = (h, (0, 0), (0, 0))
    S, tfull = (0, 0, 63, 15), (-40, -20, 40, 20)
    w = F32(h[6]) * F32(-30) + F32(1)
    assert w < 0 and round(float(F32(-30) / w)) == 15 and round(float(F32(-4) / w)) == 2
    rng = np.random.default_rng(5)
    for half in (True, False):
        pixels = _pixels(rng, S, half)
        pixels[..., 3] = f2h_rz_model(np.ones(_box(S), F32)) if half else 1            # opaque: a ghost would show
        for fname, filt in FILTERS:
            got, win = _check(cvs, half, tfull, S, S, pixels, p, filt, "vanishing line")
            assert win == tfull
            assert not got[:, :31].any()                                                # every pixel with X <= -10
            assert got[20:24, 41:].any()                                                # the layer itself, at x >= 0


def test_a_layers_edge_keeps_its_colour_and_transparent_taps_give_zero(cvs):
    """A constant layer under a general quad: along the rim alpha falls off and the colour stays within rounding of the layer's;
    where all four taps have alpha 0 the pixel is exactly 0, whatever colour the transparent pixels carry."""
    S, tfull = (0, 0, 39, 23), (-4, -4, 60, 40)
    quad = [(2.0, 1.5), (52.0, 6.0), (47.5, 35.0), (5.5, 28.0)]
    p = pm.from_quad(pm.outer(S), quad)
    color = (0.1, 0.6, 0.15, 0.875)
    rng = np.random.default_rng(47)
    for half in (True, False):
        solid = np.broadcast_to(np.array(color, F32), _box(S) + (4,)).copy()
        solid = f2h_rz_model(solid) if half else solid
        got, win = _check(cvs, half, tfull, S, S, solid, p, pm.BILINEAR, "constant layer")
        wide = pm.widen(pm.crop(got, tfull, win)) if half else pm.crop(got, tfull, win)
        alpha = wide[..., 3]
        layer = float(pm.widen(solid)[0, 0, 3] if half else solid[0, 0, 3])
        assert ((alpha > 0) & (alpha < layer)).any() and (alpha == F32(layer)).any()
        for ch in range(3):
            c = float(pm.widen(solid)[0, 0, ch] if half else solid[0, 0, ch])
            unit = float(np.spacing(F32(c))) * (2 ** 13 if half else 1)                  # a half's spacing: the store truncates
            off = np.abs(wide[..., ch][alpha > 0].astype(np.float64) - c) / unit
            assert off.max() <= 4, (half, ch, off.max())
        holes = _pixels(rng, S, half)
        holes[6:18, 10:30, 3] = 0
        got, win = _check(cvs, half, tfull, S, S, holes, p, pm.BILINEAR, "hole")
        u, v, w = pm.source_coords(p, win)
        i, j = np.floor(u) + p[2][0], np.floor(v) + p[2][1]
        deep = (i >= 10) & (i + 1 <= 29) & (j >= 6) & (j + 1 <= 17) & (w > 0)
        assert deep.sum() > 100 and not pm.crop(got, tfull, win)[deep].any()


def test_a_window_taller_than_one_launch(cvs):
    """8 columns x (65 535 * 8 + 9) rows of half pixels: the rows of tiles beyond a grid's 65 535 go out as a second launch."""
    rows = 65535 * 8 + 9
    tfull, S = (0, 0, 7, rows - 1), (0, 0, 5, 40)
    quad = [(0.5, -0.5), (7.0, 100.5), (7.5, rows - 200.25), (-0.5, rows - 0.5)]
    p = pm.from_quad(pm.outer(S), quad)
    assert p is not None and (p[0][6] != 0 or p[0][7] != 0)
    pixels = _pixels(np.random.default_rng(9), S, True)
    got, win = _check(cvs, True, tfull, S, S, pixels, p, pm.BILINEAR, "tall", flavours=FLAVOURS[:1])
    assert win == tfull
    assert got[-1].any() or got[-40:].any()                                              # the last band was written
