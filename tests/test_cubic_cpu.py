"""The Catmull-Rom filter of the two warps without a GPU (DESIGN.md "Catmull-Rom warps"): the numpy model
(tests/cubic_model.py) against the properties the contract promises -- exact weights, the clamp rule, exact permutations, sources
narrower than the support; the margins of the four windows against the f32 pixel rule by brute force; the host functions against
the model through the library; the header, the built code object, the catalogue of tests/cubic_cases.py and the nodes' surface."""
import ctypes as C
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from tests import cubic_model as cm
from tests import perspective_model as pm
from tests import transform_model as tm
from tests.models import f2h_rz_model
from tests.test_perspective_cpu import BOX, FAR, QUADS, RECT, _draw, _from_quad, _moved, _triple
from tests.test_perspective_cpu import _windows as _pin_windows
from tests.test_transform_cpu import EVERYWHERE, IDENTITY, _bits, _source_window, _target_window, _transforms
from tests.test_unsharp_cpu import _kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
CUBIC = cm.CATMULL_ROM


@pytest.fixture(scope="module")
def lib():
    from canvas_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def process():
    from fluggo.media import process
    return process


def _pictures(rng, h, w, wild=False):
    """(f32 pixels, half codes) with alpha in [0, 1]; wild: colours of either sign up to 1e4"""
    f32 = rng.uniform(-1e4, 1e4, (h, w, 4)).astype(F32) if wild else rng.uniform(-0.25, 1.25, (h, w, 4)).astype(F32)
    f32[..., 3] = rng.uniform(0.0, 1.0, (h, w)).astype(F32)
    return f32, f2h_rz_model(f32 if not wild else np.clip(f32, -6e4, 6e4))


M30 = lambda S: tm.from_parts(anchor=((S[0] + S[2]) / 2.0, (S[1] + S[3]) / 2.0), position=((S[0] + S[2]) / 2.0 + 0.25, (S[1] + S[3]) / 2.0), rotation=30.0)  # noqa: E731


def _keystone(S, tw, th):
    return pm.from_quad(pm.outer(S), [(0.2 * tw - 0.5, 0.5), (0.8 * tw - 0.5, 0.5), (tw - 0.5, th - 1.5), (-0.5, th - 1.5)])


# ---------------------------------------------------------------- the model: weights and the clamp rule

def test_the_constant_is_the_support_and_is_mirrored():
    from canvas_amd import _lib
    assert _lib.TRANSFORM_CATMULL_ROM == 4 == CUBIC and (_lib.TRANSFORM_NEAREST, _lib.TRANSFORM_BILINEAR) == (0, 1)


def test_exact_weights():
    """t = 0 gives exactly (-+0, 1, 0, -+0), t = 1/2 exactly (-1/16, 9/16, 9/16, -1/16); everywhere the four sum to 1 within the
    rounding of nine operations (each weight is at most 1 in magnitude: 16 * 2^-24)."""
    w = [float(v) for v in cm.weights(F32(0.0))]
    assert w == [0.0, 1.0, 0.0, 0.0] and all(isinstance(v, float) for v in w)
    w = [float(v) for v in cm.weights(F32(0.5))]
    assert w == [-0.0625, 0.5625, 0.5625, -0.0625]
    t = np.linspace(0, 1, 4097, dtype=F32)[:-1]
    total = sum(v.astype(np.float64) for v in cm.weights(t))
    assert np.abs(total - 1.0).max() <= 16 * 2.0 ** -24
    w0, w1, w2, w3 = cm.weights(t)
    assert (w0 <= 0).all() and (w3 <= 0).all() and (w1 >= 0).all() and (w2 >= 0).all() and w0.min() >= -0.075 and w1.max() <= 1.0


def _samples(seed, wild=False):
    """(what, source, S, u, v, front) over seeded pictures: 30 degrees and a keystone, f32 and half"""
    rng = np.random.default_rng(seed)
    S = (3, 1, 27, 17)
    f32, codes = _pictures(rng, 17, 25, wild)
    tfull = (0, 0, 32, 19)
    out = []
    for source in (f32, codes):
        u, v = tm.source_coords(M30(S), tfull)
        out.append(("30 degrees", source, S, u, v, np.ones(u.shape, bool)))
        p = _keystone(S, 33, 20)
        so = p[2]
        u, v, w = pm.source_coords(p, tfull)
        out.append(("keystone", source, (S[0] - so[0], S[1] - so[1], S[2] - so[0], S[3] - so[1]), u, v, w > 0))
    return out


def _within_limits(out, limits, what):
    wide = tm.widen(out) if out.dtype == np.uint16 else out
    blended = limits["blended"]
    assert blended.sum() > 100, what
    lo, hi = limits["lo"], limits["hi"]
    # (a half result is truncated towards zero between limits that are halfs themselves, or 0: it stays inside them)
    for ch in range(4):
        assert (wide[..., ch][blended] >= lo[..., ch][blended]).all() and (wide[..., ch][blended] <= hi[..., ch][blended]).all(), (what, ch)
    # and the limits are those of the sixteen taps, never the initial infinities
    assert np.isfinite(lo[blended]).all() and np.isfinite(hi[blended]).all(), what


def test_every_channel_stays_within_the_limits_of_its_taps():
    for what, source, S, u, v, front in _samples(2701):
        limits = {}
        out = cm.sample(source, S, u, v, limits=limits)
        _within_limits(out, limits, what)
        wide = tm.widen(out) if out.dtype == np.uint16 else out
        assert (wide[..., 3] >= 0).all() and (wide[..., 3] <= 1).all(), what
        # the clamp does bite on such pictures: without it the cubic overshoots
        assert ((wide == limits["lo"]) | (wide == limits["hi"]))[limits["blended"]].any(), what


def test_a_one_pixel_alpha_checker_with_wild_colours_stays_in_the_sources_range():
    """Alpha alternates 0 / 1 from pixel to pixel: under mixed-sign weights A nearly cancels, and R / A would be anything."""
    for what, source, S, u, v, front in _samples(2702, wild=True):
        source = source.copy()
        yy, xx = np.mgrid[0:source.shape[0], 0:source.shape[1]]
        one = np.uint16(0x3C00) if source.dtype == np.uint16 else F32(1)
        source[..., 3] = np.where((xx + yy) & 1, one, 0)
        limits = {}
        out = cm.sample(source, S, u, v, limits=limits)
        _within_limits(out, limits, what)
        wide, swide = (tm.widen(out), tm.widen(source)) if out.dtype == np.uint16 else (out, source)
        assert np.isfinite(wide).all()
        solid = swide[..., 3] > 0
        for ch in range(3):
            drawn = wide[..., 3] > 0
            assert wide[..., ch][drawn].min() >= swide[..., ch][solid].min() and wide[..., ch][drawn].max() <= swide[..., ch][solid].max(), (what, ch)
        assert wide[..., 3].min() >= 0 and wide[..., 3].max() <= 1


def test_an_opaque_flat_layer_stays_exactly_flat_and_opaque():
    color = np.array([0.1, 0.6, 0.15, 1.0], F32)
    for what, source, S, u, v, front in _samples(2703):
        flat = np.broadcast_to(f2h_rz_model(color) if source.dtype == np.uint16 else color, source.shape).copy()
        out = cm.sample(flat, S, u, v)
        interior = front.copy()
        for ti, tj in cm.taps(u, v):
            interior &= tm.inside(ti, tj, S)
        assert interior.sum() > 100, what
        assert (out[interior] == flat[0, 0]).all(), what
        # at the rim alpha falls off and never exceeds the layer's own
        alpha = (tm.widen(out) if out.dtype == np.uint16 else out)[..., 3]
        assert alpha.max() == 1 and alpha.min() == 0 and ((alpha > 0) & (alpha < 1)).any()


def test_model_exact_maps_are_permutations_of_the_codes():
    """Identity, integer shifts, the mirrors and the right-angle rotations move the source's codes, NaN payloads and zero signs
    included, in both formats; so does the corner pin of the same maps."""
    h, w = 5, 7
    S = (0, 0, w - 1, h - 1)
    rng = np.random.default_rng(9)
    f32, _ = _pictures(rng, h, w)
    f32[0, 0] = [np.nan, -0.0, 1e-40, 0.5]
    f32[2, 3] = [0.25, -0.0, 0.0, 0.0]
    f32.view(np.uint32)[1, 1, 0] = 0x7FA00001                        # a signalling NaN with a payload
    codes = rng.integers(0, 0x3C01, (h, w, 4), dtype=np.uint16)
    codes[0, 0] = [0x7C01, 0x8000, 0x0001, 0x3555]
    turned = (0, 0, h - 1, w - 1)
    for s in (f32, codes):
        for name, tfull, parts, want in (
                ("identity", S, {}, s), ("shift", (5, -3, w + 4, h - 4), dict(position=(5, -3)), s),
                ("mirror x", S, dict(scale=(-1, 1), position=(w - 1, 0)), s[:, ::-1]), ("mirror y", S, dict(scale=(1, -1), position=(0, h - 1)), s[::-1]),
                ("90", turned, dict(rotation=90, position=(h - 1, 0)), np.rot90(s, -1)), ("180", S, dict(rotation=180, position=(w - 1, h - 1)), np.rot90(s, 2)),
                ("270", turned, dict(rotation=270, position=(0, w - 1)), np.rot90(s, 1))):
            m = tm.from_parts(**parts)
            assert cm.transform_target_window(m, S, (-50, -50, 50, 50)) == (tfull[0] - 3, tfull[1] - 3, tfull[2] + 3, tfull[3] + 3), name
            got = cm.transform_plane(s, S, m, tfull)
            assert np.array_equal(_bits(got), _bits(np.ascontiguousarray(want))), name
            ring = cm.transform_plane(s, S, m, (tfull[0] - 3, tfull[1] - 3, tfull[2] + 3, tfull[3] + 3))
            assert not ring[:3].any() and not ring[-3:].any() and not ring[:, :3].any() and not ring[:, -3:].any(), name
    for name, quad in QUADS[:8]:
        p = pm.from_quad(RECT, quad)
        bh, bw = BOX[3] - BOX[1] + 1, BOX[2] - BOX[0] + 1
        s = rng.integers(0, 0x3C01, (bh, bw, 4), dtype=np.uint16)
        s[0, 0] = [0x7C01, 0x8000, 0x0001, 0x3555]
        win = cm.perspective_target_window(p, BOX, (-100, -100, 100, 100))
        got = cm.perspective_plane(s, BOX, p, win)
        assert sorted(map(tuple, got.reshape(-1, 4)[got.reshape(-1, 4).any(axis=1)].tolist())) == sorted(map(tuple, s.reshape(-1, 4)[s.reshape(-1, 4).any(axis=1)].tolist())), name
        assert np.array_equal(got, pm.perspective_plane(s, BOX, p, pm.NEAREST, win)), name


@pytest.mark.parametrize("sw,sh", [(1, 1), (1, 5), (5, 1), (2, 2), (3, 3)])
def test_sources_narrower_than_the_support(sw, sh):
    """Every tap row or column clamps: the result is the same as that of the source padded with transparent pixels carrying wild
    colours (a tap outside S counts for nothing), lies within the source's range, and an identity still copies."""
    rng = np.random.default_rng(sw * 10 + sh)
    S = (4, 2, 4 + sw - 1, 2 + sh - 1)
    f32, codes = _pictures(rng, sh, sw)
    f32[..., 3] = np.maximum(f32[..., 3], F32(0.25))
    tfull = (0, 0, 12, 9)
    for source in (f32, codes):
        for m in (tm.from_parts(position=(0.5, 0.25)), M30(S), tm.from_parts(anchor=(4, 2), position=(4.125, 2.5), scale=(2, 2))):
            limits = {}
            out = cm.transform_plane(source, S, m, tfull, limits=limits)
            assert limits["blended"].any()
            _check = tm.widen(out) if out.dtype == np.uint16 else out
            swide = tm.widen(source) if source.dtype == np.uint16 else source
            drawn = _check[..., 3] > 0
            for ch in range(3):
                assert _check[..., ch][drawn].min() >= swide[..., ch].min() and _check[..., ch][drawn].max() <= swide[..., ch].max()
            big = (S[0] - 3, S[1] - 3, S[2] + 3, S[3] + 3)
            padded = np.full((sh + 6, sw + 6, 4), 777.0, F32)
            padded[..., 3] = 0
            if source.dtype == np.uint16:
                padded = f2h_rz_model(padded)
            padded[3:-3, 3:-3] = source
            assert np.array_equal(_bits(cm.transform_plane(padded, big, m, tfull)), _bits(out))
        assert np.array_equal(_bits(cm.transform_plane(source, S, IDENTITY, S)), _bits(source))


# ---------------------------------------------------------------- the windows by brute force

def _tapped(u, v, S):
    taps = cm.taps(u, v)
    hit = np.zeros(u.shape, bool)
    for ti, tj in taps:
        hit |= tm.inside(ti, tj, S)
    return hit, taps


def test_affine_windows_are_safe_by_brute_force():
    """1000 seeded transforms with coordinates within +-2^14 (the generator of tests/test_transform_cpu.py): no target pixel
    outside the target window has a tap inside S (looked for in a ring of 6 pixels around it), and no tap of a target window lies
    outside the source window.  The smallest slack found is in DESIGN.md."""
    slack_t, slack_s, sampled = 10 ** 9, 10 ** 9, 0
    for S, parts, m in _transforms(14, 1000, 1 << 14):
        # a target window about where the layer lands, some of it off the layer
        px, py = int(parts["position"][0]), int(parts["position"][1])
        window = (px - 5, py - 9, px + 8, py + 3)
        need = cm.transform_source_window(m, window)
        _, taps = _tapped(*tm.source_coords(m, window), EVERYWHERE)
        for ti, tj in taps:
            assert need[0] <= ti.min() and ti.max() <= need[2] and need[1] <= tj.min() and tj.max() <= need[3], (parts, window, need)
            slack_s = min(slack_s, int(min(ti.min() - need[0], need[2] - ti.max(), tj.min() - need[1], need[3] - tj.max())))
        win = cm.transform_target_window(m, S, EVERYWHERE)
        assert win is not None
        ring = (win[0] - 6, win[1] - 6, win[2] + 6, win[3] + 6)
        assert (ring[2] - ring[0]) * (ring[3] - ring[1]) < 1 << 18, (S, parts, win)
        hit, _ = _tapped(*tm.source_coords(m, ring), S)
        ys, xs = np.nonzero(hit)
        if not len(xs):                                              # a layer shrunk to less than a pixel can miss every sample
            continue
        sampled += 1
        x0, x1, y0, y1 = ring[0] + xs.min(), ring[0] + xs.max(), ring[1] + ys.min(), ring[1] + ys.max()
        assert win[0] <= x0 and x1 <= win[2] and win[1] <= y0 and y1 <= win[3], (S, parts, win, (x0, y0, x1, y1))
        slack_t = min(slack_t, int(min(x0 - win[0], win[2] - x1, y0 - win[1], win[3] - y1)))
    print("smallest slack: target window %d, source window %d; %d of 1000 maps meet a sample" % (slack_t, slack_s, sampled))
    assert slack_t >= 0 and slack_s >= 0 and sampled > 900


def test_corner_pin_windows_are_safe_by_brute_force(lib):
    """The 600 quads of tests/test_perspective_cpu.py's generator, none skipped, as its own brute-force test walks them: no pixel
    with a tap in S lies outside the target window; no tap of a 64 x 64 tile that lies in the source rectangle lies outside the
    source window.  The windows walked are the library's, each the model's on every draw."""
    rng = np.random.default_rng(20261019)
    slack_t, slack_s, folded_t, folded_s, sampled = 10 ** 9, 10 ** 9, 0, 0, 0
    huge = (-2000, -2000, 2000, 2000)
    for n in range(600):
        box, S, quad = _draw(rng)
        p = pm.from_quad(pm.outer(box), quad)
        assert p is not None, (n, quad)
        _h, to, so = p
        rc, made = _from_quad(lib, pm.outer(box), quad, CUBIC)
        assert rc == 0 and _triple(made) == p and made.filter == CUBIC, (n, _triple(made), p)
        win = cm.perspective_target_window(p, S, huge)
        if win == huge:
            folded_t += 1
        else:
            region = (win[0] - 8, win[1] - 8, win[2] + 8, win[3] + 8)
            u, v, w = pm.source_coords(p, region)
            rel = (S[0] - so[0], S[1] - so[1], S[2] - so[0], S[3] - so[1])
            hit, _ = _tapped(u, v, rel)
            hit &= w > 0
            if hit.any():
                sampled += 1
                ys, xs = np.nonzero(hit)
                xs, ys = xs + region[0], ys + region[1]
                slack_t = min(slack_t, xs.min() - win[0], win[2] - xs.max(), ys.min() - win[1], win[3] - ys.max())
        tx, ty = int(math.floor(quad[0][0])) - int(rng.integers(0, 64)), int(math.floor(quad[0][1])) - int(rng.integers(0, 64))
        tile = (tx, ty, tx + 63, ty + 63)
        need = cm.perspective_source_window(p, tile)
        assert _pin_windows(lib, p, CUBIC, S, huge, tile) == (win, need), (n, win, need)
        if need == pm.WHOLE:
            folded_s += 1
        else:
            u, v, w = pm.source_coords(p, tile)
            assert (w > 0).all()
            rel = (box[0] - so[0], box[1] - so[1], box[2] - so[0], box[3] - so[1])
            for i, j in cm.taps(u, v):
                ok = tm.inside(i, j, rel)
                if ok.any():
                    ii, jj = i[ok].astype(np.int64) + so[0], j[ok].astype(np.int64) + so[1]
                    slack_s = min(slack_s, ii.min() - need[0], need[2] - ii.max(), jj.min() - need[1], need[3] - jj.max())
    print("smallest slack: target window %d, source window %d; windows on the vanishing line: %d target, %d source" % (slack_t, slack_s, folded_t, folded_s))
    assert slack_t >= 0 and slack_s >= 0
    assert folded_t < 300 and folded_s < 300 and sampled > 300


# ---------------------------------------------------------------- the host functions against the model

def test_affine_window_functions_are_the_models(lib):
    for S, parts, m in _transforms(31, 200, 4096):
        window = (int(parts["position"][0]) - 4, int(parts["position"][1]) - 2, int(parts["position"][0]) + 9, int(parts["position"][1]) + 5)
        for tfull in (EVERYWHERE, (S[0] - 7, S[1] - 40, S[0] + 30, S[1] + 3), (-4096, -4096, 4096, 4096)):
            assert _target_window(lib, m, CUBIC, S, tfull) == (0, cm.transform_target_window(m, S, tfull)), (S, parts, tfull)
            # the two filters there were: not a bit has moved
            for filt in (tm.NEAREST, tm.BILINEAR):
                assert _target_window(lib, m, filt, S, tfull) == (0, tm.target_window(m, filt, S, tfull)), (S, parts, filt, tfull)
        assert _source_window(lib, m, CUBIC, window) == (0, cm.transform_source_window(m, window)), (parts, window)
        for filt in (tm.NEAREST, tm.BILINEAR):
            assert _source_window(lib, m, filt, window) == (0, tm.source_window(m, window)), (parts, window)
    one = (5, -3, 5, -3)
    assert _target_window(lib, IDENTITY, CUBIC, one, EVERYWHERE) == (0, (2, -6, 8, 0)) == (0, cm.transform_target_window(IDENTITY, one, EVERYWHERE))
    assert _source_window(lib, IDENTITY, CUBIC, one) == (0, (2, -6, 8, 0)) == (0, cm.transform_source_window(IDENTITY, one))
    assert _source_window(lib, IDENTITY, tm.BILINEAR, one) == (0, (3, -5, 7, -1)) and _source_window(lib, IDENTITY, tm.NEAREST, one) == (0, (3, -5, 7, -1))


@pytest.mark.parametrize("name,quad", QUADS, ids=[q[0] for q in QUADS])
def test_corner_pin_window_functions_are_the_models(lib, name, quad):
    for d in ((0, 0), FAR):
        rect = (RECT[0] + d[0], RECT[1] + d[1], RECT[2] + d[0], RECT[3] + d[1])
        triple = pm.from_quad(rect, _moved(quad, *d))
        rc, made = _from_quad(lib, rect, _moved(quad, *d), CUBIC)
        assert rc == 0 and made.filter == CUBIC and made.flags == 0 and _triple(made) == triple
        mv = lambda b: (b[0] + d[0], b[1] + d[1], b[2] + d[0], b[3] + d[1])
        for S in (BOX, (5, 2, 5, 2), (4, 3, 20, 9)):
            for tfull in ((-60, -60, 90, 90), (0, 0, 20, 10), (200, 200, 220, 220)):
                for window in ((0, 0, 63, 63), (-5, 7, 11, 8)):
                    got = _pin_windows(lib, triple, CUBIC, mv(S), mv(tfull), mv(window))
                    assert got == (cm.perspective_target_window(triple, mv(S), mv(tfull)), cm.perspective_source_window(triple, mv(window))), (name, d, S, tfull, window)
                    for filt in (pm.NEAREST, pm.BILINEAR):
                        got = _pin_windows(lib, triple, filt, mv(S), mv(tfull), mv(window))
                        assert got == (pm.target_window(triple, filt, mv(S), mv(tfull)), pm.source_window(triple, mv(window))), (name, d, filt)


def test_the_other_values_stay_refused_and_the_messages_name_three_filters(lib):
    from canvas_amd import _lib
    box = _lib.box2i.of
    b = box(0, 0, 7, 7)
    for filt in (2, 3, 5, -1, 6, 7):
        for call in (lambda w: lib.cvs_transform_target_window(C.byref(_lib.transform(IDENTITY, filt)), C.byref(b), C.byref(b), C.byref(w)),
                     lambda w: lib.cvs_transform_source_window(C.byref(_lib.transform(IDENTITY, filt)), C.byref(b), C.byref(w)),
                     lambda w: lib.cvs_perspective_target_window(C.byref(_lib.perspective(filter=filt)), C.byref(b), C.byref(b), C.byref(w)),
                     lambda w: lib.cvs_perspective_source_window(C.byref(_lib.perspective(filter=filt)), C.byref(b), C.byref(w))):
            win = box(1, 1, 2, 2)
            lib.cvs_clear_last_error()
            assert call(win) == -1 and win.is_empty(), filt
            msg = _lib.last_error()
            assert "filter" in msg and all(n in msg for n in ("CVS_TRANSFORM_NEAREST", "CVS_TRANSFORM_BILINEAR", "CVS_TRANSFORM_CATMULL_ROM")), msg
        rc, _p = _from_quad(lib, RECT, pm.rect_quad(RECT), filt)
        assert rc == -1 and "filter" in _lib.last_error() and "CVS_TRANSFORM_CATMULL_ROM" in _lib.last_error()
    # the device entries refuse them too, and accept 4 up to the device
    from canvas_amd.abi import HostFrame
    for entry, dtype, params in ((lib.cvs_transform_f16_dev, np.uint16, lambda f: _lib.transform(IDENTITY, f)), (lib.cvs_transform_f32_dev, np.float32, lambda f: _lib.transform(IDENTITY, f)),
                                 (lib.cvs_perspective_f16_dev, np.uint16, lambda f: _lib.perspective(filter=f)), (lib.cvs_perspective_f32_dev, np.float32, lambda f: _lib.perspective(filter=f))):
        full = (0, 0, 7, 7)
        for filt in (2, 3, 5, -1):
            out, src = HostFrame(full, dtype, current_window=full), HostFrame(full, dtype, current_window=full)
            lib.cvs_clear_last_error()
            assert entry(out.ref(), src.ref(), C.byref(params(filt)), None) == -1 and "filter" in _lib.last_error() and out.current_window.is_empty()
        if lib.cvs_device_count() == 0:
            out, src = HostFrame(full, dtype, current_window=full), HostFrame(full, dtype, current_window=full)
            lib.cvs_clear_last_error()
            assert entry(out.ref(), src.ref(), C.byref(params(CUBIC)), None) != 0 and "no CPU path" in _lib.last_error(), _lib.last_error()
            assert out.current_window.is_empty()


# ---------------------------------------------------------------- the header, the code object

def test_the_headers_compile_as_c_and_as_cpp_with_the_constant():
    text = open(os.path.join(ROOT, "include", "canvas_hip.h")).read()
    assert "enum { CVS_TRANSFORM_NEAREST = 0, CVS_TRANSFORM_BILINEAR = 1 };\n" in text and "enum { CVS_TRANSFORM_CATMULL_ROM = 4 };\n" in text
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "t.c")
        with open(src, "w") as f:
            f.write('#include "canvas_perspective.h"\nint main(void) { cvs_perspective p; cvs_transform t; p.filter = CVS_TRANSFORM_CATMULL_ROM; t.filter = CVS_TRANSFORM_CATMULL_ROM; '
                    'return p.filter == 4 && t.filter == 4 && CVS_TRANSFORM_NEAREST == 0 && CVS_TRANSFORM_BILINEAR == 1 ? 0 : 1; }\n')
        for cc, std, lang in (("gcc", "-std=c99", "c"), ("g++", "-std=c++14", "c++")):
            exe = os.path.join(tmp, "t_" + cc)
            subprocess.run([cc, std, "-Wall", "-Werror", "-x", lang, src, "-I", os.path.join(ROOT, "include"), "-o", exe], check=True)
            assert subprocess.run([exe]).returncode == 0


def test_code_object_holds_the_four_instances_without_scratch():
    """One build for both arithmetic flavours; k_transform_cubic / k_perspective_cubic x f32 / f16; no private segment, no spills,
    and no register read between a load into it and the wait that retires it.  Both launchers are exported to the hosts."""
    from canvas_amd import _lib
    assert os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"), "the ROCm LLVM tools the build itself needs are missing"
    found = _kernels("warp_cubic_ops.hip.o")
    assert len(found) == 4, sorted(found)
    for half in (0, 1):
        assert any(re.search(r"k_transform_cubicILi%dEEE" % half, n) for n in found), (half, sorted(found))
        assert any(re.search(r"k_perspective_cubicILi%dEEE" % half, n) for n in found), (half, sorted(found))
    for name, (scratch, spills) in found.items():
        assert scratch == 0 and spills == 0, (name, scratch, spills)
    assert not os.path.exists(os.path.join(ROOT, "canvas_amd", "csrc", "build", "warp_cubic_ops.fma.hip.o"))
    spec = __import__("importlib.util").util.spec_from_file_location("check_asm_loads", os.path.join(ROOT, "tools", "check_asm_loads.py"))
    chk = __import__("importlib.util").util.module_from_spec(spec)
    spec.loader.exec_module(chk)
    checked, problems = chk.check_paths([os.path.join(ROOT, "canvas_amd", "csrc", "build", "warp_cubic_ops.hip.o")])
    assert checked >= 4 and not problems, problems[:5]
    symbols = subprocess.run(["nm", _lib.LIB_PATH], stdout=subprocess.PIPE, text=True).stdout
    for name in ("cvk_transform_cubic", "cvk_perspective_cubic"):
        assert re.search(r"\b%s\b" % name, symbols) and not re.search(r"\b%s_fma\b" % name, symbols), name


# ---------------------------------------------------------------- the catalogue

def test_the_catalogue_calls_the_four_entries_with_the_cubic_filter():
    """What tests/test_perspective_cpu.py holds its catalogue to, for tests/cubic_cases.py: every case makes one call of one of the
    four entries on the factory's stream with filter CVS_TRANSFORM_CATMULL_ROM, asks for the same operands every time, and the
    Shifted factory moves the frames, the coefficients' translation and both origins."""
    from canvas_amd import _lib
    from tests import cubic_cases as cc
    from tests import entry_cases as ec
    from tests.test_entry_cases_cpu import OFFSET, Geometry, HostOnly, Recorder, _check_shifted

    class Params(Recorder):
        def __getattr__(self, name):
            def call(*args):
                p = args[2]._obj
                self.calls.append((name, args[3], p.filter, p.flags, tuple(p.m) if hasattr(p, "m") else (tuple(p.h), tuple(p.target_origin), tuple(p.source_origin))))
                return 0
            return call
    seen, cases = {}, 0
    for gid, build in cc.GROUPS:
        assert cc.warp_of(gid) in cc.FAR_RULE
        near, far = Params(), Params()
        for (what, a), (_, b) in zip(build(near), build(far)):
            cases += 1
            fac = HostOnly(near, 0x5EED)
            assert a(fac) == 0
            name, stream, filt, flags, _geometry = near.calls[-1]
            assert stream == 0x5EED and filt == _lib.TRANSFORM_CATMULL_ROM and flags == 0, (gid, what)
            assert cc.warp_of(gid) in name
            seen.setdefault(name, []).append(what)
            assert any(o.out for o in fac.objects) and all(o.frame is not None for o in fac.objects) and len(fac.objects) == 2, (gid, what)
            again = HostOnly(near, 0x5EED)
            a(again)
            spec = lambda f: [(o.cls, o.name, o.out, o.cmp, o.nbytes, o.row_bytes, o.reads) for o in f.objects]
            assert spec(fac) == spec(again), (gid, what)
            boxes = [(o.out, o.frame.c.full_window.tuple()) for o in fac.objects if o.frame is not None]
            assert len(ec.far_offsets(cc.FAR_RULE[cc.warp_of(gid)], boxes)) >= 4, (gid, what)
            b(ec.Shifted(HostOnly(far, 1), OFFSET))
            n, f = near.calls[-2][4], far.calls[-1][4]
            if cc.warp_of(gid) == "perspective":
                assert f[0] == n[0] and f[1] == (n[1][0] + OFFSET[0], n[1][1] + OFFSET[1]) and f[2] == (n[2][0] + OFFSET[0], n[2][1] + OFFSET[1])
            else:
                # the linear part stays; the translation follows the frames (a pure shift's stays too: source and target move alike)
                assert (f[0], f[1], f[3], f[4]) == (n[0], n[1], n[3], n[4]) and ((f[2], f[5]) != (n[2], n[5])) == ("shift" not in what), (gid, what)
    assert sorted(seen) == sorted(cc.ENTRIES) and cases == 2 * (30 + 18)
    assert len(seen["cvs_transform_f16_dev"]) == len(seen["cvs_transform_f32_dev"]) == 30 and len(seen["cvs_perspective_f16_dev"]) == len(seen["cvs_perspective_f32_dev"]) == 18
    for word in ("half-pixel shift", "30 degrees", "half size", "double size", "mirror"):
        assert any(word in w for w in seen["cvs_transform_f16_dev"]), word
    for word in ("half-pixel shift", "keystone", "general"):
        assert any(word in w for w in seen["cvs_perspective_f32_dev"]), word
    frames = 0
    for gid, build in cc.GROUPS:
        a, b = Geometry(), Geometry()
        for (what, near), (_, far) in zip(build(a), build(b)):
            frames += _check_shifted(gid, what, (near, far, a, b), 1)
    assert frames == 2 * cases


# ---------------------------------------------------------------- the nodes

def test_the_nodes_take_the_name_and_give_it_back(process):
    from fluggo.media import basetypes as bt
    red = process.SolidColorVideoSource((1, 0, 0, 1))
    rect = bt.box2i(0, 0, 31, 17)
    corners = ((0, 0), (32, 0), (30, 18), (2, 18))
    for make in (lambda **kw: process.VideoTransformFilter(red, rect, **kw), lambda **kw: process.VideoCornerPinFilter(red, rect, corners, **kw)):
        node = make(filter="catmull-rom")
        assert node.filter == "catmull-rom"
        node = make()
        assert node.filter == "bilinear"
        for good in ("catmull-rom", "nearest", "catmull-rom", "bilinear", "catmull-rom"):
            node.filter = good
            assert node.filter == good
        for bad in ("bicubic", "cubic", "", "Catmull-Rom", "catmull_rom", 4, 4.0, None, b"catmull-rom"):
            with pytest.raises((TypeError, ValueError)) as e:
                node.filter = bad
            assert "catmull-rom" in str(e.value) and "bilinear" in str(e.value) and "nearest" in str(e.value)
            assert node.filter == "catmull-rom"
            with pytest.raises((TypeError, ValueError)):
                make(filter=bad)
        assert "catmull-rom" in type(node).filter.__doc__


def test_a_pull_without_a_device_gives_an_empty_window_and_never_raises():
    script = """
import sys
sys.path.insert(0, %r)
from fluggo.media import process, basetypes
window = basetypes.box2i(0, 0, 31, 17)
red = process.SolidColorVideoSource((1, 0, 0, 1))
corners = ((0, 0), (32, 0), (30, 18), (2, 18))
for source in (None, red):
    for node in (process.VideoTransformFilter(source, window, (16, 9), (1, 1), 30.0, (16, 9), "catmull-rom"),
                 process.VideoCornerPinFilter(source, window, corners, "catmull-rom")):
        assert node.filter == "catmull-rom"
        assert node.get_frame_f16(0, window).current_window.empty()
        assert node.get_frame_f32(0, window).current_window.empty()
        assert process.last_error(), "no message"
print("message:", process.last_error())
""" % ROOT
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    p = subprocess.run([os.sys.executable, "-c", script], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout
    assert "message:" in p.stdout and re.search(r"device|HIP|hip", p.stdout), p.stdout
