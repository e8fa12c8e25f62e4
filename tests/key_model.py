"""Numpy statement of the chroma key's contract (DESIGN.md "Chroma key"), independent of the kernel and of host/key.c.

Every intermediate is cast to float32, so every operation is rounded on its own, the same in both arithmetic flavours:

    kpb = (key.r*c10 + key.g*c11) + key.b*c12 ;  kpr likewise with row 2        inv_soft = 1 / softness, inv_spill = 1 / spill_range
    pb = (s.r*c10 + s.g*c11) + s.b*c12 ;  pr = (s.r*c20 + s.g*c21) + s.b*c22
    dx = pb - kpb ; dy = pr - kpr ; d = sqrt(dx*dx + dy*dy)                     np.sqrt on float32: correctly rounded
    ramp(t) = (t < 1) ? ((t > 0) ? t : 0) : 1                                    NaN -> 1
    m  = softness > 0 ? ramp((d - tolerance) * inv_soft) : (d <= tolerance ? 0 : 1) ;  a' = s.a * m
    spill > 0 (after the clamp to [0, 1]):
        q  = spill_range > 0 ? ramp((d - tolerance) * inv_spill) : (d <= tolerance ? 0 : 1)
        ws = spill * (1 - q) ;  y = (s.r*c00 + s.g*c01) + s.b*c02 ;  for c in r, g, b:  e = y - s.c ; f = ws * e ; c' = s.c + f
    else c' = s.c, code for code
    out = show_matte ? (a', a', a', 1) : (r', g', b', a')

`s` is the source pixel; an f16 source is widened exactly (tests/unsharp_model.py widen); f16 results are truncated once, by
tests/models.py f2h_rz_model, except that colour codes the key does not touch (spill == 0, no matte view) are the source's."""
import numpy as np

from tests.models import f2h_rz_model
from tests.unsharp_model import crop, intersect, widen  # noqa: F401  (re-exported for the tests)

F32 = np.float32
C0 = (F32(0.2126), F32(0.7152), F32(0.0722))
C1 = (F32(-0.114572), F32(-0.385428), F32(0.5))
C2 = (F32(0.5), F32(-0.454153), F32(-0.045847))


def _row(r, g, b, c):
    """(r*c0 + g*c1) + b*c2, each operation rounded to f32"""
    t = ((r * c[0]).astype(F32) + (g * c[1]).astype(F32)).astype(F32)
    return (t + (b * c[2]).astype(F32)).astype(F32)


def ramp(t):
    t = np.asarray(t, F32)
    with np.errstate(invalid="ignore"):
        return np.where(t < 1, np.where(t > 0, t, F32(0)), F32(1)).astype(F32)


def clamp_spill(spill):
    spill = F32(spill)
    return (spill if spill < 1 else F32(1)) if spill > 0 else F32(0)


def distance(s, key):
    """d of every pixel of the (..., 4) f32 array `s` from the colour key[0:3]"""
    s = np.ascontiguousarray(s, F32)
    k = [np.asarray(F32(v)) for v in key[:3]]
    with np.errstate(all="ignore"):
        kpb, kpr = _row(k[0], k[1], k[2], C1), _row(k[0], k[1], k[2], C2)
        dx = (_row(s[..., 0], s[..., 1], s[..., 2], C1) - kpb).astype(F32)
        dy = (_row(s[..., 0], s[..., 1], s[..., 2], C2) - kpr).astype(F32)
        return np.sqrt(((dx * dx).astype(F32) + (dy * dy).astype(F32)).astype(F32)).astype(F32)


def _edge(d, tolerance, width):
    """ramp((d - tolerance) * (1 / width)) for width > 0, the hard edge otherwise"""
    tolerance, width = F32(tolerance), F32(width)
    with np.errstate(all="ignore"):
        if width > 0:
            return ramp(((d - tolerance).astype(F32) * (F32(1.0) / width)).astype(F32))
        return np.where(d <= tolerance, F32(0), F32(1)).astype(F32)


def matte(s, key, tolerance, softness):
    """m of every pixel"""
    return _edge(distance(s, key), tolerance, softness)


def spill_weight(s, key, tolerance, spill, spill_range):
    """ws of every pixel (zeros when the clamped spill is 0)"""
    spill = clamp_spill(spill)
    d = distance(s, key)
    if not spill > 0:
        return np.zeros(d.shape, F32)
    with np.errstate(all="ignore"):
        return (spill * (F32(1.0) - _edge(d, tolerance, spill_range)).astype(F32)).astype(F32)


def key_f32(s, key, tolerance, softness, spill=0.0, spill_range=0.0, show_matte=False):
    """(..., 4) f32 pixels -> the keyed pixels, f32"""
    s = np.ascontiguousarray(s, F32)
    out = s.copy()
    with np.errstate(all="ignore"):
        alpha = (s[..., 3] * matte(s, key, tolerance, softness)).astype(F32)
        if show_matte:
            for c in range(3):
                out[..., c] = alpha
            out[..., 3] = F32(1.0)
            return out
        out[..., 3] = alpha
        if clamp_spill(spill) > 0:
            ws = spill_weight(s, key, tolerance, spill, spill_range)
            y = _row(s[..., 0], s[..., 1], s[..., 2], C0)
            for c in range(3):
                e = (y - s[..., c]).astype(F32)
                out[..., c] = (s[..., c] + (ws * e).astype(F32)).astype(F32)
    return out


def key_pixels(pixels, key, tolerance, softness, spill=0.0, spill_range=0.0, show_matte=False):
    """Pixels in either format (uint16 codes or f32) -> keyed pixels in the same format."""
    if pixels.dtype != np.uint16:
        return key_f32(pixels, key, tolerance, softness, spill, spill_range, show_matte)
    out = f2h_rz_model(key_f32(widen(pixels), key, tolerance, softness, spill, spill_range, show_matte))
    if not show_matte and not clamp_spill(spill) > 0:
        out[..., :3] = pixels[..., :3]                                  # code for code, signalling NaNs included
    return out


def expected(before, target_full, source, source_full, source_cur, key, tolerance, softness, spill=0.0, spill_range=0.0, show_matte=False):
    """The target buffer after the call and its window.  before: the target's pixels beforehand (uint16 codes or f32);
    source: pixels over source_full in the same format.  Pixels outside the window keep what `before` held."""
    out = before.copy()
    win = None if source_cur is None else intersect(source_cur, target_full)
    if win is None:
        return out, None
    crop(out, target_full, win)[...] = key_pixels(crop(source, source_full, win), key, tolerance, softness, spill, spill_range, show_matte)
    return out, win


GREEN = (0.08, 0.62, 0.12)


def green_screen(width, height, seed=0, key=GREEN):
    """A synthetic green-screen shot as f32 RGBA, opaque: an elliptical subject of varied colours over a ground of the key colour
    (slightly uneven, as a lit screen is), a soft edge about a sixth of the subject wide where the two mix, and green spill on
    the subject that grows towards its rim.  Seeded: the same picture for the same arguments."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:height, 0:width].astype(np.float64)
    cx, cy, rx, ry = width / 2.0, height / 2.0, max(width * 0.42, 1.0), max(height * 0.45, 1.0)
    r = np.sqrt(((xx - cx) / rx) ** 2 + ((yy - cy) / ry) ** 2)           # 1 on the subject's outline
    cover = np.clip((1.0 - r) / 0.6 + 0.5, 0.0, 1.0)                     # a wide soft edge: 0 ground .. 1 subject
    subject = np.stack([0.55 + 0.4 * np.sin(xx * 0.11 + 0.3), 0.35 + 0.3 * np.cos(yy * 0.07), 0.5 + 0.45 * np.sin((xx + yy) * 0.05)], -1)
    subject += rng.uniform(-0.03, 0.03, subject.shape)
    ground = np.array(key, np.float64) * (1.0 + rng.uniform(-0.06, 0.06, (height, width, 1)))
    spill = np.clip(r, 0.0, 1.0)[..., None] * 0.35                       # the screen's light on the subject
    lit = subject * (1.0 - spill) + np.array(key, np.float64) * spill
    rgb = lit * cover[..., None] + ground * (1.0 - cover[..., None])
    out = np.ones((height, width, 4), F32)
    out[..., :3] = rgb.astype(F32)
    return out
