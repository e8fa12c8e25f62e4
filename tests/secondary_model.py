"""Numpy statement of the secondaries' contract (DESIGN.md "Secondaries"; include/canvas_secondary.h): the qualifier that makes
a matte from hue, saturation and luma, and the mix of two frames through a matte.  Everything is float32, one operation per
statement, the host's precomputation included; half frames are widened exactly and truncated once (tests/models.py
f2h_rz_model), colours and selected pixels pass code for code."""
import numpy as np

from tests.models import f2h_rz_model
from tests.unsharp_model import crop, intersect, widen  # noqa: F401  (re-exported for the tests)

F32 = np.float32
C0, C1, C2 = F32(0.2126), F32(0.7152), F32(0.0722)
ONE, ZERO, SIX = F32(1), F32(0), F32(6)


class Qualifier:
    """hue: None or (center, width, softness) in degrees; saturation, luma: None or (low, high, soft_low, soft_high)"""

    def __init__(self, hue=None, saturation=None, luma=None, invert=False, show_matte=False):
        self.hue, self.saturation, self.luma, self.invert, self.show_matte = hue, saturation, luma, invert, show_matte

    def __repr__(self):
        return "Qualifier(hue=%r, saturation=%r, luma=%r, invert=%r, show_matte=%r)" % (self.hue, self.saturation, self.luma, self.invert, self.show_matte)


def sel(t):
    """(t > 0) ? ((t < 1) ? t : 1) : 0; NaN -> 0"""
    return np.where(t > 0, np.where(t < 1, t, ONE), ZERO).astype(F32)


def luma_of(r, g, b):
    with np.errstate(all="ignore"):
        p0 = (r * C0).astype(F32)
        p1 = (g * C1).astype(F32)
        p2 = (b * C2).astype(F32)
        s = (p0 + p1).astype(F32)
        return (s + p2).astype(F32)


def hue_plan(hue):
    """what the host forms of a hue range: (hc, hw, h_edge, hs, inv_hs or None)"""
    center, width, softness = (F32(v) for v in hue)
    hc = F32(np.fmod(center, F32(360)))
    hc = F32(hc / F32(60))
    if hc < 0:
        hc = F32(hc + SIX)
    hw = F32(width / F32(120))
    hs = F32(softness / F32(60))
    h_edge = F32(hw + hs)
    return hc, hw, h_edge, hs, (F32(ONE / hs) if hs > 0 else None)


def hue_of(r, g, b):
    """(h in sextants where c > 0 (elsewhere 0), c) of f32 arrays without NaNs in any channel that matters"""
    with np.errstate(all="ignore"):
        mx = np.maximum(np.maximum(r, g), b)
        mn = np.minimum(np.minimum(r, g), b)
        c = (mx - mn).astype(F32)
        rmax = r == mx
        gmax = (g == mx) & ~rmax
        num = np.where(rmax, (g - b).astype(F32), np.where(gmax, (b - r).astype(F32), (r - g).astype(F32))).astype(F32)
        q = (num / c).astype(F32)
        wrapped = (q + SIX).astype(F32)
        h = np.where(rmax, np.where(q < 0, wrapped, q), np.where(gmax, (q + F32(2)).astype(F32), (q + F32(4)).astype(F32))).astype(F32)
    return np.where(c > 0, h, ZERO).astype(F32), c


def range_of(rng, v):
    low, high, soft_low, soft_high = (F32(x) for x in rng)
    with np.errstate(all="ignore"):
        if soft_low > 0:
            lo_edge = F32(low - soft_low)
            inv = F32(ONE / soft_low)
            t = (v - lo_edge).astype(F32)
            lo = sel((t * inv).astype(F32))
        else:
            lo = np.where(v >= low, ONE, ZERO).astype(F32)
        if soft_high > 0:
            hi_edge = F32(high + soft_high)
            inv = F32(ONE / soft_high)
            t = (hi_edge - v).astype(F32)
            hi = sel((t * inv).astype(F32))
        else:
            hi = np.where(v <= high, ONE, ZERO).astype(F32)
    return np.where(hi < lo, hi, lo).astype(F32)


def matte_of(key, q):
    """(..., 4) f32 key pixels -> m, the factor on the source's alpha, (...) f32"""
    key = np.ascontiguousarray(key, F32)
    r, g, b = key[..., 0], key[..., 1], key[..., 2]
    nan = np.isnan(r) | np.isnan(g) | np.isnan(b)
    with np.errstate(all="ignore"):
        h, c = hue_of(r, g, b)
        mx = np.maximum(np.maximum(r, g), b)
        m = np.ones(r.shape, F32)
        if q.hue is not None:
            hc, hw, h_edge, hs, inv_hs = hue_plan(q.hue)
            d = np.abs((h - hc).astype(F32))
            e = (SIX - d).astype(F32)
            d = np.where(e < d, e, d).astype(F32)
            if inv_hs is not None:
                t = (h_edge - d).astype(F32)
                mh = sel((t * inv_hs).astype(F32))
            else:
                mh = np.where(d <= hw, ONE, ZERO).astype(F32)
            m = np.where(c > 0, mh, ZERO).astype(F32)
        if q.saturation is not None:
            s = np.where(mx > 0, (c / mx).astype(F32), ZERO).astype(F32)
            m = (m * range_of(q.saturation, s)).astype(F32)
        if q.luma is not None:
            m = (m * range_of(q.luma, luma_of(r, g, b))).astype(F32)
        m = np.where(nan, ZERO, m).astype(F32)
        if q.invert:
            m = (ONE - m).astype(F32)
    return m


def qualify_pixels(source, key, q):
    """Pixels in either format (uint16 codes or f32), source and key of one shape (key None: the source) -> the qualified pixels"""
    half = source.dtype == np.uint16
    s = widen(source) if half else np.ascontiguousarray(source, F32)
    k = s if key is None else (widen(key) if half else np.ascontiguousarray(key, F32))
    with np.errstate(all="ignore"):
        a1 = (s[..., 3] * matte_of(k, q)).astype(F32)
    if half:
        code = f2h_rz_model(a1)
        out = np.ascontiguousarray(source).copy()
        if q.show_matte:
            out[..., 0] = out[..., 1] = out[..., 2] = code
            out[..., 3] = 0x3C00
        else:
            out[..., 3] = code
        return out
    out = s.copy()
    if q.show_matte:
        out[..., 0] = out[..., 1] = out[..., 2] = a1
        out[..., 3] = ONE
    else:
        out[..., 3] = a1
    return out


def weight_of(matte, luma=False, invert=False):
    m = np.ascontiguousarray(matte, F32)
    with np.errstate(all="ignore"):
        k = sel(luma_of(m[..., 0], m[..., 1], m[..., 2]) if luma else m[..., 3])
        if invert:
            k = (ONE - k).astype(F32)
    return k


def mix_pixels(a, b, matte, luma=False, invert=False):
    """Pixels in either format, all of one shape -> a + k * (b - a) with k from the matte; k == 0 and k == 1 select codes"""
    half = a.dtype == np.uint16
    fa, fb, fm = (widen(x) if half else np.ascontiguousarray(x, F32) for x in (a, b, matte))
    k = weight_of(fm, luma, invert)[..., None]
    with np.errstate(all="ignore"):
        e = (fb - fa).astype(F32)
        f = (k * e).astype(F32)
        o = (fa + f).astype(F32)
    if half:
        o = f2h_rz_model(o)
        return np.where(k == 0, np.ascontiguousarray(a), np.where(k == 1, np.ascontiguousarray(b), o)).astype(np.uint16)
    bits = np.where(k == 0, fa.view(np.uint32), np.where(k == 1, fb.view(np.uint32), o.view(np.uint32))).astype(np.uint32)
    return bits.view(F32)


def window_of(target_full, *currents):
    """the window worked on: the intersection of every input's current window (None: empty) with the target's buffer"""
    win = tuple(target_full)
    for cur in currents:
        if cur is None or win is None:
            return None
        win = intersect(win, cur)
    return win


def expected_qualify(before, tfull, source, sfull, scur, q, key=None, kfull=None, kcur=None):
    """The target buffer after the call and its window (pixels outside it keep what `before` held); key None: no key frame"""
    out = before.copy()
    win = window_of(tfull, scur) if key is None else window_of(tfull, scur, kcur)
    if win is None:
        return out, None
    crop(out, tfull, win)[...] = qualify_pixels(crop(source, sfull, win), None if key is None else crop(key, kfull, win), q)
    return out, win


def expected_mix(before, tfull, a, afull, acur, b, bfull, bcur, matte, mfull, mcur, luma=False, invert=False):
    out = before.copy()
    win = window_of(tfull, acur, bcur, mcur)
    if win is None:
        return out, None
    crop(out, tfull, win)[...] = mix_pixels(crop(a, afull, win), crop(b, bfull, win), crop(matte, mfull, win), luma, invert)
    return out, win
