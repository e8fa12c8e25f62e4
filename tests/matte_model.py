"""Numpy statement of the matte refine's contract (DESIGN.md "Matte refine"), independent of the kernel and of host/matte.c.

Every intermediate is cast to float32, so every operation is rounded on its own, the same in both arithmetic flavours.  With
S the source's current window, r = |choke|, c = (ntaps - 1) / 2 and inv = 1.0f / (white - black):

    a0 = s.a, a NaN alpha counting as 0
    a1 = ramp((a0 - black) * inv) unless black == 0 and white == 1 ;  ramp(t) = (t < 1) ? ((t > 0) ? t : 0) : 1
    a2(x, y) = min (choke > 0) or max (choke < 0) of a1 over the square |i| <= r, |j| <= r clipped to S; choke == 0: a1
    h(x, y)  = t after: t = 0; for k ascending: if (x + k - c, y) in S: t = t + a2(x + k - c, y) * taps[k]
    a3(x, y) = t after: t = 0; for k ascending: if (x, y + k - c) in S: t = t + h(x, y + k - c) * taps[k]       no taps: a2
    out = show_matte ? (a3, a3, a3, 1) : (s.r, s.g, s.b code for code, a3)

All of it over the whole of S, plain loops over offsets and taps; the caller crops.  `s` is the source pixel; an f16 source is
widened exactly (tests/unsharp_model.py widen); f16 results are truncated once, by tests/models.py f2h_rz_model, and colour
codes are the source's own."""
import numpy as np

from tests.models import f2h_rz_model
from tests.unsharp_model import crop, intersect, widen  # noqa: F401  (re-exported for the tests)

F32 = np.float32


def ramp(t):
    t = np.asarray(t, F32)
    with np.errstate(invalid="ignore"):
        return np.where(t < 1, np.where(t > 0, t, F32(0)), F32(1)).astype(F32)


def levels(a0, black, white):
    """a1 over an array of alphas without NaNs"""
    black, white = F32(black), F32(white)
    if black == 0 and white == 1:
        return a0.copy()
    with np.errstate(all="ignore"):
        inv = F32(F32(1.0) / F32(white - black))
        return ramp(((a0 - black).astype(F32) * inv).astype(F32))


def choke_plane(a1, choke):
    """a2: the plane IS S, so offsets that leave the array are the skipped samples"""
    r = abs(int(choke))
    if r == 0:
        return a1.copy()
    h, w = a1.shape
    pick = np.minimum if choke > 0 else np.maximum
    out = a1.copy()
    for j in range(-r, r + 1):
        for i in range(-r, r + 1):
            ys, ye, xs, xe = max(0, -j), min(h, h - j), max(0, -i), min(w, w - i)
            if ys >= ye or xs >= xe:
                continue
            out[ys:ye, xs:xe] = pick(out[ys:ye, xs:xe], a1[ys + j:ye + j, xs + i:xe + i])
    return out


def _fir(plane, taps, axis):
    """One pass along `axis` (1: x, 0: y) over a plane that is S: t = 0, then t = t + sample * tap for the taps inside, ascending."""
    c = (len(taps) - 1) // 2
    n = plane.shape[axis]
    out = np.zeros_like(plane)
    index = np.arange(n)
    with np.errstate(all="ignore"):
        for k, tap in enumerate(taps):
            src = index + k - c
            ok = (src >= 0) & (src < n)
            if not ok.any():
                continue
            if axis == 1:
                p = (plane[:, src[ok]] * F32(tap)).astype(F32)
                out[:, ok] = (out[:, ok] + p).astype(F32)
            else:
                p = (plane[src[ok], :] * F32(tap)).astype(F32)
                out[ok, :] = (out[ok, :] + p).astype(F32)
    return out


def feather_plane(a2, taps):
    if taps is None or len(taps) == 0:
        return a2.copy()
    taps = [F32(t) for t in taps]
    return _fir(_fir(a2, taps, 1), taps, 0)


def refine_alpha(alpha, choke=0, feather=None, black=0.0, white=1.0):
    """a3 over a plane of f32 alphas that is the whole of S"""
    a0 = np.ascontiguousarray(alpha, F32).copy()
    a0[np.isnan(a0)] = F32(0)
    return feather_plane(choke_plane(levels(a0, black, white), choke), feather)


def refine_pixels(pixels, choke=0, feather=None, black=0.0, white=1.0, show_matte=False):
    """Pixels over S in either format (uint16 codes or f32) -> refined pixels in the same format."""
    half = pixels.dtype == np.uint16
    alpha = widen(pixels[..., 3]) if half else np.ascontiguousarray(pixels[..., 3], F32)
    a3 = refine_alpha(alpha, choke, feather, black, white)
    out = pixels.copy()
    code = f2h_rz_model(a3) if half else a3
    if show_matte:
        for ch in range(3):
            out[..., ch] = code
        out[..., 3] = 0x3C00 if half else F32(1.0)
    else:
        out[..., 3] = code
    return out


def expected(before, target_full, source, source_full, source_cur, choke=0, feather=None, black=0.0, white=1.0, show_matte=False):
    """The target buffer after the call and its window.  before: the target's pixels beforehand (uint16 codes or f32);
    source: pixels over source_full in the same format.  Every stage runs over the whole of source_cur; the window written is
    its crop to target_full, and pixels outside it keep what `before` held."""
    out = before.copy()
    win = None if source_cur is None else intersect(source_cur, target_full)
    if win is None:
        return out, None
    refined = refine_pixels(crop(source, source_full, source_cur), choke, feather, black, white, show_matte)
    crop(out, target_full, win)[...] = crop(refined, source_cur, win)
    return out, win


def soft_disc(width, height):
    """An alpha plane: a disc with an edge a few pixels wide, 1 inside and 0 outside"""
    yy, xx = np.mgrid[0:height, 0:width].astype(np.float64)
    d = np.hypot((xx - width / 2.0) / max(width * 0.35, 1.0), (yy - height / 2.0) / max(height * 0.35, 1.0))
    return np.clip((1.0 - d) * 4.0 + 0.5, 0.0, 1.0).astype(F32)
