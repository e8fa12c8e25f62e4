"""Numpy statement of the affine transform's contract (DESIGN.md "Affine transform"), independent of the kernel and of
host/transform.c.

Pixels: every intermediate is cast to float32, so every operation is rounded on its own, the same in both arithmetic flavours.
With S the source's current window and m the TARGET -> SOURCE coefficients (f32):

    x, y = float32 of the target pixel's coordinates;  u = (m0*x + m1*y) + m2;  v = (m3*x + m4*y) + m5
    in(i, j) = S.min.x <= i <= S.max.x and S.min.y <= j <= S.max.y, compared as floats (false for NaN and +-Inf)
    nearest:   i = floor(u + 0.5), j = floor(v + 0.5);  out = in(i, j) ? source(i, j) code for code : (0, 0, 0, 0)
    bilinear:  i = floor(u), j = floor(v);  a = u - i;  b = v - j;  wa = 1 - a;  wb = 1 - b
               a == 0 and b == 0:  out = in(i, j) ? source(i, j) code for code : (0, 0, 0, 0)
               else A = R = G = B = 0;  for (w, di, dj) in (wa*wb, 0, 0), (a*wb, 1, 0), (wa*b, 0, 1), (a*b, 1, 1):
                        if in(i + di, j + dj):  p = source(i + di, j + dj);  q = w * p.a;  A = A + q;  R = R + q*p.r; ...
                    out = A != 0 ? (R / A, G / A, B / A, A) : (0, 0, 0, 0)

An f16 source is widened exactly; f16 results are truncated once (tests/models.py f2h_rz_model), the copy paths move the code.
Windows: float64, every operation on its own, in the order DESIGN.md writes them."""
import math

import numpy as np

from tests.models import f2h_rz_model
from tests.unsharp_model import crop, intersect, widen  # noqa: F401  (re-exported for the tests)

F32 = np.float32
NEAREST, BILINEAR = 0, 1
LIMIT = float(1 << 30)


# ---------------------------------------------------------------- coefficients and windows, float64

def from_parts(anchor=(0.0, 0.0), scale=(1.0, 1.0), rotation=0.0, position=(0.0, 0.0)):
    """The six f32 coefficients (target -> source) of  target = position + R * diag(scale) * (p - anchor), or None when a scale is 0."""
    ax, ay, sx, sy, px, py, rotation = (float(v) for v in (anchor[0], anchor[1], scale[0], scale[1], position[0], position[1], rotation))
    if sx == 0.0 or sy == 0.0:
        return None
    q = math.fmod(rotation, 360.0)
    if q < 0.0:
        q = q + 360.0
    exact = {0.0: (1.0, 0.0), 90.0: (0.0, 1.0), 180.0: (-1.0, 0.0), 270.0: (0.0, -1.0)}
    if q in exact:
        c, s = exact[q]
    else:
        r = rotation * math.pi / 180.0
        c, s = math.cos(r), math.sin(r)
    f00, f01, f10, f11 = sx * c, -sy * s, sx * s, sy * c
    f02 = px - (f00 * ax + f01 * ay)
    f12 = py - (f10 * ax + f11 * ay)
    det = f00 * f11 - f01 * f10
    m0, m1, m3, m4 = f11 / det, -f01 / det, -f10 / det, f00 / det
    m2 = -(m0 * f02 + m1 * f12)
    m5 = -(m3 * f02 + m4 * f12)
    return tuple(float(F32(v)) for v in (m0, m1, m2, m3, m4, m5))


def forward(m):
    """F (source -> target) of the f32 coefficients m, in float64: (f00, f01, f02, f10, f11, f12)"""
    m = [float(F32(v)) for v in m]
    det = m[0] * m[4] - m[1] * m[3]
    f00, f01, f10, f11 = m[4] / det, -m[1] / det, -m[3] / det, m[0] / det
    return f00, f01, -(f00 * m[2] + f01 * m[5]), f10, f11, -(f10 * m[2] + f11 * m[5])


def _bounds(values, pad):
    if any(math.isnan(v) for v in values):
        return int(-LIMIT), int(LIMIT)
    lo, hi = min(values), max(values)
    if math.isfinite(lo):                                            # C's floor and ceil leave an infinity as it is
        lo = math.floor(lo) - pad
    if math.isfinite(hi):
        hi = math.ceil(hi) + pad
    return int(min(max(lo, -LIMIT), LIMIT)), int(min(max(hi, -LIMIT), LIMIT))


def target_window(m, filt, S, target_full):
    """The window the entry writes, as a tuple, or None when it is empty.  S, target_full: (x0, y0, x1, y1) or None."""
    if S is None or target_full is None:
        return None
    f00, f01, f02, f10, f11, f12 = forward(m)
    g = 1.0 if filt == BILINEAR else 0.5
    corners = [(S[0] - g, S[1] - g), (S[2] + g, S[1] - g), (S[0] - g, S[3] + g), (S[2] + g, S[3] + g)]
    tx = [f00 * sx + f01 * sy + f02 for sx, sy in corners]
    ty = [f10 * sx + f11 * sy + f12 for sx, sy in corners]
    (x0, x1), (y0, y1) = _bounds(tx, 1), _bounds(ty, 1)
    return intersect((x0, y0, x1, y1), target_full)


def source_window(m, window):
    """The source pixels the taps of target window `window` can touch (not clipped to anything)."""
    if window is None:
        return None
    m = [float(F32(v)) for v in m]
    corners = [(window[0], window[1]), (window[2], window[1]), (window[0], window[3]), (window[2], window[3])]
    u = [m[0] * float(x) + m[1] * float(y) + m[2] for x, y in corners]
    v = [m[3] * float(x) + m[4] * float(y) + m[5] for x, y in corners]
    (x0, x1), (y0, y1) = _bounds(u, 2), _bounds(v, 2)
    return (x0, y0, x1, y1)


# ---------------------------------------------------------------- pixels, float32

def source_coords(m, window):
    """u, v (float32 planes) of every pixel of target window `window`"""
    m = [F32(v) for v in m]
    x = np.arange(window[0], window[2] + 1, dtype=np.int64).astype(F32)[None, :]
    y = np.arange(window[1], window[3] + 1, dtype=np.int64).astype(F32)[:, None]
    with np.errstate(all="ignore"):
        u = ((m[0] * x).astype(F32) + (m[1] * y).astype(F32)).astype(F32) + m[2]
        v = ((m[3] * x).astype(F32) + (m[4] * y).astype(F32)).astype(F32) + m[5]
    return u.astype(F32), v.astype(F32)


def inside(i, j, S):
    """in(i, j) over float32 planes of tap coordinates"""
    with np.errstate(invalid="ignore"):
        return (i >= F32(S[0])) & (i <= F32(S[2])) & (j >= F32(S[1])) & (j <= F32(S[3]))


def _fetch(src, S, i, j, ok):
    """source(i, j) where ok (elsewhere the pixel at S's corner, to be discarded): never an index outside S"""
    ii = np.where(ok, i, F32(S[0])).astype(np.int64) - S[0]
    jj = np.where(ok, j, F32(S[1])).astype(np.int64) - S[1]
    return src[jj, ii]


def transform_plane(source, S, m, filt, window):
    """The infinite-plane result over target window `window`.  source: pixels over S (uint16 codes or float32) -> same format."""
    return sample(source, S, *source_coords(m, window), filt)


def sample(source, S, u, v, filt):
    """The filter from the source coordinates on, shared with tests/perspective_model.py: S and the float32 planes u, v in one
    coordinate system, source the pixels over S."""
    half = source.dtype == np.uint16
    wide = widen(source) if half else np.ascontiguousarray(source, F32)
    out = np.zeros(u.shape + (4,), source.dtype)
    with np.errstate(all="ignore"):
        if filt == NEAREST:
            i, j = np.floor((u + F32(0.5)).astype(F32)), np.floor((v + F32(0.5)).astype(F32))
            ok = inside(i, j, S)
            out[ok] = _fetch(source, S, i, j, ok)[ok]
            return out
        i, j = np.floor(u), np.floor(v)
        a, b = (u - i).astype(F32), (v - j).astype(F32)
        wa, wb = (F32(1) - a).astype(F32), (F32(1) - b).astype(F32)
        A = np.zeros(u.shape, F32)
        C = [np.zeros(u.shape, F32) for _ in range(3)]
        for w, di, dj in (((wa * wb).astype(F32), 0, 0), ((a * wb).astype(F32), 1, 0), ((wa * b).astype(F32), 0, 1), ((a * b).astype(F32), 1, 1)):
            ti, tj = (i + F32(di)).astype(F32), (j + F32(dj)).astype(F32)
            ok = inside(ti, tj, S)
            p = _fetch(wide, S, ti, tj, ok)
            q = (w * p[..., 3]).astype(F32)
            A = np.where(ok, (A + q).astype(F32), A)
            for ch in range(3):
                C[ch] = np.where(ok, (C[ch] + (q * p[..., ch]).astype(F32)).astype(F32), C[ch])
        solid = A != 0
        result = np.zeros(u.shape + (4,), F32)
        for ch in range(3):
            result[..., ch] = np.where(solid, (C[ch] / A).astype(F32), F32(0))
        result[..., 3] = np.where(solid, A, F32(0))
        out[...] = f2h_rz_model(result) if half else result
        on_sample = (a == 0) & (b == 0)
        ok = inside(i, j, S)
        copied = np.where(ok[..., None], _fetch(source, S, i, j, ok), np.zeros(4, source.dtype))
        out[on_sample] = copied[on_sample]
    return out


def expected(before, target_full, source, source_full, source_cur, m, filt):
    """The target buffer after the call and its window (None: empty).  before: the target's pixels beforehand; source: pixels
    over source_full in the same format."""
    out = before.copy()
    win = target_window(m, filt, source_cur, target_full)
    if win is None:
        return out, None
    crop(out, target_full, win)[...] = transform_plane(crop(source, source_full, source_cur), source_cur, m, filt, win)
    return out, win
