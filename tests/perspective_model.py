"""Numpy statement of the corner pin's contract (DESIGN.md "Corner pin"), independent of the kernel and of host/perspective.c.

Pixels: every intermediate is cast to float32, so every operation is rounded on its own, the same in both arithmetic flavours.
With S the source's current window, S' = S - source_origin and h the TARGET -> SOURCE coefficients (f32) between the origins:

    x = float32(X - target_origin.x);  y = float32(Y - target_origin.y)
    nu = (h0*x + h1*y) + h2;  nv = (h3*x + h4*y) + h5;  w = (h6*x + h7*y) + h8
    not (w > 0):  out = (0, 0, 0, 0)
    u = nu / w;  v = nv / w
    then nearest / bilinear as tests/transform_model.py states them, in() tested against S', source(i, j) the pixel at
    (source_origin.x + i, source_origin.y + j)

Coefficients and windows: float64, every operation on its own, in the order DESIGN.md writes them."""
import math

import numpy as np

from tests import transform_model as tm
from tests.unsharp_model import crop, intersect, widen  # noqa: F401  (re-exported for the tests)

F32 = np.float32
NEAREST, BILINEAR = 0, 1
LIMIT = float(1 << 30)
WHOLE = (int(-LIMIT), int(-LIMIT), int(LIMIT), int(LIMIT))


def outer(box):
    """The outer edges of a box of samples: min - 1/2 .. max + 1/2"""
    return (box[0] - 0.5, box[1] - 0.5, box[2] + 0.5, box[3] + 0.5)


def rect_quad(rect):
    """The rectangle's own corners: top-left, top-right, bottom-right, bottom-left"""
    return [(rect[0], rect[1]), (rect[2], rect[1]), (rect[2], rect[3]), (rect[0], rect[3])]


def _clamp(v):
    return min(max(v, -LIMIT), LIMIT)


# ---------------------------------------------------------------- coefficients and windows, float64

def from_quad(rect, quad):
    """(h: nine floats that are float32 values, target_origin, source_origin) of the map that puts `rect` = (x0, y0, x1, y1) onto
    `quad` (top-left, top-right, bottom-right, bottom-left), or None when the quad is not strictly convex."""
    rect = [float(v) for v in rect]
    quad = [(float(a), float(b)) for a, b in quad]
    tox = _clamp(math.floor(((quad[0][0] + quad[1][0]) + (quad[2][0] + quad[3][0])) / 4.0))
    toy = _clamp(math.floor(((quad[0][1] + quad[1][1]) + (quad[2][1] + quad[3][1])) / 4.0))
    sox = _clamp(math.floor((rect[0] + rect[2]) / 2.0))
    soy = _clamp(math.floor((rect[1] + rect[3]) / 2.0))
    x = [q[0] - tox for q in quad]
    y = [q[1] - toy for q in quad]
    rx0, ry0, rx1, ry1 = rect[0] - sox, rect[1] - soy, rect[2] - sox, rect[3] - soy
    W, H = rx1 - rx0, ry1 - ry0
    c = []
    for k in range(4):
        k1, k2 = (k + 1) % 4, (k + 2) % 4
        c.append((x[k1] - x[k]) * (y[k2] - y[k1]) - (y[k1] - y[k]) * (x[k2] - x[k1]))
    if not (all(v > 0 for v in c) or all(v < 0 for v in c)):
        return None
    sx = (x[0] - x[1]) + (x[2] - x[3])
    sy = (y[0] - y[1]) + (y[2] - y[3])
    if sx == 0.0 and sy == 0.0:
        f00, f01, f10, f11 = (x[1] - x[0]) / W, (x[3] - x[0]) / H, (y[1] - y[0]) / W, (y[3] - y[0]) / H
        f02 = x[0] - (f00 * rx0 + f01 * ry0)
        f12 = y[0] - (f10 * rx0 + f11 * ry0)
        det = f00 * f11 - f01 * f10
        r0, r1, r3, r4 = f11 / det, -f01 / det, -f10 / det, f00 / det
        r = [r0, r1, -(r0 * f02 + r1 * f12), r3, r4, -(r3 * f02 + r4 * f12), 0.0, 0.0, 1.0]
    else:
        dx1, dx2, dy1, dy2 = x[1] - x[2], x[3] - x[2], y[1] - y[2], y[3] - y[2]
        den = dx1 * dy2 - dx2 * dy1
        g, hh = (sx * dy2 - dx2 * sy) / den, (dx1 * sy - sx * dy1) / den
        a, b, cc = (x[1] - x[0]) + g * x[1], (x[3] - x[0]) + hh * x[3], x[0]
        d, e, f = (y[1] - y[0]) + g * y[1], (y[3] - y[0]) + hh * y[3], y[0]
        a0 = (e - f * hh, cc * hh - b, b * f - cc * e)
        a1 = (f * g - d, a - cc * g, cc * d - a * f)
        a2 = (d * hh - e * g, b * g - a * hh, a * e - b * d)
        r = [rx0 * a2[k] + W * a0[k] for k in range(3)] + [ry0 * a2[k] + H * a1[k] for k in range(3)] + list(a2)
        cx, cy = ((x[0] + x[1]) + (x[2] + x[3])) / 4.0, ((y[0] + y[1]) + (y[2] + y[3])) / 4.0
        wc = (r[6] * cx + r[7] * cy) + r[8]
        r = [v / wc for v in r]
    return tuple(float(F32(v)) for v in r), (int(tox), int(toy)), (int(sox), int(soy))


def _bounds(values, pad, origin):
    if any(math.isnan(v) for v in values):
        return int(-LIMIT), int(LIMIT)
    lo, hi = min(values), max(values)
    if math.isfinite(lo):                                            # C's floor and ceil leave an infinity as it is
        lo = (math.floor(lo) - pad) + float(origin)
    if math.isfinite(hi):
        hi = (math.ceil(hi) + pad) + float(origin)
    return int(_clamp(lo)), int(_clamp(hi))


def forward(h):
    """adjugate / determinant of the f32 coefficients h, in float64: the nine coefficients source -> target"""
    h = [float(F32(v)) for v in h]
    adj = [h[4] * h[8] - h[5] * h[7], h[2] * h[7] - h[1] * h[8], h[1] * h[5] - h[2] * h[4],
           h[5] * h[6] - h[3] * h[8], h[0] * h[8] - h[2] * h[6], h[2] * h[3] - h[0] * h[5],
           h[3] * h[7] - h[4] * h[6], h[1] * h[6] - h[0] * h[7], h[0] * h[4] - h[1] * h[3]]
    det = (h[0] * adj[0] + h[1] * adj[3]) + h[2] * adj[6]
    return [v / det for v in adj]


def target_window(p, filt, S, target_full):
    """The window the entry writes, as a tuple, or None when it is empty.  p = (h, target_origin, source_origin)."""
    if S is None or target_full is None:
        return None
    h, to, so = p
    f = forward(h)
    g = 1.0 if filt == BILINEAR else 0.5
    x0, x1, y0, y1 = float(S[0] - so[0]) - g, float(S[2] - so[0]) + g, float(S[1] - so[1]) - g, float(S[3] - so[1]) + g
    tx, ty = [], []
    for sx, sy in ((x0, y0), (x1, y0), (x0, y1), (x1, y1)):
        nx, ny, w = (f[0] * sx + f[1] * sy) + f[2], (f[3] * sx + f[4] * sy) + f[5], (f[6] * sx + f[7] * sy) + f[8]
        if not w > 0.0:
            return tuple(target_full)
        tx.append(nx / w)
        ty.append(ny / w)
    (a0, a1), (b0, b1) = _bounds(tx, 1, to[0]), _bounds(ty, 1, to[1])
    return intersect((a0, b0, a1, b1), target_full)


def source_window(p, window):
    """The source pixels the taps of target window `window` can touch (not clipped to anything)."""
    if window is None:
        return None
    h, to, so = p
    h = [float(F32(v)) for v in h]
    x0, x1, y0, y1 = float(window[0] - to[0]), float(window[2] - to[0]), float(window[1] - to[1]), float(window[3] - to[1])
    u, v = [], []
    for x, y in ((x0, y0), (x1, y0), (x0, y1), (x1, y1)):
        nu, nv, w = (h[0] * x + h[1] * y) + h[2], (h[3] * x + h[4] * y) + h[5], (h[6] * x + h[7] * y) + h[8]
        if not w > 0.0:
            return WHOLE
        u.append(nu / w)
        v.append(nv / w)
    (a0, a1), (b0, b1) = _bounds(u, 2, so[0]), _bounds(v, 2, so[1])
    return (a0, b0, a1, b1)


# ---------------------------------------------------------------- pixels, float32

def source_coords(p, window):
    """u, v, w (float32 planes) of every pixel of target window `window`; u and v relative to the source origin"""
    h, to, _so = p
    h = [F32(v) for v in h]
    x = (np.arange(window[0], window[2] + 1, dtype=np.int64) - to[0]).astype(F32)[None, :]
    y = (np.arange(window[1], window[3] + 1, dtype=np.int64) - to[1]).astype(F32)[:, None]
    with np.errstate(all="ignore"):
        row = lambda a, b, c: (((a * x).astype(F32) + (b * y).astype(F32)).astype(F32) + c).astype(F32)
        nu, nv, w = row(h[0], h[1], h[2]), row(h[3], h[4], h[5]), row(h[6], h[7], h[8])
        u, v = (nu / w).astype(F32), (nv / w).astype(F32)
    return u, v, w


def perspective_plane(source, S, p, filt, window):
    """The infinite-plane result over target window `window`.  source: pixels over S (uint16 codes or float32) -> same format."""
    _h, _to, so = p
    rel = (S[0] - so[0], S[1] - so[1], S[2] - so[0], S[3] - so[1])
    u, v, w = source_coords(p, window)
    out = tm.sample(source, rel, u, v, filt)
    with np.errstate(invalid="ignore"):
        out[~(w > 0)] = 0
    return out


def expected(before, target_full, source, source_full, source_cur, p, filt):
    """The target buffer after the call and its window (None: empty).  before: the target's pixels beforehand; source: pixels
    over source_full in the same format."""
    out = before.copy()
    win = target_window(p, filt, source_cur, target_full)
    if win is None or source_cur is None:
        return out, None
    crop(out, target_full, win)[...] = perspective_plane(crop(source, source_full, source_cur), source_cur, p, filt, win)
    return out, win
