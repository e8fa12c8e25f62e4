"""Numpy statement of the Catmull-Rom filter of the two warps (DESIGN.md "Catmull-Rom warps"), independent of the kernels and
of host/transform.c and host/perspective.c.  u and v are those of tests/transform_model.py (source_coords) and of
tests/perspective_model.py (source_coords, with its w > 0 rule); they are not restated here.

Pixels: every intermediate is cast to float32, so every product and every sum is rounded on its own, the same in both arithmetic
flavours.  With S the source window in the coordinate system of u and v:

    i = floor(u), j = floor(v);  a = u - i;  b = v - j
    weights of a fraction t (wx[0..3] from a, wy[0..3] from b), Horner, in this order:
        w0 = ((-0.5*t + 1.0)*t - 0.5)*t        w1 = ((1.5*t - 2.5)*t)*t + 1.0
        w2 = ((-1.5*t + 2.0)*t + 0.5)*t        w3 = ((0.5*t - 0.5)*t)*t
    a == 0 and b == 0:  out = in(i, j) ? source(i, j) code for code : 0
    else  A = R = G = B = 0;  lo_c = +inf, hi_c = -inf per colour channel;  lo_a = +inf, hi_a = -inf
          for l in 0..3 (rows j-1+l), for k in 0..3 (columns i-1+k), in this order:
              p = source(i-1+k, j-1+l) if in(...);  counts = in(...) and p.a > 0
              if counts:  q = (wx[k]*wy[l]) * p.a;  A += q;  R += q*p.r;  G += q*p.g;  B += q*p.b
                          lo_c = fmin(lo_c, p.c);  hi_c = fmax(hi_c, p.c)
              ta = counts ? p.a : 0;  lo_a = fmin(lo_a, ta);  hi_a = fmax(hi_a, ta)
          out = A > 0 ? (clamp(R/A, lo_r, hi_r), clamp(G/A, ..), clamp(B/A, ..), clamp(A, lo_a, hi_a)) : 0
          clamp(t, lo, hi) = fmin(fmax(t, lo), hi);  fmin / fmax: a NaN operand loses (the sign of a zero they return is not pinned)

An f16 source is widened exactly; f16 results are truncated once (tests/models.py f2h_rz_model), the copy path moves the code.
Windows: float64, every operation on its own; S is grown by the filter's reach 2 (taps i-1 .. i+2) for the target window, and the
source window's pad around the mapped corners is 3."""
import numpy as np

from tests import perspective_model as pm
from tests import transform_model as tm
from tests.models import f2h_rz_model
from tests.unsharp_model import crop, intersect, widen  # noqa: F401  (re-exported for the tests)

F32 = np.float32
CATMULL_ROM = 4
REACH, PAD = 2.0, 3


# ---------------------------------------------------------------- windows, float64

def transform_target_window(m, S, target_full):
    if S is None or target_full is None:
        return None
    f00, f01, f02, f10, f11, f12 = tm.forward(m)
    g = REACH
    corners = [(S[0] - g, S[1] - g), (S[2] + g, S[1] - g), (S[0] - g, S[3] + g), (S[2] + g, S[3] + g)]
    tx = [f00 * sx + f01 * sy + f02 for sx, sy in corners]
    ty = [f10 * sx + f11 * sy + f12 for sx, sy in corners]
    (x0, x1), (y0, y1) = tm._bounds(tx, 1), tm._bounds(ty, 1)
    return intersect((x0, y0, x1, y1), target_full)


def transform_source_window(m, window):
    if window is None:
        return None
    m = [float(F32(v)) for v in m]
    corners = [(window[0], window[1]), (window[2], window[1]), (window[0], window[3]), (window[2], window[3])]
    u = [m[0] * float(x) + m[1] * float(y) + m[2] for x, y in corners]
    v = [m[3] * float(x) + m[4] * float(y) + m[5] for x, y in corners]
    (x0, x1), (y0, y1) = tm._bounds(u, PAD), tm._bounds(v, PAD)
    return (x0, y0, x1, y1)


def perspective_target_window(p, S, target_full):
    if S is None or target_full is None:
        return None
    h, to, so = p
    f = pm.forward(h)
    g = REACH
    x0, x1, y0, y1 = float(S[0] - so[0]) - g, float(S[2] - so[0]) + g, float(S[1] - so[1]) - g, float(S[3] - so[1]) + g
    tx, ty = [], []
    for sx, sy in ((x0, y0), (x1, y0), (x0, y1), (x1, y1)):
        nx, ny, w = (f[0] * sx + f[1] * sy) + f[2], (f[3] * sx + f[4] * sy) + f[5], (f[6] * sx + f[7] * sy) + f[8]
        if not w > 0.0:
            return tuple(target_full)
        tx.append(nx / w)
        ty.append(ny / w)
    (a0, a1), (b0, b1) = pm._bounds(tx, 1, to[0]), pm._bounds(ty, 1, to[1])
    return intersect((a0, b0, a1, b1), target_full)


def perspective_source_window(p, window):
    if window is None:
        return None
    h, to, so = p
    h = [float(F32(v)) for v in h]
    x0, x1, y0, y1 = float(window[0] - to[0]), float(window[2] - to[0]), float(window[1] - to[1]), float(window[3] - to[1])
    u, v = [], []
    for x, y in ((x0, y0), (x1, y0), (x0, y1), (x1, y1)):
        nu, nv, w = (h[0] * x + h[1] * y) + h[2], (h[3] * x + h[4] * y) + h[5], (h[6] * x + h[7] * y) + h[8]
        if not w > 0.0:
            return pm.WHOLE
        u.append(nu / w)
        v.append(nv / w)
    (a0, a1), (b0, b1) = pm._bounds(u, PAD, so[0]), pm._bounds(v, PAD, so[1])
    return (a0, b0, a1, b1)


# ---------------------------------------------------------------- pixels, float32

def weights(t):
    """(w0, w1, w2, w3) of the float32 plane t, every operation rounded on its own"""
    t = np.asarray(t, F32)
    f = lambda x: np.asarray(x, F32)
    with np.errstate(all="ignore"):
        w0 = f(f(f(f(f(F32(-0.5) * t) + F32(1.0)) * t) - F32(0.5)) * t)
        w1 = f(f(f(f(f(F32(1.5) * t) - F32(2.5)) * t) * t) + F32(1.0))
        w2 = f(f(f(f(f(F32(-1.5) * t) + F32(2.0)) * t) + F32(0.5)) * t)
        w3 = f(f(f(f(F32(0.5) * t) - F32(0.5)) * t) * t)
    return w0, w1, w2, w3


def fmin(a, b):
    """a NaN operand loses (the sign of a zero returned is not pinned: the tests fold it)"""
    return np.fmin(np.asarray(a, F32), np.asarray(b, F32)).astype(F32)


def fmax(a, b):
    return np.fmax(np.asarray(a, F32), np.asarray(b, F32)).astype(F32)


def clamp(t, lo, hi):
    return fmin(fmax(t, lo), hi)


def taps(u, v):
    """The sixteen tap coordinates (float32 planes) in the contract's order: [(i-1+k, j-1+l) for l for k]"""
    with np.errstate(all="ignore"):
        i, j = np.floor(u), np.floor(v)
        return [((i + F32(k - 1)).astype(F32), (j + F32(l - 1)).astype(F32)) for l in range(4) for k in range(4)]


def sample(source, S, u, v, limits=None):
    """The filter from the source coordinates on: S and the float32 planes u, v in one coordinate system, source the pixels over S
    (uint16 codes or float32) -> the same format.  `limits`, a dict, receives the float32 planes lo / hi (y, x, 4) of the clamp
    rule and `blended`, where the sixteen taps gave the pixel (not the copy rule, and A > 0)."""
    half = source.dtype == np.uint16
    wide = widen(source) if half else np.ascontiguousarray(source, F32)
    out = np.zeros(u.shape + (4,), source.dtype)
    inf = F32(np.inf)
    with np.errstate(all="ignore"):
        i, j = np.floor(u), np.floor(v)
        a, b = (u - i).astype(F32), (v - j).astype(F32)
        wx, wy = weights(a), weights(b)
        A = np.zeros(u.shape, F32)
        C = [np.zeros(u.shape, F32) for _ in range(3)]
        lo = np.full(u.shape + (4,), inf, F32)
        hi = np.full(u.shape + (4,), -inf, F32)
        for n, (ti, tj) in enumerate(taps(u, v)):
            k, l = n & 3, n >> 2
            ok = tm.inside(ti, tj, S)
            p = tm._fetch(wide, S, ti, tj, ok)
            counts = ok & (p[..., 3] > 0)
            q = ((wx[k] * wy[l]).astype(F32) * p[..., 3]).astype(F32)
            A = np.where(counts, (A + q).astype(F32), A)
            for ch in range(3):
                C[ch] = np.where(counts, (C[ch] + (q * p[..., ch]).astype(F32)).astype(F32), C[ch])
                lo[..., ch] = np.where(counts, fmin(lo[..., ch], p[..., ch]), lo[..., ch])
                hi[..., ch] = np.where(counts, fmax(hi[..., ch], p[..., ch]), hi[..., ch])
            ta = np.where(counts, p[..., 3], F32(0))
            lo[..., 3] = fmin(lo[..., 3], ta)
            hi[..., 3] = fmax(hi[..., 3], ta)
        solid = A > 0
        result = np.zeros(u.shape + (4,), F32)
        for ch in range(3):
            result[..., ch] = np.where(solid, clamp((C[ch] / A).astype(F32), lo[..., ch], hi[..., ch]), F32(0))
        result[..., 3] = np.where(solid, clamp(A, lo[..., 3], hi[..., 3]), F32(0))
        out[...] = f2h_rz_model(result) if half else result
        on_sample = (a == 0) & (b == 0)
        ok = tm.inside(i, j, S)
        copied = np.where(ok[..., None], tm._fetch(source, S, i, j, ok), np.zeros(4, source.dtype))
        out[on_sample] = copied[on_sample]
    if limits is not None:
        limits.update(lo=lo, hi=hi, blended=solid & ~on_sample)
    return out


def transform_plane(source, S, m, window, limits=None):
    return sample(source, S, *tm.source_coords(m, window), limits=limits)


def perspective_plane(source, S, p, window, limits=None):
    _h, _to, so = p
    rel = (S[0] - so[0], S[1] - so[1], S[2] - so[0], S[3] - so[1])
    u, v, w = pm.source_coords(p, window)
    out = sample(source, rel, u, v, limits=limits)
    with np.errstate(invalid="ignore"):
        out[~(w > 0)] = 0
    if limits is not None:
        with np.errstate(invalid="ignore"):
            limits["blended"] = limits["blended"] & (w > 0)
    return out


def transform_expected(before, target_full, source, source_full, source_cur, m):
    """The target buffer after the call and its window (None: empty), as tests/transform_model.py expected()"""
    out = before.copy()
    win = transform_target_window(m, source_cur, target_full)
    if win is None:
        return out, None
    crop(out, target_full, win)[...] = transform_plane(crop(source, source_full, source_cur), source_cur, m, win)
    return out, win


def perspective_expected(before, target_full, source, source_full, source_cur, p):
    out = before.copy()
    win = perspective_target_window(p, source_cur, target_full)
    if win is None or source_cur is None:
        return out, None
    crop(out, target_full, win)[...] = perspective_plane(crop(source, source_full, source_cur), source_cur, p, win)
    return out, win
