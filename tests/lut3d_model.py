"""Numpy statement of the 3D LUT's contract (DESIGN.md "3D LUT"), independent of the kernel and of host/lut3d.c.

Every intermediate is cast to float32, so every operation is rounded on its own, the same in both arithmetic flavours:

    scale[c] = (float)(N-1) / (domain_max[c] - domain_min[c])
    for c in r, g, b:
        t   = (s.c - domain_min[c]) * scale[c]
        t   = (t > 0) ? ((t < (float)(N-1)) ? t : (float)(N-1)) : 0          NaN -> 0, -Inf -> 0, +Inf -> N-1
        i_c = min((int)t, N-2) ;  f_c = t - (float)i_c
    order the channels by descending f, a tie to r before g and g before b (a stable sort on (-f, channel))
    V0 = L[i] ; V1 = L[i + e1] ; V2 = L[i + e1 + e2] ; V3 = L[i + (1,1,1)]
    w0 = 1 - f1 ; w1 = f1 - f2 ; w2 = f2 - f3 ; w3 = f3
    out.c = ((V0.c*w0 + V1.c*w1) + V2.c*w2) + V3.c*w3 ;  out.a = s.a, code for code

The lattice is an (N, N, N, 3) float32 array indexed [ib, ig, ir] (red fastest when flattened: the .cube order).  `s` is the
source pixel; an f16 source is widened exactly (tests/unsharp_model.py widen); f16 results are truncated once, by tests/models.py
f2h_rz_model, and their alpha is the source's code."""
import numpy as np

from tests.models import f2h_rz_model
from tests.unsharp_model import crop, intersect, widen  # noqa: F401  (re-exported for the tests)

F32 = np.float32
UNIT = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))


def lattice(table, size):
    """N^3 * 3 numbers, red fastest -> (N, N, N, 3) float32 indexed [ib, ig, ir]"""
    return np.ascontiguousarray(np.asarray(table, F32).reshape(size, size, size, 3))


def identity(size, domain=UNIT):
    """the lattice whose node (ir, ig, ib) holds its own colour: domain_min + i * (domain_max - domain_min) / (N-1), in float64, rounded once"""
    steps = [np.asarray(domain[0][c], np.float64) + np.arange(size, dtype=np.float64) * (np.float64(domain[1][c]) - np.float64(domain[0][c])) / (size - 1) for c in range(3)]
    out = np.empty((size, size, size, 3), F32)
    out[..., 0] = steps[0][None, None, :]
    out[..., 1] = steps[1][None, :, None]
    out[..., 2] = steps[2][:, None, None]
    return out


def distinct(size, seed=0):
    """a lattice whose every node holds values no other node holds: a wrong vertex or a wrong order shows"""
    rng = np.random.default_rng(seed)
    values = (np.arange(size ** 3 * 3, dtype=np.float64) / (size ** 3 * 3) * 2.0 - 0.5)
    return lattice(rng.permutation(values), size)


def packed(lat):
    """(N, N, N, 3) -> the device form: N^3 nodes of (R, G, B, 0) as a flat float32 array"""
    n = lat.shape[0]
    out = np.zeros((n ** 3, 4), F32)
    out[:, :3] = lat.reshape(-1, 3)
    return out.reshape(-1)


def scale_of(size, domain):
    return [F32(F32(size - 1) / F32(F32(domain[1][c]) - F32(domain[0][c]))) for c in range(3)]


def cell(s, size, domain=UNIT):
    """(..., >=3) f32 colours -> (i: (..., 3) int32, f: (..., 3) float32) per channel r, g, b"""
    s = np.ascontiguousarray(s, F32)
    scale = scale_of(size, domain)
    top = F32(size - 1)
    i = np.empty(s.shape[:-1] + (3,), np.int32)
    f = np.empty(s.shape[:-1] + (3,), F32)
    with np.errstate(all="ignore"):
        for c in range(3):
            t = ((s[..., c] - F32(domain[0][c])).astype(F32) * scale[c]).astype(F32)
            t = np.where(t > 0, np.where(t < top, t, top), F32(0)).astype(F32)
            i[..., c] = np.minimum(np.trunc(t).astype(np.int32), size - 2)
            f[..., c] = (t - i[..., c].astype(F32)).astype(F32)
    return i, f


def vertices(i, f):
    """the four lattice indices (each (..., 3) as ir, ig, ib) and the four weights of every pixel"""
    order = np.argsort(-f, axis=-1, kind="stable")                       # channels by descending f, ties in channel order
    fs = np.take_along_axis(f, order, axis=-1)
    one = np.eye(3, dtype=np.int32)
    v0 = i
    v1 = v0 + one[order[..., 0]]
    v2 = v1 + one[order[..., 1]]
    v3 = i + 1
    w = [(F32(1) - fs[..., 0]).astype(F32), (fs[..., 0] - fs[..., 1]).astype(F32), (fs[..., 1] - fs[..., 2]).astype(F32), fs[..., 2]]
    return (v0, v1, v2, v3), w


def _fetch(lat, v):
    return lat[v[..., 2], v[..., 1], v[..., 0]]


def apply_f32(s, lat, domain=UNIT):
    """(..., 4) f32 pixels -> the graded pixels, f32; alpha is the source's, bit for bit"""
    s = np.ascontiguousarray(s, F32)
    lat = np.ascontiguousarray(lat, F32)
    i, f = cell(s, lat.shape[0], domain)
    v, w = vertices(i, f)
    q = [_fetch(lat, k) for k in v]
    out = s.copy()
    with np.errstate(all="ignore"):
        for c in range(3):
            acc = ((q[0][..., c] * w[0]).astype(F32) + (q[1][..., c] * w[1]).astype(F32)).astype(F32)
            acc = (acc + (q[2][..., c] * w[2]).astype(F32)).astype(F32)
            out[..., c] = (acc + (q[3][..., c] * w[3]).astype(F32)).astype(F32)
    return out


def apply_f64(s, lat, domain=UNIT):
    """The same tetrahedron evaluated in float64 (the cell and the order are the f32 model's, the weights and sums are not rounded
    to f32): what test_lut3d_cpu.py holds the model's error to."""
    s = np.ascontiguousarray(s, F32)
    i, f = cell(s, lat.shape[0], domain)
    v, _ = vertices(i, f)
    order = np.argsort(-f, axis=-1, kind="stable")
    fs = np.take_along_axis(f.astype(np.float64), order, axis=-1)
    w = [1.0 - fs[..., 0], fs[..., 0] - fs[..., 1], fs[..., 1] - fs[..., 2], fs[..., 2]]
    q = [_fetch(lat, k).astype(np.float64) for k in v]
    return sum(q[k] * w[k][..., None] for k in range(4))


def apply_pixels(pixels, lat, domain=UNIT):
    """Pixels in either format (uint16 codes or f32) -> graded pixels in the same format."""
    if pixels.dtype != np.uint16:
        return apply_f32(pixels, lat, domain)
    out = f2h_rz_model(apply_f32(widen(pixels), lat, domain))
    out[..., 3] = pixels[..., 3]                                         # code for code, signalling NaNs included
    return out


def expected(before, target_full, source, source_full, source_cur, lat, domain=UNIT):
    """The target buffer after the call and its window.  before: the target's pixels beforehand (uint16 codes or f32);
    source: pixels over source_full in the same format.  Pixels outside the window keep what `before` held."""
    out = before.copy()
    win = None if source_cur is None else intersect(source_cur, target_full)
    if win is None:
        return out, None
    crop(out, target_full, win)[...] = apply_pixels(crop(source, source_full, win), lat, domain)
    return out, win
