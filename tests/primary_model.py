"""Numpy statement of the primary colour corrector's contract (DESIGN.md "Primary colour correction"; include/canvas_primary.h),
independent of the kernel and of host/primary.c.

Every intermediate is cast to float32, so every operation is rounded on its own, the same in both arithmetic flavours:

    scale[c] = (float)(K-1) / (domain_max[c] - domain_min[c])
    curve(T, c, s):  t = (s - domain_min[c]) * scale[c]
                     t = (t > 0) ? ((t < (float)(K-1)) ? t : (float)(K-1)) : 0       NaN -> 0, -Inf -> 0, +Inf -> K-1
                     i = min((int)t, K-2) ;  f = t - (float)i
                     return T[c][i] * (1 - f) + T[c][i+1] * f
    v = s.rgb ;  pre: v.c = curve(pre, c, v.c) ;  matrix: v.c = ((m[4c]*v.r + m[4c+1]*v.g) + m[4c+2]*v.b) + m[4c+3], from the three
    values before the stage ;  post: v.c = curve(post, c, v.c) ;  out.rgb = v ;  out.a = s.a, code for code

A curve set here is Curves(table, domain): table a (K, 3) float32 array, one row of (r, g, b) per node, the order of a 1D .cube.
An f16 source is widened exactly (tests/unsharp_model.py widen); f16 results are truncated once, by tests/models.py f2h_rz_model,
and their alpha is the source's code."""
import numpy as np

from tests.models import f2h_rz_model
from tests.unsharp_model import crop, intersect, widen  # noqa: F401  (re-exported for the tests)

F32 = np.float32
UNIT = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
# Two sets of domains that differ per channel.  SKEWED: a negative start, a wide one, and one of width 2^-10 whose start is no half
# code.  WIDE: none starts or ends where another does.  No width but the narrow one is a power of two, and that one starts off
# the halfs' grid: a domain with dyadic ends puts most half codes exactly on the nodes of a table of 2^n + 1 nodes, and the test
# picture is to fall mostly inside cells (classes() below).
SKEWED = ((-0.25, 0.0, float(F32(0.1))), (1.0, 1.5, float(F32(0.1)) + 2.0 ** -10))
WIDE = ((0.0, -0.5, float(F32(0.05))), (float(F32(1.1)), float(F32(0.9)), float(F32(1.3))))
SPECIALS16 = np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x03FF, 0x83FF, 0x0400, 0x7BFF, 0xFBFF, 0x7C00, 0xFC00,
                       0x7E00, 0xFE00, 0x7C01, 0x7DFF, 0xFC01, 0x7FFF, 0xFFFF, 0x3C00, 0xBC00], np.uint16)
SPECIALS32 = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x00800000, 0x477FE000, 0xC77FE000, 0x7F7FFFFF, 0xFF7FFFFF,
                       0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FBFFFFF, 0xFF800001, 0x7FFFFFFF, 0x3F800000, 0xBF800000], np.uint32)


class Curves:
    def __init__(self, table, domain=UNIT):
        self.table = np.ascontiguousarray(np.asarray(table, F32).reshape(-1, 3))
        self.size = self.table.shape[0]
        self.domain = (tuple(float(v) for v in domain[0]), tuple(float(v) for v in domain[1]))

    def planar(self):
        """the device form: K floats of R, K of G, K of B"""
        return np.ascontiguousarray(self.table.T).reshape(-1)


def identity(size, domain=UNIT):
    """node i of channel c holds domain_min + i * (domain_max - domain_min) / (K-1), in float64, rounded once"""
    steps = [np.float64(domain[0][c]) + np.arange(size, dtype=np.float64) * (np.float64(domain[1][c]) - np.float64(domain[0][c])) / (size - 1) for c in range(3)]
    return Curves(np.stack(steps, axis=1).astype(F32), domain)


def distinct(size, domain=UNIT, seed=0):
    """curves whose every node of every channel holds a value no other holds, in -0.5 .. 1.5: a wrong node or channel shows"""
    rng = np.random.default_rng(seed + 7 * size)
    values = np.arange(size * 3, dtype=np.float64) / (size * 3) * 2.0 - 0.5
    return Curves(rng.permutation(values).reshape(size, 3), domain)


def scale_of(size, domain):
    return [F32(F32(size - 1) / F32(F32(domain[1][c]) - F32(domain[0][c]))) for c in range(3)]


def position(s, size, domain):
    """(..., 3) f32 colours -> (i: int32, f: float32, t before the clamp: float32), each (..., 3)"""
    s = np.ascontiguousarray(s, F32)
    scale, top = scale_of(size, domain), F32(size - 1)
    i, f, raw = np.empty(s.shape, np.int32), np.empty(s.shape, F32), np.empty(s.shape, F32)
    with np.errstate(all="ignore"):
        for c in range(3):
            t = ((s[..., c] - F32(domain[0][c])).astype(F32) * scale[c]).astype(F32)
            raw[..., c] = t
            t = np.where(t > 0, np.where(t < top, t, top), F32(0)).astype(F32)
            i[..., c] = np.minimum(np.trunc(t).astype(np.int32), size - 2)
            f[..., c] = (t - i[..., c].astype(F32)).astype(F32)
    return i, f, raw


def curve(cv, v):
    """(..., 3) f32 -> (..., 3) f32 through the three curves"""
    i, f, _ = position(v, cv.size, cv.domain)
    out = np.empty(v.shape, F32)
    with np.errstate(all="ignore"):
        for c in range(3):
            a, b = cv.table[i[..., c], c], cv.table[i[..., c] + 1, c]
            g = (F32(1) - f[..., c]).astype(F32)
            out[..., c] = ((a * g).astype(F32) + (b * f[..., c]).astype(F32)).astype(F32)
    return out


def matrix_stage(m, v):
    m = np.asarray(m, F32).reshape(3, 4)
    out = np.empty(v.shape, F32)
    with np.errstate(all="ignore"):
        for c in range(3):
            acc = ((m[c, 0] * v[..., 0]).astype(F32) + (m[c, 1] * v[..., 1]).astype(F32)).astype(F32)
            acc = (acc + (m[c, 2] * v[..., 2]).astype(F32)).astype(F32)
            out[..., c] = (acc + m[c, 3]).astype(F32)
    return out


def apply_f32(s, pre=None, matrix=None, post=None):
    """(..., 4) f32 pixels -> the graded pixels, f32; alpha is the source's, bit for bit"""
    s = np.ascontiguousarray(s, F32)
    v = s[..., :3].copy()
    if pre is not None:
        v = curve(pre, v)
    if matrix is not None:
        v = matrix_stage(matrix, v)
    if post is not None:
        v = curve(post, v)
    out = s.copy()
    out[..., :3] = v
    return out


def apply_pixels(pixels, pre=None, matrix=None, post=None):
    """Pixels in either format (uint16 codes or f32) -> graded pixels in the same format."""
    if pixels.dtype != np.uint16:
        return apply_f32(pixels, pre, matrix, post)
    out = f2h_rz_model(apply_f32(widen(pixels), pre, matrix, post))
    out[..., 3] = pixels[..., 3]                                         # code for code, signalling NaNs included
    return out


def brute(pixels, pre=None, matrix=None, post=None):
    """apply_f32 as a loop over pixels and channels, scalar by scalar"""
    def one(cv, c, s):
        k = cv.size
        scale = F32(F32(k - 1) / F32(F32(cv.domain[1][c]) - F32(cv.domain[0][c])))
        with np.errstate(all="ignore"):
            t = F32(F32(s - F32(cv.domain[0][c])) * scale)
            t = (t if t < F32(k - 1) else F32(k - 1)) if t > 0 else F32(0)
            i = min(int(t), k - 2)
            f = F32(t - F32(i))
            return F32(F32(cv.table[i, c] * F32(F32(1) - f)) + F32(cv.table[i + 1, c] * f))
    out = np.array(pixels, F32)
    flat = out.reshape(-1, 4)
    for p in flat:
        v = [F32(p[0]), F32(p[1]), F32(p[2])]
        if pre is not None:
            v = [one(pre, c, v[c]) for c in range(3)]
        if matrix is not None:
            m = np.asarray(matrix, F32).reshape(3, 4)
            with np.errstate(all="ignore"):
                v = [F32(F32(F32(F32(m[c, 0] * v[0]) + F32(m[c, 1] * v[1])) + F32(m[c, 2] * v[2])) + m[c, 3]) for c in range(3)]
        if post is not None:
            v = [one(post, c, v[c]) for c in range(3)]
        p[:3] = v
    return out


def expected(before, target_full, source, source_full, source_cur, pre=None, matrix=None, post=None):
    """The target buffer after the call and its window.  before: the target's pixels beforehand (uint16 codes or f32);
    source: pixels over source_full in the same format.  Pixels outside the window keep what `before` held."""
    out = before.copy()
    win = None if source_cur is None else intersect(source_cur, target_full)
    if win is None:
        return out, None
    crop(out, target_full, win)[...] = apply_pixels(crop(source, source_full, win), pre, matrix, post)
    return out, win


def picture(rng, width=131, height=9, half=True, size=17, domain=UNIT):
    """The test picture for curves of `size` nodes on `domain` (the first stage the pixels meet), uint16 codes or float32:
    ramps from a tenth of the domain's width below it to a tenth above it, a different direction per channel, plus noise of
    +-0.01 of the width; then a scatter over the colour channels of values exactly on nodes (node 0 and node K-1 among them),
    values far below and above the domain, and the special codes of the format (both infinities, quiet and signalling NaNs, both
    zeros, subnormals, the largest finite half); the same special codes in alpha.  A picture of 40 pixels or more holds every
    special code in a colour channel and in alpha."""
    lo, hi = np.array(domain[0], np.float64), np.array(domain[1], np.float64)
    span = hi - lo
    n = width * height
    ramp = np.arange(n, dtype=np.float64).reshape(height, width) / max(n - 1, 1)
    ramps = np.stack([ramp, 1.0 - ramp, (ramp * 3.0) % 1.0], axis=-1)
    s = np.empty((height, width, 4), np.float64)
    s[..., :3] = lo + span * (ramps * 1.2 - 0.1 + rng.uniform(-0.01, 0.01, (height, width, 3)))
    s[..., 3] = rng.uniform(0.0, 1.0, (height, width))
    colour = s[..., :3]
    kind = rng.uniform(size=(height, width, 3))
    nodes = rng.integers(0, size, (height, width, 3))
    on_node = lo + nodes * span / (size - 1)
    colour[...] = np.where(kind < 0.09, on_node, colour)
    colour[...] = np.where(kind < 0.06, lo, colour)                      # node 0
    colour[...] = np.where(kind < 0.03, hi, colour)                      # node K-1
    colour[...] = np.where((kind >= 0.09) & (kind < 0.11), lo - span * rng.uniform(1.0, 100.0, (height, width, 3)), colour)
    colour[...] = np.where((kind >= 0.11) & (kind < 0.13), hi + span * rng.uniform(1.0, 100.0, (height, width, 3)), colour)
    special = rng.uniform(size=(height, width, 4)) < 0.05
    specials = SPECIALS16 if half else SPECIALS32
    out = f2h_rz_model(s.astype(F32)) if half else s.astype(F32).view(np.uint32)
    out[special] = specials[rng.integers(0, len(specials), int(special.sum()))]
    flat = out.reshape(-1, 4)
    if flat.shape[0] >= 2 * len(specials):                               # every special code once in a colour channel and once in alpha, whatever the draw
        at = np.arange(len(specials))
        flat[at, at % 3] = specials
        flat[len(specials) + at, 3] = specials
    return out if half else out.view(F32)


def classes(pixels, size, domain):
    """Shares of the picture's colour samples that fall (strictly inside a cell, clamped below, clamped above, exactly on a node
    of the domain): what tests/test_primary_cpu.py holds every test picture to."""
    s = widen(pixels) if pixels.dtype == np.uint16 else pixels
    _, f, raw = position(s[..., :3], size, domain)
    with np.errstate(invalid="ignore"):
        inside = (raw > 0) & (raw < F32(size - 1))
        within = inside & (f > 0) & (f < 1)
        below, above = raw < 0, raw > F32(size - 1)
        node = (raw >= 0) & (raw <= F32(size - 1)) & (raw == np.trunc(raw))
    return float(within.mean()), float(below.mean()), float(above.mean()), float(node.mean())
