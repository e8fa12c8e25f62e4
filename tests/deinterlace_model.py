"""numpy restatement of the motion-adaptive deinterlace contract (DESIGN.md "Adaptive deinterlace", include/canvas_deinterlace.h; the
reference has no code for it).  Strict float32, one operation per statement, no fused multiply-add anywhere; the truncating
float -> half conversion is handed in (oracle.float_to_half).  Windows, frames and row parity as in tests/fields_model.py: a window
is (x0, y0, x1, y1) inclusive or None, a frame is (half codes over its full window, full window, current window)."""
import numpy as np

from tests import fields_model as fm

F = np.float32
NONE = F(-1.0)                      # "no sample counts": below every difference


def present(frame):
    return frame is not None and frame[2] is not None


def differences(cur, neighbours):
    """D over cur's current window, (H, W) float32: per pixel the largest |cur - n| over the four channels and the present
    neighbours whose current window holds the pixel, a NaN difference counted as +inf; NONE where no neighbour holds it."""
    array, full, cw = cur
    c = fm.widen(fm.crop(array, full, cw))
    d = np.full(c.shape[:2], NONE, F)
    for n in neighbours:
        if not present(n):
            continue
        v = fm.intersect(cw, n[2])
        if v is None:
            continue
        with np.errstate(all="ignore"):
            e = fm.crop(c, cw, v) - fm.widen(fm.crop(n[0], n[1], v))
        e = np.abs(e)
        e = np.where(np.isnan(e), F(np.inf), e).max(axis=-1)
        part = fm.crop(d, cw, v)
        part[...] = np.maximum(part, e)
    return d


def neighbourhood(d):
    """m: the largest D of the 3 x 3 pixels around each pixel, those outside the array not counting."""
    h, w = d.shape
    padded = np.full((h + 2, w + 2), NONE, F)
    padded[1:-1, 1:-1] = d
    m = d.copy()
    for dy in range(3):
        for dx in range(3):
            m = np.maximum(m, padded[dy:dy + h, dx:dx + w])
    return m


def ramp(t):
    return np.where(t < F(1.0), np.where(t > F(0.0), t, F(0.0)), F(1.0)).astype(F)


def weights(m, threshold, softness):
    """k per pixel, float32: 1 where nothing counts, else the ramp (softness > 0) or the hard switch."""
    threshold, softness = F(threshold), F(softness)
    with np.errstate(all="ignore"):
        if softness > 0:
            inv_soft = F(1.0) / softness
            past = m - threshold
            t = past * inv_soft
            k = ramp(t)
        else:
            k = np.where(m <= threshold, F(0.0), F(1.0)).astype(F)
    return np.where(m < 0, F(1.0), k).astype(F)


def adaptive(cur, prev, nxt, field, threshold, softness, float_to_half):
    """Every row of cur's current window as the operation defines it: (codes (H, W, 4), k (H, W) float32 with NaN on the kept
    rows, copied (H, W) bool: the pixel's codes are copies of input codes, to be compared code for code)."""
    assert field in (0, 1)
    array, full, cw = cur
    c = np.ascontiguousarray(fm.crop(array, full, cw))
    h = c.shape[0]
    k = weights(neighbourhood(differences(cur, [prev, nxt])), threshold, softness)
    rows = np.arange(h)
    kept = ((cw[1] + rows) & 1) == field
    has_up, has_dn = rows >= 1, rows <= h - 2
    both = (has_up & has_dn)[:, None, None]
    up = np.concatenate([c[:1], c[:-1]], axis=0)                   # (row 0 and the last row: never used)
    dn = np.concatenate([c[1:], c[-1:]], axis=0)
    with np.errstate(all="ignore"):
        t = fm.widen(up) * F(0.5)
        u = fm.widen(dn) * F(0.5)
        mean = t + u
        one = np.where(has_up[:, None, None], up, np.where(has_dn[:, None, None], dn, np.uint16(0)))
        sp_codes = np.where(both, float_to_half(mean), one)
        sp = np.where(both, mean, fm.widen(one))
        wv = fm.widen(c)
        kr = k[:, :, None]
        e = sp - wv
        f = kr * e
        s = wv + f
    made = np.where(kr == 0, c, np.where(kr == 1, sp_codes, float_to_half(s)))
    out = np.where(kept[:, None, None], c, made).astype(np.uint16)
    copied = kept[:, None] | (k == 0) | ((k == 1) & ~both[:, :, 0])
    return out, np.where(kept[:, None], F(np.nan), k).astype(F), copied


def expected(before, out_full, cur, prev, nxt, field, threshold, softness, float_to_half):
    """The output buffer `before` (over out_full) after the call: (buffer, current window or None, mask over the buffer of the
    pixels to compare code for code: everything outside the window and every copy inside it, k over the window or None)."""
    after = before.copy()
    exact = np.ones(before.shape[:2], bool)
    window = fm.intersect(out_full, cur[2])
    if window is None:
        return after, None, exact, None
    whole, k, copied = adaptive(cur, prev, nxt, field, threshold, softness, float_to_half)
    fm.crop(after, out_full, window)[...] = fm.crop(whole, cur[2], window)
    fm.crop(exact, out_full, window)[...] = fm.crop(copied, cur[2], window)
    return after, window, exact, fm.crop(k, cur[2], window)


def classes(k):
    """The shares of the made pixels with k == 0, 0 < k < 1 and k == 1."""
    made = k[~np.isnan(k)]
    if made.size == 0:
        return 0.0, 0.0, 0.0
    return float((made == 0).mean()), float(((made > 0) & (made < 1)).mean()), float((made == 1).mean())


# tests/test_fields_gpu.py's special halfs; the finite ones among them (a difference that involves one of the others is +inf or NaN)
SPECIALS = np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x03FF, 0x83FF, 0x0400, 0x7BFF, 0xFBFF, 0x7C00, 0xFC00,
                     0x7E00, 0xFE00, 0x7C01, 0x7DFF, 0xFC01, 0x7FFF, 0xFFFF, 0x3C00, 0xBC00], np.uint16)
FINITE_SPECIALS = SPECIALS[(SPECIALS & 0x7C00) != 0x7C00]


def _sprinkle(rng, codes, specials):
    """tests/test_fields_gpu.py's band and scatter: three rows of special halfs a third of the way down (so that specials meet
    specials vertically) and a scatter of 2 % elsewhere."""
    if codes.size == 0:
        return
    top = codes.shape[0] // 3
    band = codes[top:top + 3]
    band[...] = specials[rng.integers(0, len(specials), band.shape)]
    scatter = rng.uniform(size=codes.shape) < 0.02
    codes[scatter] = specials[rng.integers(0, len(specials), int(scatter.sum()))]


def thirds(rng, full, threshold=0.05, softness=0.1, specials=True):
    """Three frames (prev, cur, next) of half codes over `full`, built in thirds by column so that every class of k is met: a
    third where both neighbours equal cur, a third where a neighbour is cur plus a perturbation uniform in
    +-(threshold + 0.8 * softness), a third of unrelated noise.  With `specials` the frames carry the band and scatter of special
    halfs: all of them, placed in each frame on its own, in the noise third; in the other two thirds only the finite ones, put
    into cur before the neighbours are derived from it -- an infinity or a NaN makes m = +inf and k = 1 in the 3 x 3 pixels around
    it whatever the neighbour holds, and the band alone would take the classes k < 1 out of a picture of nine rows."""
    h, w = full[3] - full[1] + 1, full[2] - full[0] + 1
    a, b = w // 3, w - w // 3
    cur = rng.uniform(0.0, 1.0, (h, w, 4)).astype(np.float16)
    if specials:
        _sprinkle(rng, cur.view(np.uint16)[:, :b], FINITE_SPECIALS)
    prev, nxt = cur.copy(), cur.copy()
    reach = threshold + 0.8 * softness
    which = rng.integers(0, 2, (h, b - a, 1)).astype(bool)
    with np.errstate(all="ignore"):
        bump = (cur[:, a:b].astype(np.float32) + rng.uniform(-reach, reach, (h, b - a, 4)).astype(np.float32)).astype(np.float16)
    prev[:, a:b] = np.where(which, bump, cur[:, a:b])
    nxt[:, a:b] = np.where(which, cur[:, a:b], bump)
    prev[:, b:] = rng.uniform(0.0, 1.0, (h, w - b, 4)).astype(np.float16)
    nxt[:, b:] = rng.uniform(0.0, 1.0, (h, w - b, 4)).astype(np.float16)
    frames = [f.view(np.uint16).copy() for f in (prev, cur, nxt)]
    if specials:
        for f in frames:
            _sprinkle(rng, f[:, b:], SPECIALS)
    return frames
