"""numpy restatement of the temporal denoise contract (DESIGN.md "Temporal denoise", include/canvas_temporal.h; the reference has no
code for it).  Strict float32, one operation per statement, no fused multiply-add anywhere; the truncating float -> half
conversion is handed in (oracle.float_to_half).  Windows and frames as in tests/deinterlace_model.py: a window is
(x0, y0, x1, y1) inclusive or None, a frame is (half codes over its full window, full window, current window) or None.
Neighbours are always handed in as the list [prev1, next1, prev2, next2]: the contract's order of summation."""
import numpy as np

from tests import deinterlace_model as dm
from tests import fields_model as fm

F = np.float32
NONE = dm.NONE
ORDER = ("prev1", "next1", "prev2", "next2")
NEAR = {2: 0, 3: 1}                          # the nearer frame on a far frame's side, as indices into ORDER
R, G, B, A, ALL = 1, 2, 4, 8, 15


def present(frame):
    return frame is not None and frame[2] is not None


def _selected(channels):
    assert 0 < channels <= ALL
    return [c for c in range(4) if channels & (1 << c)]


def motion(cur, n, channels):
    """D over cur's current window, (H, W) float32: per pixel the largest |cur - n| over the selected channels where n's
    current window holds the pixel, a NaN difference counted as +inf; NONE elsewhere."""
    array, full, cw = cur
    sel = _selected(channels)
    d = np.full((cw[3] - cw[1] + 1, cw[2] - cw[0] + 1), NONE, F)
    v = fm.intersect(cw, n[2])
    if v is None:
        return d
    with np.errstate(all="ignore"):
        e = fm.widen(fm.crop(array, full, v)[..., sel]) - fm.widen(fm.crop(n[0], n[1], v)[..., sel])
    e = np.abs(e)
    fm.crop(d, cw, v)[...] = np.where(np.isnan(e), F(np.inf), e).max(axis=-1)
    return d


def raw_weight(cur, n, threshold, softness, channels):
    """v_n over cur's current window, float32"""
    cw = cur[2]
    shape = (cw[3] - cw[1] + 1, cw[2] - cw[0] + 1)
    if not present(n) or fm.intersect(cw, n[2]) is None:
        return np.zeros(shape, F)
    m = dm.neighbourhood(motion(cur, n, channels))
    threshold, softness = F(threshold), F(softness)
    with np.errstate(all="ignore"):
        if softness > 0:
            inv_soft = F(1.0) / softness
            past = m - threshold
            t = past * inv_soft
            v = F(1.0) - dm.ramp(t)
        else:
            v = np.where(m <= threshold, F(1.0), F(0.0)).astype(F)
    inside = np.zeros(shape, bool)
    fm.crop(inside, cw, fm.intersect(cw, n[2]))[...] = True
    return np.where(inside & (m >= 0), v, F(0.0)).astype(F)


def weights(cur, neighbours, threshold, softness, channels, chain=True):
    """([w_prev1, w_next1, w_prev2, w_next2], [v_...]) over cur's current window; chain=False leaves the chain rule out (what a
    wrong implementation would do: the tests' teeth)."""
    assert len(neighbours) == 4
    v = [raw_weight(cur, n, threshold, softness, channels) for n in neighbours]
    w = list(v)
    if chain:
        for far, near in NEAR.items():
            w[far] = np.minimum(v[far], w[near])
    return w, v


def denoise(cur, neighbours, threshold, softness, channels, float_to_half):
    """Every pixel of cur's current window as the operation defines it: (codes (H, W, 4), [w_n] float32 (H, W), copied (H, W, 4)
    bool: the code is a copy of cur's, to be compared code for code)."""
    array, full, cw = cur
    c = np.ascontiguousarray(fm.crop(array, full, cw))
    w, _ = weights(cur, neighbours, threshold, softness, channels)
    acc = fm.widen(c)
    total = np.ones(c.shape[:2], F)
    for n, wn in zip(neighbours, w):
        if not wn.any():
            continue
        v = fm.intersect(cw, n[2])
        pixels = np.zeros(c.shape, F)
        fm.crop(pixels, cw, v)[...] = fm.widen(fm.crop(n[0], n[1], v))
        with np.errstate(all="ignore"):
            t = wn[:, :, None] * pixels
            s = acc + t
            ws = total + wn
        acc = np.where((wn > 0)[:, :, None], s, acc)
        total = np.where(wn > 0, ws, total)
    with np.errstate(all="ignore"):
        inv = F(1.0) / total
        o = acc * inv[:, :, None]
    touched = np.zeros(c.shape[:2], bool)
    for wn in w:
        touched |= wn > 0
    made = touched[:, :, None] & np.array([bool(channels & (1 << k)) for k in range(4)])[None, None, :]
    out = np.where(made, float_to_half(o.astype(F)), c).astype(np.uint16)
    return out, w, ~made


def expected(before, out_full, cur, neighbours, threshold, softness, channels, float_to_half):
    """The output buffer `before` (over out_full) after the call: (buffer, current window or None, mask over the buffer's codes
    of those to compare code for code: everything outside the window and every copy inside it, [w_n] over the window or None)."""
    after = before.copy()
    exact = np.ones(before.shape, bool)
    window = fm.intersect(out_full, cur[2])
    if window is None:
        return after, None, exact, None
    whole, w, copied = denoise(cur, neighbours, threshold, softness, channels, float_to_half)
    fm.crop(after, out_full, window)[...] = fm.crop(whole, cur[2], window)
    fm.crop(exact, out_full, window)[...] = fm.crop(copied, cur[2], window)
    return after, window, exact, [fm.crop(wn, cur[2], window) for wn in w]


def classes(w):
    """The shares of the pixels with w == 0, 0 < w < 1 and w == 1."""
    if w.size == 0:
        return 0.0, 0.0, 0.0
    return float((w == 0).mean()), float(((w > 0) & (w < 1)).mean()), float((w == 1).mean())


def sequence(rng, full, threshold=0.05, softness=0.1, specials=True):
    """Five frames [prev2, prev1, cur, next1, next2] of half codes over `full`, built in thirds by column so that every class of
    every neighbour's weight is met: a static third, where each neighbour is cur plus noise of at most threshold / 4; a third
    that straddles the ramp, where each neighbour is cur plus a perturbation whose size, drawn per neighbour and column, spreads
    the differences over threshold +- softness (from threshold + 0.1 * softness to threshold + 0.8 * softness, so that the far
    frames' raw weights fall on both sides of the near frames': the chain rule bites); a third of unrelated noise.  With
    `specials` the frames carry tests/deinterlace_model.py's band and scatter of special halfs: all of them, placed in each frame
    on its own, in the noise third -- an infinity or a NaN forces weight 0 in the 3 x 3 pixels around it -- and in the other two
    thirds only the finite ones, put into cur before the neighbours are derived from it."""
    h, w = full[3] - full[1] + 1, full[2] - full[0] + 1
    a, b = w // 3, w - w // 3
    cur = rng.uniform(0.0, 1.0, (h, w, 4)).astype(np.float16)
    if specials:
        dm._sprinkle(rng, cur.view(np.uint16)[:, :b], dm.FINITE_SPECIALS)
    frames = []
    for _ in range(4):
        f = cur.copy()
        with np.errstate(all="ignore"):
            c32 = cur.astype(np.float32)
            f[:, :a] = (c32[:, :a] + rng.uniform(-threshold / 4, threshold / 4, (h, a, 4)).astype(np.float32)).astype(np.float16)
            reach = threshold + softness * rng.uniform(0.1, 0.8, (1, b - a, 1))
            f[:, a:b] = (c32[:, a:b] + (reach * rng.uniform(-1.0, 1.0, (h, b - a, 4))).astype(np.float32)).astype(np.float16)
        f[:, b:] = rng.uniform(0.0, 1.0, (h, w - b, 4)).astype(np.float16)
        frames.append(f)
    frames = [f.view(np.uint16).copy() for f in (frames[2], frames[0], cur, frames[1], frames[3])]
    if specials:
        for f in frames:
            dm._sprinkle(rng, f[:, b:], dm.SPECIALS)
    return frames
