"""numpy restatement of the field-conversion contract (DESIGN.md "Field conversions", include/canvas_hip.h; the reference has no
code for it).  Strict float32, one operation per statement, no fused multiply-add anywhere; the truncating float -> half
conversion is handed in (oracle.float_to_half).  Windows are (x0, y0, x1, y1) inclusive, None when empty; a frame is its half
codes over its full window, (H, W, 4) uint16, plus the two windows.  Row parity is that of the absolute coordinate (Python's
`y & 1` is two's complement for negative y, as the contract asks)."""
import numpy as np

F = np.float32


def widen(codes):
    """Half codes -> float32, exact for every code."""
    return np.ascontiguousarray(codes, np.uint16).view(np.float16).astype(F)


def intersect(a, b):
    if a is None or b is None:
        return None
    w = (max(a[0], b[0]), max(a[1], b[1]), min(a[2], b[2]), min(a[3], b[3]))
    return None if w[2] < w[0] or w[3] < w[1] else w


def bounding(a, b):
    """The bounding box of the windows that are not empty."""
    if a is None or b is None:
        return a if b is None else b
    return (min(a[0], b[0]), min(a[1], b[1]), max(a[2], b[2]), max(a[3], b[3]))


def crop(array, full, window):
    """The pixels of `window` (inside `full`) of a frame stored over `full`."""
    return array[window[1] - full[1]:window[3] - full[1] + 1, window[0] - full[0]:window[2] - full[0] + 1]


def field_to_frame(cur, y0, field, float_to_half):
    """cur: the pixels of the input's current window, first row at absolute row y0.  Returns every row of that window as the
    operation defines it: rows of parity `field` copied, the others made from the rows above and below that exist."""
    assert field in (0, 1)
    h = cur.shape[0]
    out = np.zeros_like(cur)
    for r in range(h):
        if ((y0 + r) & 1) == field:
            out[r] = cur[r]
            continue
        upper, lower = r - 1 >= 0, r + 1 < h
        if upper and lower:
            with np.errstate(all="ignore"):
                t = widen(cur[r - 1]) * F(0.5)
                u = widen(cur[r + 1]) * F(0.5)
                s = t + u
            out[r] = float_to_half(s)
        elif upper:
            out[r] = cur[r - 1]
        elif lower:
            out[r] = cur[r + 1]
    return out


def soften(cur, float_to_half):
    """Vertical [1/4, 1/2, 1/4] over the rows of the input's current window; a missing neighbour is the row itself."""
    b = widen(cur)
    a = np.concatenate([b[:1], b[:-1]], axis=0)
    c = np.concatenate([b[1:], b[-1:]], axis=0)
    with np.errstate(all="ignore"):
        t = a * F(0.25)
        p = b * F(0.5)
        t = t + p
        q = c * F(0.25)
        t = t + q
    return float_to_half(t)


def provided(frame, window):
    """The pixels of `window` as `frame` = (array, full, current) provides them: zero outside its current window."""
    array, full, current = frame
    out = np.zeros((window[3] - window[1] + 1, window[2] - window[0] + 1, 4), np.uint16)
    part = intersect(current, window)
    if part is not None:
        crop(out, window, part)[...] = crop(array, full, part)
    return out


def interlace(even, odd, window):
    """The pixels of `window`: even absolute rows from `even`, odd ones from `odd` (frames as for provided())."""
    e, o = provided(even, window), provided(odd, window)
    rows = (np.arange(window[1], window[3] + 1) & 1) == 1
    out = e.copy()
    out[rows] = o[rows]
    return out


def expected_one_input(before, out_full, in_frame, op):
    """The output buffer `before` (over out_full) after field_to_frame or soften: op(pixels of the input's current window, its
    first row) -> the same rows converted.  Returns (buffer, current window or None)."""
    array, full, current = in_frame
    window = intersect(out_full, current)
    after = before.copy()
    if window is None:
        return after, None
    whole = op(crop(array, full, current), current[1])
    crop(after, out_full, window)[...] = crop(whole, current, window)
    return after, window


def expected_interlace(before, out_full, even, odd):
    window = intersect(out_full, bounding(even[2], odd[2]))
    after = before.copy()
    if window is None:
        return after, None
    crop(after, out_full, window)[...] = interlace(even, odd, window)
    return after, window


# ---- 2:3 pulldown addition (cadence AA BB BC CD DD: first letter the even rows, second the odd rows)

_EVEN, _ODD, _SHIFT = (0, 1, 1, 2, 3), (0, 1, 2, 3, 3), (0, 1, 2, 3, 3)


def pulldown23_add(offset, i):
    """(even source frame, odd source frame) of output frame i."""
    k, r = divmod(i + offset, 5)
    return 4 * k + _EVEN[r] - _SHIFT[offset], 4 * k + _ODD[r] - _SHIFT[offset]
