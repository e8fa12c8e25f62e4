"""Numpy statement of the median's contract (DESIGN.md "Median", include/canvas_median.h), independent of the kernel and of
host/median.c.  Pixels are BIT PATTERNS throughout: uint16 arrays for half frames, uint32 arrays for f32 frames (the tests view
an f32 buffer as uint32), shape (h, w, 4), channels r, g, b, a.

    key(c)  = c has its sign bit ? ~c : c | sign bit           compared unsigned: -NaN < -inf < .. < -0 < +0 < .. < +inf < +NaN
    med[ch] = the middle of the sorted keys of the n * n samples source(clamp(x + dx), clamp(y + dy)), clamped to the source's
              current window (np.pad mode="edge"), turned back into its code
    threshold == 0: the selected channels take med
    threshold > 0:  d = max over the selected channels of fabsf(s - med), one f32 subtraction (halfs widened exactly);
                    !(d <= threshold): the selected channels take med; else the pixel keeps the source's codes whole
A channel that is not selected keeps the source's code.  Nothing is rounded: the tests compare raw bytes."""
import numpy as np

from tests.unsharp_model import crop, intersect  # noqa: F401  (re-exported for the tests)

F32 = np.float32
LETTERS = "rgba"
ALL, COLOUR, ALPHA = 15, 7, 8
THRESHOLD = 0.0625
# signalling and quiet NaNs of both signs, subnormals, both zeros, the largest half, the infinities
SPECIALS16 = np.array([0x7C01, 0xFC01, 0x7DFF, 0x7E00, 0xFE00, 0x7FFF, 0xFFFF, 0x0001, 0x8001, 0x03FF, 0x83FF, 0x0000, 0x8000,
                       0x7BFF, 0xFBFF, 0x7C00, 0xFC00], np.uint16)
SPECIALS32 = np.array([0x7F800001, 0xFF800001, 0x7FBFFFFF, 0x7FC00000, 0xFFC00000, 0x7FFFFFFF, 0xFFFFFFFF, 0x00000001, 0x80000001,
                       0x007FFFFF, 0x807FFFFF, 0x00000000, 0x80000000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000], np.uint32)


def mask_of(channels):
    """'rgba' letters or a CVS_MEDIAN_* mask -> the mask"""
    if isinstance(channels, str):
        return sum(1 << LETTERS.index(c) for c in channels)
    return int(channels)


def _sign(dtype):
    return dtype.type(1 << (dtype.itemsize * 8 - 1))


def key(codes):
    codes = np.asarray(codes)
    assert codes.dtype in (np.uint16, np.uint32)
    sign = _sign(codes.dtype)
    return np.where(codes & sign != 0, ~codes, codes | sign).astype(codes.dtype)


def unkey(keys):
    keys = np.asarray(keys)
    sign = _sign(keys.dtype)
    return np.where(keys & sign != 0, keys & ~sign, ~keys).astype(keys.dtype)


def widen(codes):
    """bit patterns -> the f32 values they stand for (a half widened exactly)"""
    codes = np.ascontiguousarray(codes)
    return codes.view(np.float16).astype(F32) if codes.dtype == np.uint16 else codes.view(F32)


def medians(pixels, radius, channels=ALL):
    """med of every pixel of `pixels`, the source over its CURRENT window, edges replicated; the channels that are not selected
    (and so never used) come back as the source's"""
    n = 2 * radius + 1
    h, w = pixels.shape[:2]
    sel = [c for c in range(4) if mask_of(channels) >> c & 1]
    padded = np.pad(key(pixels[..., sel]), ((radius, radius), (radius, radius), (0, 0)), mode="edge")
    shifts = np.stack([padded[dy:dy + h, dx:dx + w] for dy in range(n) for dx in range(n)])
    out = pixels.copy()
    out[..., sel] = unkey(np.partition(shifts, (n * n) // 2, axis=0)[(n * n) // 2])
    return out


def replaced(pixels, radius, threshold, channels=ALL):
    """(h, w) bool: the pixels whose selected channels take the median"""
    if not threshold > 0:
        return np.ones(pixels.shape[:2], bool)
    sel = [c for c in range(4) if mask_of(channels) >> c & 1]
    with np.errstate(all="ignore"):
        d = np.abs((widen(pixels)[..., sel] - widen(medians(pixels, radius, channels))[..., sel]).astype(F32))
        return (~(d <= F32(threshold))).any(axis=-1)


def filter_pixels(pixels, radius, threshold=0.0, channels=ALL):
    """The source over its current window -> the filtered pixels over the same window."""
    out = pixels.copy()
    med, take = medians(pixels, radius, channels), replaced(pixels, radius, threshold, channels)
    for c in range(4):
        if mask_of(channels) >> c & 1:
            out[..., c] = np.where(take, med[..., c], pixels[..., c])
    return out


def expected(before, tfull, pixels, sfull, scur, radius, threshold=0.0, channels=ALL):
    """The target buffer after the call and its window.  before: the target's pixels beforehand; pixels: the source over
    sfull; scur its current window (None: empty).  Pixels outside the window keep what `before` held."""
    out = before.copy()
    win = None if scur is None else intersect(scur, tfull)
    if win is None:
        return out, None
    made = filter_pixels(crop(pixels, sfull, scur), radius, threshold, channels)
    crop(out, tfull, win)[...] = crop(made, scur, win)
    return out, win


def filter_tiled(tile, height, radius, threshold=0.0, channels=ALL):
    """filter_pixels of the picture made of `tile` repeated down to `height` rows, for pictures too tall to model row by row in
    a test's time.  The filter is local: a row's result depends on the 2 * radius + 1 rows around it alone, so away from the
    picture's first and last rows the result repeats with the tile, and the rows near the two ends are modelled as they are."""
    period = tile.shape[0]
    assert period > 2 * radius and height >= 4 * period
    three = filter_pixels(np.concatenate([tile, tile, tile]), radius, threshold, channels)[period:2 * period]
    out = np.tile(three, (-(-height // period), 1, 1))[:height]
    picture_top = np.concatenate([tile, tile])
    out[:period] = filter_pixels(picture_top, radius, threshold, channels)[:period]
    rows = np.arange(height - 2 * period, height) % period
    out[height - period:] = filter_pixels(tile[rows], radius, threshold, channels)[period:]
    return out


def brute(pixels, radius, threshold=0.0, channels=ALL):
    """filter_pixels by a loop over pixels and python's own sort, for tests/test_median_cpu.py"""
    h, w = pixels.shape[:2]
    sign = int(_sign(pixels.dtype))
    full = (1 << pixels.dtype.itemsize * 8) - 1
    k = lambda c: (~c & full) if c & sign else c | sign
    out = pixels.copy()
    sel = [c for c in range(4) if mask_of(channels) >> c & 1]
    for y in range(h):
        for x in range(w):
            med = {}
            for c in sel:
                near = [int(pixels[min(max(y + dy, 0), h - 1), min(max(x + dx, 0), w - 1), c]) for dy in range(-radius, radius + 1) for dx in range(-radius, radius + 1)]
                med[c] = sorted(near, key=k)[len(near) // 2]
            take = True
            if threshold > 0:
                with np.errstate(all="ignore"):
                    ds = [np.abs(F32(widen(pixels[y, x, c:c + 1])[0] - widen(np.array([med[c]], pixels.dtype))[0])) for c in sel]
                take = any(not d <= F32(threshold) for d in ds)
            if take:
                for c in sel:
                    out[y, x, c] = med[c]
    return out


def speck_picture(rng, width, height, dtype=np.uint16, specials=True):
    """The test picture as bit patterns: a ramp per channel with +-0.01 noise; 15 % of the pixels are specks, in each of which
    each channel has a 0.6 chance of taking one of 0, 1, 4, -0.5; a scatter of SPECIALS; one flat block, ties everywhere."""
    yy, xx = np.mgrid[0:height, 0:width].astype(np.float64)
    fx, fy = xx / max(width, 1), yy / max(height, 1)
    pic = np.stack([0.2 + 0.5 * fx + 0.1 * fy, 0.7 - 0.3 * fx + 0.2 * fy, 0.3 + 0.2 * fx + 0.4 * fy, 0.9 - 0.2 * fx - 0.3 * fy], -1)
    pic += rng.uniform(-0.01, 0.01, pic.shape)
    speck = (rng.uniform(size=(height, width)) < 0.15)[..., None] & (rng.uniform(size=pic.shape) < 0.6)
    pic[speck] = np.array([0.0, 1.0, 4.0, -0.5])[rng.integers(0, 4, int(speck.sum()))]
    by, bx, bh, bw = height // 2, width // 3, height // 3 + 1, width // 4 + 1
    pic[by:by + bh, bx:bx + bw] = [0.5, 0.25, 0.75, 1.0]
    if dtype == np.uint16:
        codes = pic.astype(np.float16).view(np.uint16)
        table = SPECIALS16
    else:
        codes = np.ascontiguousarray(pic.astype(F32)).view(np.uint32)
        table = SPECIALS32
    if specials:
        hit = rng.uniform(size=codes.shape) < 0.01
        codes[hit] = table[rng.integers(0, len(table), int(hit.sum()))]
    return codes


def classes(pixels, radius, threshold=THRESHOLD, channels=ALL):
    """(fraction kept, fraction replaced) of the pixels"""
    take = replaced(pixels, radius, threshold, channels)
    return float(1.0 - take.mean()), float(take.mean())
