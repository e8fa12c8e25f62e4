"""numpy restatement of the MPEG-2 4:2:0 reconstruction contract (DESIGN.md "MPEG-2 4:2:0 reconstruction"; the reference has no
code for it).  Strict float32, one operation per statement, no fused multiply-add anywhere; the truncating float -> half
conversion and the Rec.709 -> linear (scene) half table are handed in (oracle.float_to_half, oracle.transfer_table(0))."""
import numpy as np

F = np.float32
# Y'CbCr -> R'G'B', row by row (video_reconstruct.c:55-59 and :62-66)
MATRICES = {"601": [[1.0, 0.0, 1.402], [1.0, -0.344136, -0.714136], [1.0, 1.772, 0.0]],
            "709": [[1.0, 0.0, 1.5748], [1.0, -0.187324, -0.468124], [1.0, 1.8556, 0.0]]}


def size_ok(width, height, interlaced=True):
    return width >= 2 and width % 2 == 0 and height >= 2 and height % 2 == 0 and (not interlaced or height % 4 == 0)


def decode_luma(y):
    return (y.astype(F) - F(16.0)) / F(219.0)


def decode_chroma(c):
    return (c.astype(F) - F(128.0)) / F(224.0)


def vertical_taps(height, interlaced=True):
    """Per luma row: (near plane row, far plane row, near weight, far weight)."""
    y = np.arange(height)
    if interlaced:
        f, l = y & 1, y >> 1
        j, odd = l >> 1, l & 1
        far = np.clip(np.where(odd == 1, j + 1, j - 1), 0, height // 4 - 1)
        outer = (f == odd)                                     # field 0 / l even and field 1 / l odd: 7/8 near
        wn = np.where(outer, F(7.0) / F(8.0), F(5.0) / F(8.0)).astype(F)
        wf = np.where(outer, F(1.0) / F(8.0), F(3.0) / F(8.0)).astype(F)
        return 2 * j + f, 2 * far + f, wn, wf
    c = y >> 1
    far = np.clip(np.where(y % 2 == 0, c - 1, c + 1), 0, height // 2 - 1)
    return c, far, np.full(height, F(0.75), F), np.full(height, F(0.25), F)


def vertical(plane, height, interlaced=True):
    """Decoded chroma (H/2, W/2) -> v per luma row (H, W/2): near * wn + far * wf, in that order."""
    near, far, wn, wf = vertical_taps(height, interlaced)
    with np.errstate(all="ignore"):
        a = plane[near] * wn[:, None]
        b = plane[far] * wf[:, None]
        return a + b


def horizontal(v):
    """v (H, W/2) -> h (H, W): even columns take v(k), odd columns (v(k) + v(k+1)) * 0.5 with k+1 clamped."""
    right = np.concatenate([v[:, 1:], v[:, -1:]], axis=1)
    h = np.empty((v.shape[0], 2 * v.shape[1]), F)
    h[:, 0::2] = v
    with np.errstate(all="ignore"):
        h[:, 1::2] = (v + right) * F(0.5)
    return h


def rgb(planes, width, height, interlaced=True, matrix="601"):
    """The f32 R'G'B' of the raster before truncation: planes [Y', Cb, Cr] (uint8, at least H x W, H/2 x W/2; padding ignored)."""
    assert size_ok(width, height, interlaced), (width, height, interlaced)
    yf = decode_luma(planes[0][:height, :width])
    cb, cr = (horizontal(vertical(decode_chroma(p[:height // 2, :width // 2]), height, interlaced)) for p in planes[1:])
    out = []
    with np.errstate(all="ignore"):
        for m0, m1, m2 in MATRICES[matrix]:
            a = yf * F(m0)
            b = cb * F(m1)
            c = cr * F(m2)
            out.append((a + b) + c)
    return out


def reconstruct_halves(planes, width, height, float_to_half, interlaced=True, matrix="601"):
    """(H, W, 4) half codes before the table: r, g, b truncated to half, alpha 1.0."""
    r, g, b = rgb(planes, width, height, interlaced, matrix)
    codes = np.empty((height, width, 4), np.uint16)
    for i, c in enumerate((r, g, b)):
        codes[..., i] = float_to_half(c)
    codes[..., 3] = float_to_half(np.array([1.0], F))[0]
    return codes


def reconstruct_model(planes, width, height, table, float_to_half, interlaced=True, matrix="601"):
    """The raster's pixels as the contract stores them: (H, W, 4) uint16 codes, all four through `table`."""
    return table[reconstruct_halves(planes, width, height, float_to_half, interlaced, matrix)]


def expected_frame(before, full, raster, width, height):
    """A frame buffer `before` (rows of the full window) after the call: pixels of full ∩ [0, W-1] x [0, H-1] replaced by the
    raster's, everything else kept.  Returns (frame, current window as (x0, y0, x1, y1), empty when x1 < x0)."""
    x0, y0 = max(full[0], 0), max(full[1], 0)
    x1, y1 = min(full[2], width - 1), min(full[3], height - 1)
    out = before.copy()
    if x0 > x1 or y0 > y1:
        return out, None
    out[y0 - full[1]:y1 - full[1] + 1, x0 - full[0]:x1 - full[0] + 1] = raster[y0:y1 + 1, x0:x1 + 1]
    return out, (x0, y0, x1, y1)
