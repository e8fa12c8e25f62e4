"""numpy restatement of the MPEG-2 4:2:0 subsample contract (DESIGN.md "MPEG-2 4:2:0 subsample"; the reference states the
filter only as a shader, src/cprocess/video_subsample.c:189-526).  Strict float32, one operation per statement, no fused
multiply-add anywhere; the transfer table is handed in (oracle.transfer_table(2), the linear -> Rec.709 table)."""
import numpy as np

F = np.float32
LUMA_SCALE, LUMA_OFFSET = F(219.0) / F(255.0), F(16.0) / F(255.0)
CHROMA_SCALE, CHROMA_OFFSET = F(224.0) / F(255.0), F(128.0) / F(255.0)
WEIGHTS = [F(3.0) / F(16.0), F(6.0) / F(16.0), F(3.0) / F(16.0), F(1.0) / F(16.0), F(2.0) / F(16.0), F(1.0) / F(16.0)]


def raster_pixels(codes, full, cur, width, height):
    """P(x, y) for the raster: the frame's half RGBA codes (H, W, 4) inside `cur`, zero elsewhere (boxes inclusive)."""
    p = np.zeros((height, width, 4), np.uint16)
    x0, y0 = max(cur[0], 0), max(cur[1], 0)
    x1, y1 = min(cur[2], width - 1), min(cur[3], height - 1)
    if cur[0] <= cur[2] and cur[1] <= cur[3] and x0 <= x1 and y0 <= y1:
        p[y0:y1 + 1, x0:x1 + 1] = codes[y0 - full[1]:y1 - full[1] + 1, x0 - full[0]:x1 - full[0] + 1]
    return p


def encode(pixels, table):
    """Rec.709 transfer through the half table, widen, Rec.601 matrix: Y, Cb, Cr as float32 arrays."""
    with np.errstate(all="ignore"):
        r, g, b = (table[pixels[..., c]].view(np.float16).astype(F) for c in range(3))
        y = r * F(0.299)
        y = y + g * F(0.587)
        y = y + b * F(0.114)
        cb = r * F(-0.168736)
        cb = cb + g * F(-0.331264)
        cb = cb + b * F(0.5)
        cr = r * F(0.5)
        cr = cr + g * F(-0.418688)
        cr = cr + b * F(-0.081312)
    return y, cb, cr


def quantise(v, scale, offset):
    with np.errstate(all="ignore"):
        q = v * scale
        q = q + offset
        return np.rint(np.fmin(np.fmax(q, F(0.0)), F(1.0)) * F(255.0)).astype(np.uint8)


def chroma_rows(height):
    """(near, far) luma row of every chroma row: even cy -> 2cy, 2cy + 2; odd cy -> 2cy + 1, 2cy - 1."""
    cy = np.arange(height // 2)
    near = np.where(cy % 2 == 0, 2 * cy, 2 * cy + 1)
    far = np.where(cy % 2 == 0, 2 * cy + 2, 2 * cy - 1)
    return near, far


def subsample_encoded(y, cb, cr):
    """Planes from encoded (H, W) arrays: Y' (H, W), Cb and Cr (H/2, W/2)."""
    height, width = y.shape
    near, far = chroma_rows(height)
    cx = np.arange(width // 2)
    cols = [np.maximum(2 * cx - 1, 0), 2 * cx, 2 * cx + 1]
    out = [quantise(y, LUMA_SCALE, LUMA_OFFSET)]
    for plane in (cb, cr):
        taps = [plane[near][:, c] for c in cols] + [plane[far][:, c] for c in cols]
        with np.errstate(all="ignore"):
            acc = WEIGHTS[0] * taps[0]
            for wgt, tap in zip(WEIGHTS[1:], taps[1:]):
                acc = acc + wgt * tap
        out.append(quantise(acc, CHROMA_SCALE, CHROMA_OFFSET))
    return out


def mpeg2_subsample_model(codes, full, cur, width, height, table):
    """codes: (H, W, 4) uint16 half RGBA of the frame whose full window is `full`; cur: its current window.
    Returns [Y' (height, width), Cb (height/2, width/2), Cr (height/2, width/2)] as uint8 arrays."""
    assert width >= 2 and width % 2 == 0 and height >= 4 and height % 4 == 0
    y, cb, cr = encode(raster_pixels(codes, full, cur, width, height), table)
    return subsample_encoded(y, cb, cr)
