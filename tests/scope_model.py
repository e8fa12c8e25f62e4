"""The scopes' contract (DESIGN.md "Scopes") in numpy: from display BYTES to the four count tables and the three pictures.

The model takes an (h, w, 4) uint8 array -- the bytes r, g, b, a the display edge gives for the frame's current window -- so
it restates no powf and no table: whatever cvs_frame_to_bytes_dev / cvs_frame_to_rgba8_intent_dev export is what it counts.
Everything is integer arithmetic; the pictures' one float product is rounded once, in f32."""
import numpy as np

from tests.models import f2h_rz_model

HISTOGRAM, WAVEFORM, PARADE, VECTORSCOPE = range(4)
KINDS = {"histogram": HISTOGRAM, "waveform": WAVEFORM, "parade": PARADE, "vectorscope": VECTORSCOPE}
MAX_COLUMNS = 4096


def luma(r, g, b):
    return (13933 * r + 46871 * g + 4732 * b + 32768) >> 16


def chroma(r, g, b):
    """(Cb, Cr); >> on numpy's signed integers and on Python's ints is a floor"""
    cb = 128 + ((-7509 * r - 25259 * g + 32768 * b + 32768) >> 16)
    cr = 128 + ((32768 * r - 29763 * g - 3005 * b + 32768) >> 16)
    return np.minimum(cb, 255), np.minimum(cr, 255)


def count(kind, columns):
    return {HISTOGRAM: 5 * 256, WAVEFORM: columns * 256, PARADE: 3 * columns * 256, VECTORSCOPE: 256 * 256}[kind]


def picture_size(kind, columns):
    """(width, height); the histogram has none"""
    return {WAVEFORM: (columns, 256), PARADE: (3 * columns, 256), VECTORSCOPE: (256, 256)}[kind]


def intersect(a, b):
    if a is None or b is None:
        return None
    r = (max(a[0], b[0]), max(a[1], b[1]), min(a[2], b[2]), min(a[3], b[3]))
    return None if r[2] < r[0] or r[3] < r[1] else r


def table(kind, px, cur, region, columns=256, skip_transparent=False):
    """The flat uint32 table of `kind` for the bytes px (h, w, 4) of the window cur = (x0, y0, x1, y1), None for an empty one,
    measured over `region`."""
    out = np.zeros(count(kind, columns), np.int64)
    m = intersect(cur, region)
    if m is None:
        return out.astype(np.uint32)
    sub = np.asarray(px)[m[1] - cur[1]:m[3] - cur[1] + 1, m[0] - cur[0]:m[2] - cur[0] + 1].astype(np.int64)
    r, g, b, a = sub[..., 0], sub[..., 1], sub[..., 2], sub[..., 3]
    keep = (a != 0) if skip_transparent else np.ones(a.shape, bool)
    width = region[2] - region[0] + 1
    c = np.broadcast_to((np.arange(m[0], m[2] + 1, dtype=np.int64) - region[0]) * columns // width, r.shape)
    y = luma(r, g, b)

    def add(index):
        np.add.at(out, index[keep], 1)
    if kind == HISTOGRAM:
        for row, level in enumerate((r, g, b, a, y)):
            add(row * 256 + level)
    elif kind == WAVEFORM:
        add(c * 256 + y)
    elif kind == PARADE:
        for panel, level in enumerate((r, g, b)):
            add((panel * columns + c) * 256 + level)
    else:
        cb, cr = chroma(r, g, b)
        add(cr * 256 + cb)
    assert out.max(initial=0) < 2 ** 32
    return out.astype(np.uint32)


def picture(kind, counts, columns, gain):
    """The whole picture as (256, width, 4) half codes: v = min(f32(n) * f32(gain), 1), truncated."""
    w, h = picture_size(kind, columns)
    n = np.asarray(counts, np.uint32)
    if kind == VECTORSCOPE:
        grid = n.reshape(256, 256)[::-1, :]                              # [255 - j][i]
    else:
        grid = n.reshape(w, 256).T[::-1, :]                              # [i][255 - j]; the parade's panels lie side by side
    v = np.minimum(grid.astype(np.float32) * np.float32(gain), np.float32(1.0)).astype(np.float32)
    out = np.zeros((h, w, 4), np.float32)
    out[..., 3] = 1.0
    if kind == PARADE:
        for panel in range(3):
            out[:, panel * columns:(panel + 1) * columns, panel] = v[:, panel * columns:(panel + 1) * columns]
    else:
        out[..., 0] = out[..., 1] = out[..., 2] = v
    return f2h_rz_model(out).astype(np.uint16).reshape(h, w, 4)


# ------------------------------------------------------------------ the same, pixel by pixel (what test_scope_cpu.py holds the above to)

def table_by_loops(kind, px, cur, region, columns=256, skip_transparent=False):
    out = [0] * count(kind, columns)
    if cur is None:
        return np.array(out, np.uint32)
    width = region[2] - region[0] + 1
    for y in range(cur[1], cur[3] + 1):
        for x in range(cur[0], cur[2] + 1):
            if not (region[0] <= x <= region[2] and region[1] <= y <= region[3]):
                continue
            r, g, b, a = (int(v) for v in px[y - cur[1]][x - cur[0]])
            if skip_transparent and a == 0:
                continue
            c = (x - region[0]) * columns // width
            lum = (13933 * r + 46871 * g + 4732 * b + 32768) // 65536
            cb = min(255, 128 + (-7509 * r - 25259 * g + 32768 * b + 32768) // 65536)
            cr = min(255, 128 + (32768 * r - 29763 * g - 3005 * b + 32768) // 65536)
            if kind == HISTOGRAM:
                for row, level in enumerate((r, g, b, a, lum)):
                    out[row * 256 + level] += 1
            elif kind == WAVEFORM:
                out[c * 256 + lum] += 1
            elif kind == PARADE:
                for panel, level in enumerate((r, g, b)):
                    out[(panel * columns + c) * 256 + level] += 1
            else:
                out[cr * 256 + cb] += 1
    return np.array(out, np.uint32)


def picture_by_loops(kind, counts, columns, gain):
    w, h = picture_size(kind, columns)
    out = np.zeros((h, w, 4), np.float32)
    for j in range(h):
        for i in range(w):
            if kind == WAVEFORM:
                n = counts[i * 256 + 255 - j]
            elif kind == PARADE:
                n = counts[((i // columns) * columns + i % columns) * 256 + 255 - j]
            else:
                n = counts[(255 - j) * 256 + i]
            v = min(np.float32(np.float32(n) * np.float32(gain)), np.float32(1.0))
            out[j, i] = (v, v, v, 1.0) if kind != PARADE else tuple(v if k == i // columns else 0.0 for k in range(3)) + (1.0,)
    return f2h_rz_model(out).astype(np.uint16).reshape(h, w, 4)
