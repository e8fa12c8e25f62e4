"""numpy restatement of the 4:2:0 Y'CbCr edges' contract (DESIGN.md "4:2:0 Y'CbCr edges", include/canvas_ycc420.h; the reference
has no code for it).  Strict float32, one operation per statement, no fused multiply-add anywhere; the truncating float -> half
conversion and the two half tables are handed in (oracle.float_to_half, oracle.transfer_table(0) and (2)).

`raster_pixels` (export) and `expected_frame` (import) are the MPEG-2 models'; everything else is stated here, so that the
cross-checks against tests/mpeg2_reconstruct_model.py hold this file to one it does not share its arithmetic with.

RULES names the rules a catalogue of cases must exercise (tests/test_ycc420_cpu.py): every model function takes `rules`, and a
rule set to False computes the plausible WRONG thing, so that a case whose expectation does not move exercises nothing."""
import numpy as np

from tests.mpeg2_model import raster_pixels
from tests.mpeg2_reconstruct_model import expected_frame  # noqa: F401  (for the callers)

F = np.float32
LAYOUTS = {"planar8": 0, "planar10": 1, "nv12": 2, "p010": 3}           # the header's CVS_420_* values
BITS = {"planar8": 8, "planar10": 10, "nv12": 8, "p010": 10}
PLANES = {"planar8": 3, "planar10": 3, "nv12": 2, "p010": 2}
ALIGN = {"planar8": 1, "planar10": 2, "nv12": 1, "p010": 2}
SHIFT = {"planar8": 0, "planar10": 0, "nv12": 0, "p010": 6}             # where a code sits in its sample
MATRIX_FLAGS = {"601": 0, "709": 2, "2020": 4}
RANGE_FLAGS = {"studio": 0, "full": 8}
SITING_FLAGS = {"left": 0, "center": 16, "topleft": 32}
TRANSFER_FLAGS = {"709": 0, "none": 64}
# Y'CbCr -> R'G'B', row by row: Rec.601 and Rec.709 as DESIGN.md 4.6 has them, Rec.2020 (non-constant luminance) as the header
MATRICES = {"601": [[1.0, 0.0, 1.402], [1.0, -0.344136, -0.714136], [1.0, 1.772, 0.0]],
            "709": [[1.0, 0.0, 1.5748], [1.0, -0.187324, -0.468124], [1.0, 1.8556, 0.0]],
            "2020": [[1.0, 0.0, 1.4746], [1.0, -0.164553, -0.571353], [1.0, 1.8814, 0.0]]}
# R'G'B' -> Y'CbCr, row by row
RGB_MATRICES = {"601": [[0.299, 0.587, 0.114], [-0.168736, -0.331264, 0.5], [0.5, -0.418688, -0.081312]],
                "709": [[0.2126, 0.7152, 0.0722], [-0.114572, -0.385428, 0.5], [0.5, -0.454153, -0.045847]],
                "2020": [[0.2627, 0.6780, 0.0593], [-0.139630, -0.360370, 0.5], [0.5, -0.459786, -0.040214]]}
WRONG_MATRIX = {"601": "709", "709": "2020", "2020": "601"}
RULES = dict(top_clamp=True, bottom_clamp=True, left_clamp=True, right_clamp=True, mask=True, sdi_clamp=True, matrix=True, range=True, siting_v=True,
             siting_h=True, transfer=True, black_outside=True)


def flags(matrix="709", range_="studio", siting="left", transfer="709"):
    return MATRIX_FLAGS[matrix] | RANGE_FLAGS[range_] | SITING_FLAGS[siting] | TRANSFER_FLAGS[transfer]


def size_ok(width, height):
    return width >= 2 and width % 2 == 0 and height >= 2 and height % 2 == 0


def least(layout, width, height):
    """(strides, line counts) of cvs_ycc420_layout, restated."""
    assert size_ok(width, height)
    b = BITS[layout] // 8 if BITS[layout] == 8 else 2
    if PLANES[layout] == 3:
        return [b * width, b * (width // 2), b * (width // 2)], [height, height // 2, height // 2]
    return [b * width, b * width], [height, height // 2]


# ---------------------------------------------------------------- layouts

def pack(layout, y, cb, cr, strides=None, lines=None, fill=0):
    """Integer code arrays y (H, W), cb and cr (H/2, W/2) -> the layout's planes as uint8 arrays (lines, stride): the least
    stride's bytes of each plane's lines are written, everything else keeps `fill`."""
    height, width = y.shape
    ls, ll = least(layout, width, height)
    strides, lines = ls if strides is None else strides, ll if lines is None else lines
    assert all(s >= m for s, m in zip(strides, ls)) and all(n >= m for n, m in zip(lines, ll))
    out = [np.full((n, s), fill, np.uint8) for n, s in zip(lines, strides)]
    if PLANES[layout] == 3:
        arrays = [y, cb, cr]
    else:
        inter = np.empty((height // 2, width), np.int64)
        inter[:, 0::2], inter[:, 1::2] = cb, cr
        arrays = [y, inter]
    for buf, a in zip(out, arrays):
        a = np.asarray(a).astype(np.int64) << SHIFT[layout]
        if BITS[layout] == 8:
            buf[:a.shape[0], :a.shape[1]] = a
        else:
            buf[:a.shape[0], :2 * a.shape[1]] = np.ascontiguousarray(a.astype("<u2")).view(np.uint8).reshape(a.shape[0], -1)
    return out


def unpack(layout, planes, width, height, rules=RULES):
    """The layout's planes (uint8 arrays (lines, stride), padding ignored) -> y (H, W), cb, cr (H/2, W/2) as int32 codes.  PLANAR10
    keeps bits 0-9 of a sample, P010 bits 6-15 (rule `mask` altered: PLANAR10 keeps all 16 bits, P010 rounds bits 0-5 into the code)."""
    cw, ch = width // 2, height // 2
    shapes = [(height, width), (ch, cw), (ch, cw)] if PLANES[layout] == 3 else [(height, width), (ch, width)]
    got = []
    for p, (n, m) in zip(planes, shapes):
        if BITS[layout] == 8:
            got.append(p[:n, :m].astype(np.int32))
        else:
            b = p[:n, :2 * m].astype(np.int32)
            raw = b[:, 0::2] + 256 * b[:, 1::2]
            if rules["mask"]:
                got.append((raw >> SHIFT[layout]) & 0x3FF)
            else:
                got.append(np.minimum((raw + 32) >> 6, 1023) if SHIFT[layout] else raw)
    if PLANES[layout] == 3:
        return tuple(got)
    return got[0], got[1][:, 0::2], got[1][:, 1::2]


# ---------------------------------------------------------------- import: samples -> half RGBA

def decode_luma(y, bits, range_="studio"):
    s, top = F(1 << (bits - 8)), F((1 << bits) - 1)
    if range_ == "full":
        return y.astype(F) / top
    return (y.astype(F) - F(16.0) * s) / (F(219.0) * s)


def decode_chroma(c, bits, range_="studio"):
    s, top = F(1 << (bits - 8)), F((1 << bits) - 1)
    if range_ == "full":
        return (c.astype(F) - F(128.0) * s) / top
    return (c.astype(F) - F(128.0) * s) / (F(224.0) * s)


def _rows(p, index, lo_rule, hi_rule):
    """p[index] with the index clamped to the plane; a rule altered: rows beyond that edge read 0."""
    n = p.shape[0]
    out = p[np.clip(index, 0, n - 1)].copy()
    if not lo_rule:
        out[index < 0] = F(0.0)
    if not hi_rule:
        out[index >= n] = F(0.0)
    return out


def vertical(p, siting="left", rules=RULES):
    """Decoded chroma (H/2, W/2) -> v per luma row (H, W/2)."""
    if not rules["siting_v"]:
        siting = "left" if siting == "topleft" else "topleft"
    y = np.arange(2 * p.shape[0])
    c = y >> 1
    near = p[c]
    with np.errstate(all="ignore"):
        if siting == "topleft":
            below = _rows(p, c + 1, True, rules["bottom_clamp"])
            mean = (near + below) * F(0.5)
            return np.where((y % 2 == 0)[:, None], near, mean)
        far = _rows(p, np.where(y % 2 == 0, c - 1, c + 1), rules["top_clamp"], rules["bottom_clamp"])
        a = near * F(0.75)
        b = far * F(0.25)
        return a + b


def horizontal(v, siting="left", rules=RULES):
    """v (H, W/2) -> h (H, W)."""
    if not rules["siting_h"]:
        siting = "left" if siting == "center" else "center"
    x = np.arange(2 * v.shape[1])
    k = x >> 1
    vt = v.T
    near = vt[k]
    with np.errstate(all="ignore"):
        if siting == "center":
            far = _rows(vt, np.where(x % 2 == 0, k - 1, k + 1), rules["left_clamp"], rules["right_clamp"])
            a = near * F(0.75)
            b = far * F(0.25)
            return (a + b).T
        right = _rows(vt, k + 1, True, rules["right_clamp"])
        mean = (near + right) * F(0.5)
        return np.where((x % 2 == 0)[:, None], near, mean).T


def rgb(layout, planes, width, height, matrix="709", range_="studio", siting="left", rules=RULES):
    """The f32 R'G'B' of the raster before truncation."""
    assert size_ok(width, height), (width, height)
    bits = BITS[layout]
    if not rules["range"]:
        range_ = "studio" if range_ == "full" else "full"
    if not rules["matrix"]:
        matrix = WRONG_MATRIX[matrix]
    y, cb, cr = unpack(layout, planes, width, height, rules)
    yf = decode_luma(y, bits, range_)
    hb, hr = (horizontal(vertical(decode_chroma(c, bits, range_), siting, rules), siting, rules) for c in (cb, cr))
    out = []
    with np.errstate(all="ignore"):
        for m0, m1, m2 in MATRICES[matrix]:
            a = yf * F(m0)
            b = hb * F(m1)
            c = hr * F(m2)
            out.append((a + b) + c)
    return out


def reconstruct_halves(layout, planes, width, height, float_to_half, matrix="709", range_="studio", siting="left", rules=RULES):
    """(H, W, 4) half codes before the table: r, g, b truncated to half, alpha 1.0."""
    codes = np.empty((height, width, 4), np.uint16)
    for i, c in enumerate(rgb(layout, planes, width, height, matrix, range_, siting, rules)):
        codes[..., i] = float_to_half(c)
    codes[..., 3] = float_to_half(np.array([1.0], F))[0]
    return codes


def reconstruct_model(layout, planes, width, height, table, float_to_half, matrix="709", range_="studio", siting="left", transfer="709", rules=RULES):
    """The raster's pixels as the contract stores them: (H, W, 4) uint16 codes, all four through `table` (Rec.709 -> linear) unless
    transfer is "none"."""
    halves = reconstruct_halves(layout, planes, width, height, float_to_half, matrix, range_, siting, rules)
    if not rules["transfer"]:
        transfer = "709" if transfer == "none" else "none"
    return halves if transfer == "none" else table[halves]


# ---------------------------------------------------------------- export: half RGBA -> samples

def encode(pixels, table, matrix, transfer="709"):
    """The linear -> Rec.709 half table (unless transfer is "none"), widen, matrix: Y, Cb, Cr as float32 arrays."""
    (y0, y1, y2), (b0, b1, b2), (r0, r1, r2) = RGB_MATRICES[matrix]
    with np.errstate(all="ignore"):
        r, g, b = ((pixels[..., c] if transfer == "none" else table[pixels[..., c]]).view(np.float16).astype(F) for c in range(3))
        y = r * F(y0)
        y = y + g * F(y1)
        y = y + b * F(y2)
        cb = r * F(b0)
        cb = cb + g * F(b1)
        cb = cb + b * F(b2)
        cr = r * F(r0)
        cr = cr + g * F(r1)
        cr = cr + b * F(r2)
    return y, cb, cr


def quantise(v, bits, chroma, range_="studio", rules=RULES):
    s, top = F(1 << (bits - 8)), F((1 << bits) - 1)
    with np.errstate(all="ignore"):
        if range_ == "full":
            q = v + (F(128.0) * s) / top if chroma else v
        else:
            scale = (F(224.0 if chroma else 219.0) * s) / top
            offset = (F(128.0 if chroma else 16.0) * s) / top
            q = v * scale
            q = q + offset
        code = np.rint(np.fmin(np.fmax(q, F(0.0)), F(1.0)) * top).astype(np.int32)
    if bits == 10 and range_ == "studio" and rules["sdi_clamp"]:
        code = np.clip(code, 4, 1019)
    return code


def _tent(a, b, c):
    with np.errstate(all="ignore"):
        v = F(0.25) * a
        v = v + F(0.5) * b
        v = v + F(0.25) * c
    return v


def filter_chroma(e, siting="left", rules=RULES):
    """E (H, W) -> C (H/2, W/2): the vertical step, then the horizontal one."""
    sv = siting if rules["siting_v"] else ("left" if siting == "topleft" else "topleft")
    sh = siting if rules["siting_h"] else ("left" if siting == "center" else "center")
    c = np.arange(e.shape[0] // 2)
    k = np.arange(e.shape[1] // 2)
    with np.errstate(all="ignore"):
        if sv == "topleft":
            above = e[np.maximum(2 * c - 1, 0)].copy()
            if not rules["top_clamp"]:
                above[0] = F(0.0)
            v = _tent(above, e[2 * c], e[2 * c + 1])
        else:
            v = (e[2 * c] + e[2 * c + 1]) * F(0.5)
        if sh == "center":
            return (v[:, 2 * k] + v[:, 2 * k + 1]) * F(0.5)
        left = v[:, np.maximum(2 * k - 1, 0)].copy()
        if not rules["left_clamp"]:
            left[:, 0] = F(0.0)
        return _tent(left, v[:, 2 * k], v[:, 2 * k + 1])


def subsample_samples(codes, full, cur, width, height, bits, table, matrix="709", range_="studio", siting="left", transfer="709", rules=RULES):
    """codes: (h, w, 4) uint16 half RGBA of the frame whose full window is `full`; cur: its current window; table: linear ->
    Rec.709.  Returns y (H, W), cb, cr (H/2, W/2) as int32 codes."""
    assert size_ok(width, height)
    if not rules["black_outside"]:
        cur = full
    if not rules["matrix"]:
        matrix = WRONG_MATRIX[matrix]
    if not rules["range"]:
        range_ = "studio" if range_ == "full" else "full"
    if not rules["transfer"]:
        transfer = "709" if transfer == "none" else "none"
    y, cb, cr = encode(raster_pixels(codes, full, cur, width, height), table, matrix, transfer)
    return (quantise(y, bits, False, range_, rules), quantise(filter_chroma(cb, siting, rules), bits, True, range_, rules),
            quantise(filter_chroma(cr, siting, rules), bits, True, range_, rules))


def subsample_model(layout, codes, full, cur, width, height, table, matrix="709", range_="studio", siting="left", transfer="709", strides=None, lines=None,
                    fill=0, rules=RULES):
    """The layout's planes after the call, on buffers that held `fill` in every byte."""
    y, cb, cr = subsample_samples(codes, full, cur, width, height, BITS[layout], table, matrix, range_, siting, transfer, rules)
    return pack(layout, y, cb, cr, strides, lines, fill)
