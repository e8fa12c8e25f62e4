"""numpy restatement of the 4:2:2 Y'CbCr edges' contract (DESIGN.md "4:2:2 Y'CbCr edges", include/canvas_ycc422.h; the
reference has no code for it).  Strict float32, one operation per statement, no fused multiply-add anywhere; the truncating
float -> half conversion and the two half tables are handed in (oracle.float_to_half, oracle.transfer_table(0) and (2)).

The arithmetic is the MPEG-2 edges' without the vertical part, so `horizontal`, `MATRICES` and `expected_frame` come from
tests/mpeg2_reconstruct_model.py and `raster_pixels` and `encode` from tests/mpeg2_model.py.  The four layouts have pack and
unpack functions written independently of each other (v210: one from shifts, one from a field table).

RULES names the rules a catalogue of cases must exercise (tests/test_ycc422_cpu.py): every model function takes `rules`, and a
rule set to False computes the plausible WRONG thing, so that a case whose expectation does not move exercises nothing."""
import numpy as np

from tests.mpeg2_model import encode as encode_601
from tests.mpeg2_model import raster_pixels
from tests.mpeg2_reconstruct_model import MATRICES, expected_frame, horizontal  # noqa: F401  (expected_frame: for the callers)

F = np.float32
LAYOUTS = {"planar8": 0, "planar10": 1, "uyvy": 2, "v210": 3}           # the header's CVS_422_* values
BITS = {"planar8": 8, "planar10": 10, "uyvy": 8, "v210": 10}
PLANES = {"planar8": 3, "planar10": 3, "uyvy": 1, "v210": 1}
ALIGN = {"planar8": 1, "planar10": 2, "uyvy": 1, "v210": 4}
# R'G'B' -> Y'CbCr, row by row: Rec.601 as DESIGN.md 4.5 has it, Rec.709 as the issue of this edge states it
RGB_MATRICES = {"601": [[0.299, 0.587, 0.114], [-0.168736, -0.331264, 0.5], [0.5, -0.418688, -0.081312]],
                "709": [[0.2126, 0.7152, 0.0722], [-0.114572, -0.385428, 0.5], [0.5, -0.454153, -0.045847]]}
RULES = dict(right_clamp=True, left_clamp=True, partial_group=True, mask=True, sdi_clamp=True, matrix=True, black_outside=True)


def size_ok(width, height):
    return width >= 2 and width % 2 == 0 and height >= 1


def least(layout, width, height):
    """(strides, line counts) of cvs_ycc422_layout, restated."""
    assert size_ok(width, height)
    strides = {"planar8": [width, width // 2, width // 2], "planar10": [2 * width, width, width], "uyvy": [2 * width],
               "v210": [16 * ((width + 5) // 6)]}[layout]
    return strides, [height] * len(strides)


# ---------------------------------------------------------------- layouts: pack

def _buffers(layout, width, height, strides, lines, fill):
    ls, ll = least(layout, width, height)
    strides, lines = ls if strides is None else strides, ll if lines is None else lines
    assert all(s >= m for s, m in zip(strides, ls)) and all(n >= height for n in lines)
    return [np.full((n, s), fill, np.uint8) for n, s in zip(lines, strides)]


def pack(layout, y, cb, cr, strides=None, lines=None, fill=0, rules=RULES):
    """Integer sample arrays y (H, W), cb and cr (H, W/2) -> the layout's planes as uint8 arrays (lines, stride): the least
    stride's bytes of the first H lines are written, everything else keeps `fill`."""
    height, width = y.shape
    out = _buffers(layout, width, height, strides, lines, fill)
    if layout == "planar8":
        for buf, a in zip(out, (y, cb, cr)):
            buf[:height, :a.shape[1]] = a
    elif layout == "planar10":
        for buf, a in zip(out, (y, cb, cr)):
            buf[:height, :2 * a.shape[1]] = np.ascontiguousarray(a.astype("<u2")).view(np.uint8).reshape(height, -1)
    elif layout == "uyvy":
        row = np.empty((height, width // 2, 4), np.uint8)
        row[..., 0], row[..., 1], row[..., 2], row[..., 3] = cb, y[:, 0::2], cr, y[:, 1::2]
        out[0][:height, :2 * width] = row.reshape(height, -1)
    else:
        out[0][:height, :16 * ((width + 5) // 6)] = _v210_words(y, cb, cr, rules).view(np.uint8).reshape(height, -1)
    return out


def _v210_words(y, cb, cr, rules):
    """From shifts: the four words of every group of six pixels; the fields beyond the width are 0."""
    height, width = y.shape
    groups = (width + 5) // 6
    # (the rule altered: a last group's unused fields hold the black codes instead of 0)
    gap_y, gap_c = (0, 0) if rules["partial_group"] else (64, 512)
    yy = np.full((height, 6 * groups), gap_y, np.uint32)
    bb, rr = np.full((height, 3 * groups), gap_c, np.uint32), np.full((height, 3 * groups), gap_c, np.uint32)
    yy[:, :width], bb[:, :width // 2], rr[:, :width // 2] = y, cb, cr
    words = np.empty((height, groups, 4), "<u4")
    words[..., 0] = bb[:, 0::3] | (yy[:, 0::6] << 10) | (rr[:, 0::3] << 20)
    words[..., 1] = yy[:, 1::6] | (bb[:, 1::3] << 10) | (yy[:, 2::6] << 20)
    words[..., 2] = rr[:, 1::3] | (yy[:, 3::6] << 10) | (bb[:, 2::3] << 20)
    words[..., 3] = yy[:, 4::6] | (rr[:, 2::3] << 10) | (yy[:, 5::6] << 20)
    return words


# ---------------------------------------------------------------- layouts: unpack

# v210 from a field table: (word, first bit, plane, sample within the group)
V210_FIELDS = [(0, 0, "cb", 0), (0, 10, "y", 0), (0, 20, "cr", 0), (1, 0, "y", 1), (1, 10, "cb", 1), (1, 20, "y", 2),
               (2, 0, "cr", 1), (2, 10, "y", 3), (2, 20, "cb", 2), (3, 0, "y", 4), (3, 10, "cr", 2), (3, 20, "y", 5)]


def unpack(layout, planes, width, height, rules=RULES, whole_groups=False):
    """The layout's planes (uint8 arrays (lines, stride), padding ignored) -> y (H, W), cb, cr (H, W/2) as int32.  The 10-bit
    layouts keep bits 0-9 of a sample (rule `mask` altered: PLANAR10 keeps all 16 bits, a v210 word's third field bits 20-31).
    whole_groups (v210): the samples of whole groups, fields beyond the width included."""
    cw = width // 2
    if layout == "planar8":
        return tuple(p[:height, :n].astype(np.int32) for p, n in zip(planes, (width, cw, cw)))
    if layout == "planar10":
        keep = 0x3FF if rules["mask"] else 0xFFFF
        out = []
        for p, n in zip(planes, (width, cw, cw)):
            b = p[:height, :2 * n].astype(np.int32)
            out.append((b[:, 0::2] + 256 * b[:, 1::2]) & keep)
        return tuple(out)
    if layout == "uyvy":
        b = planes[0][:height, :2 * width].astype(np.int32)
        y = np.empty((height, width), np.int32)
        y[:, 0::2], y[:, 1::2] = b[:, 1::4], b[:, 3::4]
        return y, b[:, 0::4], b[:, 2::4]
    groups = (width + 5) // 6
    words = np.ascontiguousarray(planes[0][:height, :16 * groups]).view("<u4").reshape(height, groups, 4).astype(np.int64)
    got = {"y": np.zeros((height, 6 * groups), np.int32), "cb": np.zeros((height, 3 * groups), np.int32), "cr": np.zeros((height, 3 * groups), np.int32)}
    for word, bit, plane, k in V210_FIELDS:
        keep = 0x3FF if rules["mask"] or bit < 20 else 0xFFF
        got[plane][:, k::6 if plane == "y" else 3] = (words[..., word] >> bit) & keep
    if whole_groups:
        return got["y"], got["cb"], got["cr"]
    return got["y"][:, :width], got["cb"][:, :cw], got["cr"][:, :cw]


# ---------------------------------------------------------------- import: samples -> half RGBA

def decode_luma(y, bits):
    s = F(1 << (bits - 8))
    return (y.astype(F) - F(16.0) * s) / (F(219.0) * s)


def decode_chroma(c, bits):
    s = F(1 << (bits - 8))
    return (c.astype(F) - F(128.0) * s) / (F(224.0) * s)


def _horizontal(v, beyond, rules):
    """mpeg2_reconstruct_model.horizontal, whose k + 1 is clamped to W/2 - 1.  Rules altered: the column right of the last is 0
    (right_clamp), or the field a v210 group holds there (`beyond`, partial_group)."""
    h = horizontal(v)
    if not rules["right_clamp"]:
        right = np.zeros_like(v[:, -1])
    elif not rules["partial_group"] and beyond is not None:
        right = beyond
    else:
        return h
    with np.errstate(all="ignore"):
        h[:, -1] = (v[:, -1] + right) * F(0.5)
    return h


def rgb(layout, planes, width, height, matrix="709", rules=RULES):
    """The f32 R'G'B' of the raster before truncation."""
    assert size_ok(width, height), (width, height)
    bits, cw = BITS[layout], width // 2
    y, cb, cr = unpack(layout, planes, width, height, rules)
    beyond = [None, None]
    if layout == "v210" and cw % 3:
        _, wb, wr = unpack(layout, planes, width, height, rules, whole_groups=True)
        beyond = [decode_chroma(wb[:, cw], bits), decode_chroma(wr[:, cw], bits)]
    yf = decode_luma(y, bits)
    hb, hr = (_horizontal(decode_chroma(c, bits), b, rules) for c, b in zip((cb, cr), beyond))
    if not rules["matrix"]:
        matrix = "601" if matrix == "709" else "709"
    out = []
    with np.errstate(all="ignore"):
        for m0, m1, m2 in MATRICES[matrix]:
            a = yf * F(m0)
            b = hb * F(m1)
            c = hr * F(m2)
            out.append((a + b) + c)
    return out


def reconstruct_halves(layout, planes, width, height, float_to_half, matrix="709", rules=RULES):
    """(H, W, 4) half codes before the table: r, g, b truncated to half, alpha 1.0."""
    codes = np.empty((height, width, 4), np.uint16)
    for i, c in enumerate(rgb(layout, planes, width, height, matrix, rules)):
        codes[..., i] = float_to_half(c)
    codes[..., 3] = float_to_half(np.array([1.0], F))[0]
    return codes


def reconstruct_model(layout, planes, width, height, table, float_to_half, matrix="709", rules=RULES):
    """The raster's pixels as the contract stores them: (H, W, 4) uint16 codes, all four through `table` (Rec.709 -> linear)."""
    return table[reconstruct_halves(layout, planes, width, height, float_to_half, matrix, rules)]


# ---------------------------------------------------------------- export: half RGBA -> samples

def encode(pixels, table, matrix):
    """Rec.709 transfer through the half table (linear -> Rec.709), widen, matrix: Y, Cb, Cr as float32 arrays.  Rec.601 is
    mpeg2_model.encode itself; the same statements with the other coefficients for Rec.709."""
    if matrix == "601":
        return encode_601(pixels, table)
    (y0, y1, y2), (b0, b1, b2), (r0, r1, r2) = RGB_MATRICES[matrix]
    with np.errstate(all="ignore"):
        r, g, b = (table[pixels[..., c]].view(np.float16).astype(F) for c in range(3))
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


def quantise(v, bits, chroma, rules=RULES):
    s, top = F(1 << (bits - 8)), F((1 << bits) - 1)
    scale = (F(224.0 if chroma else 219.0) * s) / top
    offset = (F(128.0 if chroma else 16.0) * s) / top
    with np.errstate(all="ignore"):
        q = v * scale
        q = q + offset
        code = np.rint(np.fmin(np.fmax(q, F(0.0)), F(1.0)) * top).astype(np.int32)
    if bits == 10 and rules["sdi_clamp"]:
        code = np.clip(code, 4, 1019)
    return code


def filter_chroma(e, rules=RULES):
    """E (H, W) -> C (H, W/2): 0.25 E(2k-1) + 0.5 E(2k) + 0.25 E(2k+1), left to right, column -1 reading column 0 (rule
    altered: reading 0)."""
    k = np.arange(e.shape[1] // 2)
    left = e[:, np.maximum(2 * k - 1, 0)].copy()
    if not rules["left_clamp"]:
        left[:, 0] = F(0.0)
    with np.errstate(all="ignore"):
        c = F(0.25) * left
        c = c + F(0.5) * e[:, 2 * k]
        c = c + F(0.25) * e[:, 2 * k + 1]
    return c


def subsample_samples(codes, full, cur, width, height, bits, table, matrix="709", rules=RULES):
    """codes: (h, w, 4) uint16 half RGBA of the frame whose full window is `full`; cur: its current window; table: linear ->
    Rec.709.  Returns y (H, W), cb, cr (H, W/2) as int32 codes."""
    assert size_ok(width, height)
    if not rules["black_outside"]:
        cur = full
    if not rules["matrix"]:
        matrix = "601" if matrix == "709" else "709"
    y, cb, cr = encode(raster_pixels(codes, full, cur, width, height), table, matrix)
    return quantise(y, bits, False, rules), quantise(filter_chroma(cb, rules), bits, True, rules), quantise(filter_chroma(cr, rules), bits, True, rules)


def subsample_model(layout, codes, full, cur, width, height, table, matrix="709", strides=None, lines=None, fill=0, rules=RULES):
    """The layout's planes after the call, on buffers that held `fill` in every byte."""
    y, cb, cr = subsample_samples(codes, full, cur, width, height, BITS[layout], table, matrix, rules)
    return pack(layout, y, cb, cr, strides, lines, fill, rules)
