"""The 4:2:2 Y'CbCr edges without a GPU (DESIGN.md "4:2:2 Y'CbCr edges"): include/canvas_ycc422.h against the library and its
bindings; cvs_ycc422_layout, which is host only; every argument refusal of the two device entries by its message (they come before
the device is touched); the numpy model (tests/ycc422_model.py) pinned against studio-range anchors,
its pack and unpack functions against each other, a float64 restatement, the MPEG-2 edges' models and the round-trip facts; the
catalogue of tests/ycc422_cases.py, which must exercise every rule of the contract; the built code objects; the nodes' arguments."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import ycc422_cases as yc
from tests import ycc422_model as ym
from tests.mpeg2_model import mpeg2_subsample_model
from tests.mpeg2_reconstruct_model import reconstruct_model as mpeg2_reconstruct_model
from tests.test_perspective_cpu import _declared
from tests.test_unsharp_cpu import _kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "canvas_ycc422.h"
F = np.float32
LAYOUTS = list(ym.LAYOUTS)


@pytest.fixture(scope="module")
def lib():
    from canvas_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def tables(orc):
    """(Rec.709 -> linear (scene), linear -> Rec.709, float -> half)"""
    return orc.transfer_table(0), orc.transfer_table(2), orc.float_to_half


# ---------------------------------------------------------------- the header, the library, the bindings

def test_every_symbol_of_the_header_is_exported_and_bound(lib):
    from canvas_amd import _lib
    funcs, entries = _declared(HEADER)
    assert funcs == sorted(_lib.YCC422_SIGNATURES) == ["cvs_reconstruct_422_dev", "cvs_subsample_422_dev", "cvs_ycc422_layout"]
    assert entries == sorted(yc.ENTRIES)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name, (res, args) in _lib.YCC422_SIGNATURES.items():
        assert name in exported and getattr(lib, name).argtypes == args and getattr(lib, name).restype is res, name
    others = (set(_lib.SIGNATURES) | set(_lib.SCOPE_SIGNATURES) | set(_lib.LUT3D_SIGNATURES) | set(_lib.PERSPECTIVE_SIGNATURES) | set(_lib.DEINTERLACE_SIGNATURES)
              | set(_lib.MEDIAN_SIGNATURES) | set(_lib.TEMPORAL_SIGNATURES))
    assert not set(_lib.YCC422_SIGNATURES) & others
    assert "422" not in open(os.path.join(ROOT, "include", "canvas_hip.h")).read()
    assert (_lib.YCC422_PLANAR8, _lib.YCC422_PLANAR10, _lib.YCC422_UYVY, _lib.YCC422_V210) == tuple(ym.LAYOUTS[n] for n in LAYOUTS) == (0, 1, 2, 3)
    # one launcher per direction, one arithmetic flavour
    symbols = subprocess.run(["nm", _lib.LIB_PATH], stdout=subprocess.PIPE, text=True).stdout
    for name in ("cvk_ycc422_reconstruct", "cvk_ycc422_subsample"):
        assert (" " + name + "\n") in symbols and name + "_fma" not in symbols, name


def test_the_header_compiles_as_c_and_as_cpp():
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "t.c")
        with open(src, "w") as f:
            f.write('#include "%s"\nint main(void) { return CVS_422_PLANAR8 == 0 && CVS_422_PLANAR10 == 1 && CVS_422_UYVY == 2 && CVS_422_V210 == 3 && '
                    'CVS_YCC_REC709 == 2 ? 0 : 1; }\n' % HEADER)
        for cc, std, lang in (("gcc", "-std=c99", "c"), ("g++", "-std=c++14", "c++")):
            exe = os.path.join(tmp, "t_" + cc)
            subprocess.run([cc, std, "-Wall", "-Werror", "-x", lang, src, "-I", os.path.join(ROOT, "include"), "-o", exe], check=True)
            assert subprocess.run([exe]).returncode == 0


@pytest.mark.parametrize("obj,kernel", [("ycc422_recon_ops.hip.o", "k_ycc422_reconstruct"), ("ycc422_ops.hip.o", "k_ycc422_subsample")])
def test_code_objects_hold_the_eight_instances_without_scratch(obj, kernel):
    """One build for both arithmetic flavours; four layouts x two table placements; no private segment, no spills."""
    assert os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"), "the ROCm LLVM tools the build itself needs are missing"
    found = _kernels(obj)
    assert len(found) == 8 and all(kernel in n for n in found), sorted(found)
    for layout in range(4):
        for table, lanes in ((0, 1024), (1, 256)):
            assert any("%sILi%dELi%dELi%dEEE" % (kernel, layout, table, lanes) in n for n in found), (layout, table, sorted(found))
    for name, (scratch, spills) in found.items():
        assert scratch == 0 and spills == 0, (name, scratch, spills)
    assert not os.path.exists(os.path.join(ROOT, "canvas_amd", "csrc", "build", obj.replace(".hip.o", ".fma.hip.o")))


# ---------------------------------------------------------------- cvs_ycc422_layout (host only)

def _layout(lib, layout, width, height):
    strides, lines = (C.c_int * 3)(-7, -7, -7), (C.c_int * 3)(-7, -7, -7)
    lib.cvs_clear_last_error()
    return lib.cvs_ycc422_layout(layout, width, height, strides, lines), list(strides), list(lines)


def test_layout_values(lib):
    for width, height in [(2, 1), (4, 3), (6, 1), (8, 2), (10, 5), (14, 1), (720, 486), (1920, 1080), (3840, 2160), (4096, 2160)]:
        assert _layout(lib, 0, width, height) == (3, [width, width // 2, width // 2], [height] * 3)
        assert _layout(lib, 1, width, height) == (3, [2 * width, width, width], [height] * 3)
        assert _layout(lib, 2, width, height) == (1, [2 * width, 0, 0], [height, 0, 0])
        assert _layout(lib, 3, width, height) == (1, [16 * -(-width // 6), 0, 0], [height, 0, 0])
        for name in LAYOUTS:
            strides, lines = ym.least(name, width, height)
            planes, s, n = _layout(lib, ym.LAYOUTS[name], width, height)
            assert planes == ym.PLANES[name] == len(strides) and s[:planes] == strides and n[:planes] == lines
    assert _layout(lib, 3, 1280, 720)[1][0] == 3424            # 214 groups: the familiar v210 stride before a card's own 128-byte rounding
    # either array may be left out
    assert lib.cvs_ycc422_layout(3, 1920, 1080, None, None) == 1


def test_layout_refusals(lib):
    from canvas_amd import _lib
    for layout, width, height, word in [(-1, 16, 16, "layout"), (4, 16, 16, "layout"), (99, 16, 16, "layout"), (0, 0, 16, "width"), (1, 1, 16, "width"),
                                        (2, 15, 16, "width"), (3, 721, 486, "width"), (3, -6, 4, "width"), (0, 16, 0, "height"), (3, 16, -1, "height"),
                                        (1, 2 ** 30, 1, "width")]:
        rc, strides, lines = _layout(lib, layout, width, height)
        assert rc == -1 and strides == [-7] * 3 and lines == [-7] * 3, (layout, width, height)
        assert "cvs_ycc422_layout" in _lib.last_error() and word in _lib.last_error(), _lib.last_error()


def test_without_a_gpu_the_device_entries_refuse_or_fail_loudly(lib):
    from canvas_amd import _lib
    from canvas_amd.abi import HostFrame
    frame = HostFrame((0, 0, 7, 7), np.uint16, current_window=(0, 0, 7, 7))
    img = _lib.coded_image()
    assert lib.cvs_reconstruct_422_dev(frame.ref(), C.byref(img), 7, 8, 3, 0, None) == -1      # odd width: refused in any case
    assert frame.current_window.is_empty() and _lib.last_error()
    assert lib.cvs_reconstruct_422_dev(None, C.byref(img), 8, 8, 3, 0, None) == -1
    assert lib.cvs_subsample_422_dev(C.byref(img), frame.ref(), 8, 8, 3, 1, None) == -1        # CVS_YCC_PROGRESSIVE: no such thing here
    assert lib.cvs_subsample_422_dev(C.byref(img), None, 8, 8, 3, 0, None) == -1


@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_argument_refusal_by_its_message_and_nothing_is_written(lib, layout):
    """The refusals of tests/test_ycc422_gpu.py with no device: each comes before the device is touched, as the 4:2:0 edges' do, so
    host memory stands in for the operands and is seen to stay as it was."""
    from canvas_amd import _lib
    from canvas_amd.abi import HostFrame
    from tests.entry_cases import SENT16
    width, height, lid = 24, 4, ym.LAYOUTS[layout]
    full = (0, 0, width - 1, height - 1)
    strides, lines = ym.least(layout, width, height)
    arrays = [np.full(s * n + 64, 0xA5, np.uint8) for s, n in zip(strides, lines)]
    assert all(a.ctypes.data % 16 == 0 for a in arrays)            # (numpy's allocations are aligned well beyond 4)
    before = np.broadcast_to(SENT16, (height, width, 4)).copy()
    frame = HostFrame(full, np.uint16, before.copy(), full)

    def image(count=len(arrays)):
        img = _lib.coded_image()
        for p, (a, s, n) in enumerate(list(zip(arrays, strides, lines))[:count]):
            img.data[p], img.stride[p], img.line_count[p] = a.ctypes.data, s, n
        return img

    def refused(img, w, h, lay, flags, word, fr=frame):
        for entry in ("reconstruct", "subsample"):
            if fr is not None:
                fr.c.current_window = _lib.box2i.of(*full)
            lib.cvs_clear_last_error()
            ref = fr.ref() if fr is not None else None
            if entry == "reconstruct":
                rc = lib.cvs_reconstruct_422_dev(ref, C.byref(img) if img is not None else None, w, h, lay, flags, None)
                assert fr is None or fr.current_window.is_empty(), (entry, word)
            else:
                rc = lib.cvs_subsample_422_dev(C.byref(img) if img is not None else None, ref, w, h, lay, flags, None)
            assert rc == -1 and word in _lib.last_error(), (entry, word, rc, _lib.last_error())
            assert "4:2:2 " + entry in _lib.last_error(), _lib.last_error()

    refused(image(), width, height, lid, 0, "need a frame", fr=None)
    for w in (23, 25, 1, 0, -2):
        refused(image(), w, height, lid, 0, "width")
    for h in (0, -1):
        refused(image(), width, h, lid, 0, "height")
    for flags in (_lib.YCC_PROGRESSIVE, _lib.YCC_PROGRESSIVE | _lib.YCC_REC709, 4, -1):
        refused(image(), width, height, lid, flags, "unknown flags")
    for lay in (-1, 4, 17):
        refused(image(), width, height, lay, 0, "unknown layout")
    refused(None, width, height, lid, 0, "need an image")
    for p in range(len(arrays)):
        img = image()
        img.data[p] = None
        refused(img, width, height, lid, 0, "plane %d is missing" % p)
        img = image()
        img.stride[p] -= ym.ALIGN[layout]
        refused(img, width, height, lid, 0, "too short")
        img = image()
        img.line_count[p] -= 1
        refused(img, width, height, lid, 0, "too short")
        for off in range(1, ym.ALIGN[layout]):
            if ym.ALIGN[layout] % off == 0:                            # 1, and 2 where the alignment is 4
                img = image()
                img.data[p] = arrays[p].ctypes.data + off
                refused(img, width, height, lid, 0, "misaligned")
        if ym.ALIGN[layout] > 1:
            img = image()
            img.stride[p] += 1
            refused(img, width, height, lid, 0, "misaligned")
    if len(arrays) == 3:                        # a planar layout handed one plane: too few planes
        refused(image(1), width, height, lid, 0, "takes 3 planes, plane 1 is missing")
    else:
        img = image()
        img.data[0] = None
        refused(img, width, height, lid, 0, "takes 1 plane, plane 0 is missing")
    # a current window outside the buffer (export only reads it)
    frame.c.current_window = _lib.box2i.of(0, 0, width, height - 1)
    lib.cvs_clear_last_error()
    assert lib.cvs_subsample_422_dev(C.byref(image()), frame.ref(), width, height, lid, 0, None) == -1 and "outside the buffer" in _lib.last_error()
    assert all((a == 0xA5).all() for a in arrays), "a refused call wrote a plane"
    assert np.array_equal(frame.array, before), "a refused call wrote the frame"


# ---------------------------------------------------------------- the model: layouts

def _samples(rng, width, height, bits):
    top = 1 << bits
    return rng.integers(0, top, (height, width)), rng.integers(0, top, (height, width // 2)), rng.integers(0, top, (height, width // 2))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("width", [2, 4, 6, 8, 10, 12, 14, 382])
def test_pack_and_unpack_are_inverses(layout, width):
    """unpack(pack(x)) == x and, on buffers with padding, pack writes the least stride's bytes of `height` lines and no other."""
    rng = np.random.default_rng(width)
    height = 3
    y, cb, cr = _samples(rng, width, height, ym.BITS[layout])
    planes = ym.pack(layout, y, cb, cr)
    strides, lines = ym.least(layout, width, height)
    assert [p.shape for p in planes] == [(n, s) for n, s in zip(lines, strides)]
    for a, b in zip(ym.unpack(layout, planes, width, height), (y, cb, cr)):
        assert np.array_equal(a, b)
    wide = ym.pack(layout, y, cb, cr, [s + 4 * (k + 1) for k, s in enumerate(strides)], [n + k + 1 for k, n in enumerate(lines)], fill=0xA5)
    for p, q, s in zip(wide, planes, strides):
        assert np.array_equal(p[:height, :s], q) and (p[:height, s:] == 0xA5).all() and (p[height:] == 0xA5).all()
    for a, b in zip(ym.unpack(layout, wide, width, height), (y, cb, cr)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("width", [6, 12, 2, 8, 14, 4, 10, 16])
def test_v210_words_by_hand_unused_fields_and_upper_bits(width):
    """W mod 6 in {0, 2, 4}: the words of a group are what the layout's table says; a last group's fields beyond the width and
    bits 30-31 of every word come out as 0, and on the way in neither they nor garbage in them reaches a sample."""
    rng = np.random.default_rng(60 + width)
    y, cb, cr = _samples(rng, width, 2, 10)
    plane = ym.pack("v210", y, cb, cr)[0]
    groups = -(-width // 6)
    assert plane.shape == (2, 16 * groups)
    words = plane.view("<u4").reshape(2, groups, 4)
    assert not (words >> 30).any()
    yy, bb, rr = np.zeros((2, 6 * groups), np.int64), np.zeros((2, 3 * groups), np.int64), np.zeros((2, 3 * groups), np.int64)
    yy[:, :width], bb[:, :width // 2], rr[:, :width // 2] = y, cb, cr
    for g in range(groups):
        want = [(bb[:, 3 * g], yy[:, 6 * g], rr[:, 3 * g]), (yy[:, 6 * g + 1], bb[:, 3 * g + 1], yy[:, 6 * g + 2]),
                (rr[:, 3 * g + 1], yy[:, 6 * g + 3], bb[:, 3 * g + 2]), (yy[:, 6 * g + 4], rr[:, 3 * g + 2], yy[:, 6 * g + 5])]
        for k, (lo, mid, hi) in enumerate(want):
            assert np.array_equal(words[:, g, k], lo | (mid << 10) | (hi << 20)), (g, k)
    # garbage where the contract looks away: bits 30-31 everywhere, the whole of the fields beyond the width
    dirty = words.astype(np.uint32) | (rng.integers(0, 4, words.shape).astype(np.uint32) << 30)
    wy, wb, wr = ym.unpack("v210", [plane], width, 2, whole_groups=True)
    assert not wy[:, width:].any() and not wb[:, width // 2:].any() and not wr[:, width // 2:].any()
    if width % 6:
        full = 6 * groups
        gy, gb, gr = yy.copy(), bb.copy(), rr.copy()
        gy[:, width:], gb[:, width // 2:], gr[:, width // 2:] = rng.integers(0, 1024, (2, full - width)), rng.integers(0, 1024, (2, (full - width) // 2)), rng.integers(0, 1024, (2, (full - width) // 2))
        dirty = ym.pack("v210", gy, gb, gr)[0].view("<u4").reshape(2, groups, 4) | (dirty & np.uint32(0xC0000000))
        assert not np.array_equal(dirty & np.uint32(0x3FFFFFFF), words)
    dirty_plane = np.ascontiguousarray(dirty.astype("<u4")).view(np.uint8).reshape(2, -1)
    for a, b in zip(ym.unpack("v210", [dirty_plane], width, 2), (y, cb, cr)):
        assert np.array_equal(a, b)


def test_planar10_keeps_bits_0_to_9():
    rng = np.random.default_rng(3)
    y, cb, cr = _samples(rng, 8, 2, 10)
    planes = ym.pack("planar10", y, cb, cr)
    assert all(not (p[:, 1::2] >> 2).any() for p in planes)                    # bits 10-15 written as 0
    dirty = [p.copy() for p in planes]
    for p in dirty:
        p[:, 1::2] |= (rng.integers(1, 64, p[:, 1::2].shape) << 2).astype(np.uint8)
    for a, b in zip(ym.unpack("planar10", dirty, 8, 2), (y, cb, cr)):
        assert np.array_equal(a, b)
    assert not np.array_equal(ym.unpack("planar10", dirty, 8, 2, rules=dict(ym.RULES, mask=False))[0], y)


# ---------------------------------------------------------------- the model: arithmetic

def _solid(tables, rgbv):
    one = tables[2](np.array([1.0], F))[0]
    px = np.zeros((1, 4, 4), np.uint16)
    for i in range(3):
        px[..., i] = one if rgbv[i] else 0
    px[..., 3] = one
    return px


ANCHORS = {
    (8, "601"): {"white": (235, 128, 128), "black": (16, 128, 128), "red": (81, 90, 240), "green": (145, 54, 34), "blue": (41, 240, 110)},
    (8, "709"): {"white": (235, 128, 128), "black": (16, 128, 128), "red": (63, 102, 240), "green": (173, 42, 26), "blue": (32, 240, 118)},
    (10, "601"): {"white": (940, 512, 512), "black": (64, 512, 512), "red": (326, 361, 960), "green": (578, 215, 137), "blue": (164, 960, 439)},
    (10, "709"): {"white": (940, 512, 512), "black": (64, 512, 512), "red": (250, 409, 960), "green": (691, 167, 105), "blue": (127, 960, 471)},
}
COLOURS = {"white": (1, 1, 1), "black": (0, 0, 0), "red": (1, 0, 0), "green": (0, 1, 0), "blue": (0, 0, 1)}


@pytest.mark.parametrize("bits,matrix", sorted(ANCHORS))
def test_export_anchors(tables, bits, matrix):
    full = (0, 0, 3, 0)
    for name, want in ANCHORS[(bits, matrix)].items():
        y, cb, cr = ym.subsample_samples(_solid(tables, COLOURS[name]), full, full, 4, 1, bits, tables[1], matrix)
        assert (y == want[0]).all() and (cb == want[1]).all() and (cr == want[2]).all(), (name, y, cb, cr)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("matrix", ["601", "709"])
def test_import_anchors(tables, layout, matrix):
    """Legal black and white come out as the table's 0.0 and 1.0, alpha as its 1.0."""
    dec, _enc, f2h = tables
    s = 1 << (ym.BITS[layout] - 8)
    one = f2h(np.array([1.0], F))[0]
    for luma, want in ((16 * s, dec[0]), (235 * s, dec[one])):
        planes = ym.pack(layout, np.full((2, 6), luma), np.full((2, 3), 128 * s), np.full((2, 3), 128 * s))
        got = ym.reconstruct_model(layout, planes, 6, 2, dec, f2h, matrix)
        assert (got[..., :3] == want).all() and (got[..., 3] == dec[one]).all()
    assert dec[0] == 0 and np.float16(dec[one:one + 1].view(np.float16)[0]) == np.float16(1.0)


def test_the_generic_encode_is_the_mpeg2_models_for_rec601(tables):
    rng = np.random.default_rng(9)
    px = rng.integers(0, 0x3C01, (3, 8, 4), dtype=np.uint16)
    ym.RGB_MATRICES["probe"] = ym.RGB_MATRICES["601"]
    try:
        for a, b in zip(ym.encode(px, tables[1], "probe"), ym.encode(px, tables[1], "601")):
            assert np.array_equal(a, b)
    finally:
        del ym.RGB_MATRICES["probe"]


def test_edges_clamp(tables):
    dec, enc, f2h = tables
    # import: the last odd column averages chroma column W/2 - 1 with itself
    planes = ym.pack("planar8", np.full((1, 4), 128), np.array([[128, 240]]), np.full((1, 2), 128))
    r, g, b = ym.rgb("planar8", planes, 4, 1)
    assert b[0, 3] == b[0, 2] and b[0, 1] != b[0, 0]
    # export: column -1 reads column 0, so a flat row stays flat in chroma
    e = np.full((1, 6), F(0.25))
    assert (ym.filter_chroma(e) == F(0.25)).all()
    assert ym.filter_chroma(e, dict(ym.RULES, left_clamp=False))[0, 0] == F(0.1875)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("matrix", ["601", "709"])
def test_model_against_a_float64_restatement_import(tables, layout, matrix):
    """The model's halves before the table against the contract restated in float64: a horizontal average between even-column
    samples and a matrix product.  Only the rounding differs: every truncated half lies within one half ulp of the float64 value."""
    rng = np.random.default_rng(41)
    width, height, bits = 22, 5, ym.BITS[layout]
    s = 1 << (bits - 8)
    y, cb, cr = _samples(rng, width, height, bits)
    planes = ym.pack(layout, y, cb, cr)
    got = ym.reconstruct_halves(layout, planes, width, height, tables[2], matrix)[..., :3].view(np.float16).astype(np.float64)
    yf = (y.astype(np.float64) - 16 * s) / (219 * s)
    chroma = []
    for c in (cb, cr):
        v = (c.astype(np.float64) - 128 * s) / (224 * s)
        h = np.empty((height, width))
        h[:, 0::2] = v
        h[:, 1::2] = (v + np.concatenate([v[:, 1:], v[:, -1:]], axis=1)) / 2
        chroma.append(h)
    m = np.array(ym.MATRICES[matrix])
    want = np.stack([m[i, 0] * yf + m[i, 1] * chroma[0] + m[i, 2] * chroma[1] for i in range(3)], axis=-1)
    ulp = np.maximum(np.abs(want), 2.0 ** -14) * 2.0 ** -10
    assert (np.abs(got - want) <= ulp * 1.001).all()


@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("matrix", ["601", "709"])
def test_model_against_a_float64_restatement_export(tables, bits, matrix):
    """The same for the export edge: the codes against float64 arithmetic on the table's values.  float32 rounding can move a
    value across a rounding boundary only where it lies within a few 1e-7 of one: no code differs by more than one, and fewer
    than one in a hundred differ at all (a code's step is 1e-3 of the range or more)."""
    rng = np.random.default_rng(43)
    width, height = 64, 16
    full = (0, 0, width - 1, height - 1)
    px = rng.integers(0, 0x3C01, (height, width, 4), dtype=np.uint16)
    got = ym.subsample_samples(px, full, full, width, height, bits, tables[1], matrix)
    rgbv = [tables[1][px[..., c]].view(np.float16).astype(np.float64) for c in range(3)]
    m = np.array(ym.RGB_MATRICES[matrix])
    yv, cbv, crv = (m[i, 0] * rgbv[0] + m[i, 1] * rgbv[1] + m[i, 2] * rgbv[2] for i in range(3))
    s, top = 1 << (bits - 8), (1 << bits) - 1
    k = np.arange(width // 2)

    def filt(e):
        return 0.25 * e[:, np.maximum(2 * k - 1, 0)] + 0.5 * e[:, 2 * k] + 0.25 * e[:, 2 * k + 1]

    def quant(v, scale, offset):
        code = np.rint(np.clip(v * scale * s / top + offset * s / top, 0, 1) * top)
        return np.clip(code, 4, 1019) if bits == 10 else code
    want = quant(yv, 219, 16), quant(filt(cbv), 224, 128), quant(filt(crv), 224, 128)
    for a, b in zip(got, want):
        d = np.abs(a - b)
        assert d.max() <= 1 and (d != 0).mean() < 0.01, (d.max(), (d != 0).mean())


# ---------------------------------------------------------------- the two cross-checks against the MPEG-2 models

def test_vertical_weights_sum_exactly_for_every_8_bit_code():
    """0.75 c + 0.25 c == c in float32 for the decoded value of every 8-bit chroma code: the progressive MPEG-2 reconstruction's
    vertical filter is the identity on chroma that is constant along columns, which the next test relies on."""
    c = (np.arange(256).astype(F) - F(128.0)) / F(224.0)
    assert np.array_equal(c * F(0.75) + c * F(0.25), c)


@pytest.mark.parametrize("matrix", ["601", "709"])
def test_planar8_import_is_the_progressive_mpeg2_import_on_chroma_constant_along_columns(tables, matrix):
    """PLANAR8 planes whose Cb and Cr are constant along columns give byte for byte what the MPEG-2 reconstruction's model gives,
    progressive, on the 4:2:0 planes that take one chroma row per row pair."""
    rng = np.random.default_rng(47)
    width, height = 26, 8
    y = rng.integers(0, 256, (height, width), dtype=np.uint8)
    cb = np.repeat(rng.integers(0, 256, (1, width // 2), dtype=np.uint8), height, 0)
    cr = np.repeat(rng.integers(0, 256, (1, width // 2), dtype=np.uint8), height, 0)
    got = ym.reconstruct_model("planar8", [y, cb, cr], width, height, tables[0], tables[2], matrix)
    want = mpeg2_reconstruct_model([y, cb[0::2], cr[0::2]], width, height, tables[0], tables[2], interlaced=False, matrix=matrix)
    assert np.array_equal(got, want)


def test_planar8_rec601_export_luma_is_the_mpeg2_exports(tables):
    from tests.entry_cases import px16
    full, cur = (-2, -1, 29, 9), (1, 0, 27, 7)
    width, height = 28, 8
    frame = px16(np.random.default_rng(49), full, cur)
    y, _cb, _cr = ym.subsample_samples(frame.array, full, cur, width, height, 8, tables[1], "601")
    want = mpeg2_subsample_model(frame.array, full, cur, width, height, tables[1])[0]
    assert np.array_equal(y, want)


# ---------------------------------------------------------------- the round trip: samples -> import -> export

def _round_trip(tables, layout, matrix, y, cb, cr):
    dec, enc, f2h = tables
    height, width = y.shape
    full = (0, 0, width - 1, height - 1)
    frame = ym.reconstruct_model(layout, ym.pack(layout, y, cb, cr), width, height, dec, f2h, matrix)
    return ym.subsample_samples(frame, full, full, width, height, ym.BITS[layout], enc, matrix)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("matrix", ["601", "709"])
def test_round_trip_of_every_legal_grey_code(tables, layout, matrix):
    """8-bit: every byte comes back.  10-bit: luma within one code (about 41 % of the codes are off by one: the truncation to a
    half's 11-bit significand), chroma exactly."""
    s = 1 << (ym.BITS[layout] - 8)
    codes = np.arange(16 * s, 235 * s + 1)
    width = 2 * ((len(codes) + 1) // 2)
    y = np.resize(codes, (1, width))
    cb = np.full((1, width // 2), 128 * s)
    y2, cb2, cr2 = _round_trip(tables, layout, matrix, y, cb, cb.copy())
    assert np.array_equal(cb2, cb) and np.array_equal(cr2, cb)
    d = np.abs(y2 - y)
    if s == 1:
        assert d.max() == 0
    else:
        assert d.max() == 1 and 0.35 < (d != 0).mean() < 0.47, (d.max(), (d != 0).mean())


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("matrix", ["601", "709"])
def test_round_trip_of_flat_in_gamut_colours(tables, layout, matrix):
    """400 colours with flat chroma, Y' in [60s, 200s), Cb and Cr in [118s, 138s): in gamut, so no clamp takes part."""
    s = 1 << (ym.BITS[layout] - 8)
    rng = np.random.default_rng(53)
    n, width = 400, 6
    y = np.repeat(rng.integers(60 * s, 200 * s, (n, 1)), width, 1)
    cb = np.repeat(rng.integers(118 * s, 138 * s, (n, 1)), width // 2, 1)
    cr = np.repeat(rng.integers(118 * s, 138 * s, (n, 1)), width // 2, 1)
    r, g, b = ym.rgb(layout, ym.pack(layout, y, cb, cr), width, n, matrix)
    assert min(r.min(), g.min(), b.min()) >= 0 and max(r.max(), g.max(), b.max()) <= 1
    y2, cb2, cr2 = _round_trip(tables, layout, matrix, y, cb, cr)
    assert np.array_equal(cb2, cb) and np.array_equal(cr2, cr)
    assert np.abs(y2 - y).max() == (0 if s == 1 else 1)


# ---------------------------------------------------------------- the catalogue

def test_the_device_entries_of_the_header_have_their_catalogue_cases():
    """Every case calls ONE of the header's two entries, once, handing it the factory's stream; asks for the same operands every
    time; the planes are buffers of class "plane" (8-bit) or "bytes" (10-bit) and the frame a frame; one output frame, or every
    plane an output.  Both entries are called by every layout's group."""
    from tests.test_entry_cases_cpu import HostOnly, Recorder
    _funcs, entries = _declared(HEADER)
    assert entries == sorted(yc.ENTRIES)
    names, stream = [], 0x5EED
    for (gid, build), layout in zip(yc.GROUPS, LAYOUTS):
        rec, called = Recorder(), set()
        for (what, case), spec in zip(build(rec), yc.specs(layout)):
            assert what == yc.name(spec)
            before = len(rec.calls)
            fac = HostOnly(rec, stream)
            assert case(fac) == 0
            made = rec.calls[before:]
            assert len(made) == 1 and made[0] == ("cvs_%s_422_dev" % spec["direction"], stream), (gid, what, made)
            called.add(made[0][0])
            names.append(what)
            again = HostOnly(rec, stream)
            case(again)
            shape = lambda f: [(o.cls, o.name, o.out, o.cmp, o.nbytes, o.row_bytes, o.reads) for o in f.objects]
            assert shape(fac) == shape(again), (gid, what)
            frames = [o for o in fac.objects if o.frame is not None]
            planes = [o for o in fac.objects if o.frame is None]
            assert len(frames) == 1 and len(planes) == ym.PLANES[layout]
            assert all(o.cls == ("plane" if ym.BITS[layout] == 8 else "bytes") for o in planes)
            assert [o.nbytes for o in planes] == [n * s for n, s in zip(spec["lines"], spec["strides"])]
            if spec["direction"] == "reconstruct":
                assert frames[0].out and not any(o.out for o in planes) and fac.objects[-1] is frames[0]
            else:
                assert not frames[0].out and all(o.out for o in planes) and fac.objects[0] is frames[0]
            assert all(s % ym.ALIGN[layout] == 0 for s in spec["strides"])
        assert called == set(yc.ENTRIES), gid
    assert len(names) == len(set(names))


def test_the_catalogue_has_the_shapes_that_can_go_wrong():
    for layout in LAYOUTS:
        specs = yc.specs(layout)
        run = 63 * yc.LANE_PIXELS[layout]
        for direction in ("reconstruct", "subsample"):
            mine = [s for s in specs if s["direction"] == direction]
            assert {2, 4, 6, 8, 10, 14, run - 2, run, run + 2, 2 * run + 2} <= {s["width"] for s in mine}
            assert {1, 2, 3, 5} <= {s["height"] for s in mine}
            assert {"601", "709"} == {s["matrix"] for s in mine}
            least = [ym.least(layout, s["width"], s["height"]) for s in mine]
            assert any(s["strides"] == l[0] and s["lines"] == l[1] for s, l in zip(mine, least))
            assert any(s["strides"][0] > l[0][0] for s, l in zip(mine, least)) and any(s["lines"][0] > l[1][0] for s, l in zip(mine, least))
            boxes = [(s["full"], s["width"], s["height"]) for s in mine]
            assert any(f == (0, 0, w - 1, h - 1) for f, w, h in boxes)                                    # the raster's own
            assert any(f[0] < 0 and f[1] < 0 and f[2] >= w and f[3] >= h for f, w, h in boxes)              # larger
            assert any(f[0] > 0 and f[2] < w - 1 for f, w, h in boxes)                                     # inside
            assert any(f[0] < 0 and f[2] < w - 1 for f, w, h in boxes)                                     # partly off, negative origin


@pytest.mark.parametrize("rule", sorted(ym.RULES))
def test_the_catalogue_exercises_every_rule(orc, rule):
    """For each rule of the contract at least one case's expected output changes when the model is run with that rule altered:
    a catalogue none of whose expectations moves would let a kernel without the rule pass.  On the model alone."""
    altered = dict(ym.RULES, **{rule: False})
    moved = []
    for layout in LAYOUTS:
        for spec in yc.specs(layout):
            a, b = yc.expected(spec, orc), yc.expected(spec, orc, altered)
            if spec["direction"] == "reconstruct":
                same = np.array_equal(a[0], b[0])
            else:
                same = all(np.array_equal(p, q) for p, q in zip(a, b))
            if not same:
                moved.append((layout, spec["direction"]))
    assert moved, rule
    by_rule = {"right_clamp": "reconstruct", "left_clamp": "subsample", "sdi_clamp": "subsample", "black_outside": "subsample"}
    if rule in by_rule:
        assert {d for _l, d in moved} == {by_rule[rule]}, moved
    if rule in ("right_clamp", "left_clamp", "matrix", "black_outside"):
        assert {l for l, _d in moved} == set(LAYOUTS), moved                 # every layout's own cases exercise it
    if rule == "matrix":
        assert {d for _l, d in moved} == {"reconstruct", "subsample"}
    if rule == "partial_group":
        assert set(moved) == {("v210", "reconstruct"), ("v210", "subsample")}, moved
    if rule == "mask":
        assert set(moved) == {("planar10", "reconstruct"), ("v210", "reconstruct")}, moved
    if rule == "sdi_clamp":
        assert {l for l, _d in moved} == {"planar10", "v210"}, moved


# ---------------------------------------------------------------- the nodes, as far as they go without a device

@pytest.fixture(scope="module")
def process():
    from fluggo.media import process
    return process


def _coded_source(process):
    class Planes(process.CodedImageSource):
        def get_frame(self, frame):
            return [process.CodedImage(bytearray(64 * 4), 64, 4)]
    return Planes()


def test_node_surface(process):
    from fluggo.media.basetypes import v2i
    src, solid = _coded_source(process), process.SolidColorVideoSource((0.2, 0.3, 0.4, 1.0))
    R, S = process.YCbCr422ReconstructionFilter, process.YCbCr422SubsampleFilter
    assert issubclass(R, process.VideoSource) and issubclass(S, process.CodedImageSource)
    assert type(R(src, (16, 4))._video_frame_source_funcs).__name__ == "PyCapsule"
    assert type(S(solid, (16, 4))._coded_image_source_funcs).__name__ == "PyCapsule"
    for layout in LAYOUTS:
        for matrix in ("601", "709"):
            R(src, v2i(1920, 1080), layout, matrix)
            S(source=solid, size=(1920, 1), layout=layout, matrix=matrix)
    R(src, size=(2, 1))
    S(solid, size=(3840, 2161), layout="uyvy")


def test_nodes_refuse_bad_sources_sizes_layouts_and_matrices(process):
    src, solid = _coded_source(process), process.SolidColorVideoSource((0.2, 0.3, 0.4, 1.0))
    for node, good, bad in ((process.YCbCr422ReconstructionFilter, src, solid), (process.YCbCr422SubsampleFilter, solid, src)):
        with pytest.raises(Exception):
            node(bad, (16, 4))
        with pytest.raises(Exception):
            node(object(), (16, 4))
        with pytest.raises(TypeError):
            node(good)                                                            # no default raster
        for size in [(721, 486), (0, 4), (16, 0), (-2, 4), (1, 1), (16, -1)]:
            with pytest.raises(ValueError):
                node(good, size)
        for layout in ["yuv422p", "V210", "", 3, None, b"v210"]:
            with pytest.raises(ValueError):
                node(good, (16, 4), layout=layout)
        for matrix in ["2020", "", "rec709", 601, 709, None, b"601"]:
            with pytest.raises(ValueError):
                node(good, (16, 4), matrix=matrix)


def test_a_pull_gives_the_raster_or_without_a_gpu_is_empty_or_loud(process):
    from canvas_amd import _lib
    from fluggo.media.basetypes import box2i
    node = process.YCbCr422ReconstructionFilter(_coded_source(process), size=(16, 4), layout="uyvy")
    try:
        frame = node.get_frame_f16(0, box2i(0, 0, 15, 3))
    except Exception:
        assert _lib.load().cvs_device_count() == 0
        return
    if _lib.load().cvs_device_count() > 0:
        assert not frame.current_window.empty()
    else:
        assert frame.current_window.empty()
        assert process.last_error()
