"""The 4:2:0 Y'CbCr edges without a GPU (DESIGN.md "4:2:0 Y'CbCr edges"): include/canvas_ycc420.h against the library and its
bindings; cvs_ycc420_layout, which is host only; every refusal of the two device entries by its message (they all come before the
device is touched, so host memory stands in for the operands and is seen to stay as it was); the numpy model
(tests/ycc420_model.py) on hand-worked values for every siting's weights at the first, an interior and the last row and column,
on studio- and full-range anchors, against the MPEG-2 progressive import's model and against the layouts' equivalences; the
round-trip facts DESIGN states; the catalogue of tests/ycc420_cases.py, which must exercise every rule of the contract; the built
code objects; the nodes' arguments."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import ycc420_cases as yc
from tests import ycc420_model as ym
from tests.mpeg2_reconstruct_model import reconstruct_model as mpeg2_reconstruct_model
from tests.test_perspective_cpu import _declared
from tests.test_unsharp_cpu import _kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "canvas_ycc420.h"
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
    assert funcs == sorted(_lib.YCC420_SIGNATURES) == ["cvs_reconstruct_420_dev", "cvs_subsample_420_dev", "cvs_ycc420_layout"]
    assert entries == sorted(yc.ENTRIES)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name, (res, args) in _lib.YCC420_SIGNATURES.items():
        assert name in exported and getattr(lib, name).argtypes == args and getattr(lib, name).restype is res, name
    others = (set(_lib.SIGNATURES) | set(_lib.SCOPE_SIGNATURES) | set(_lib.LUT3D_SIGNATURES) | set(_lib.PERSPECTIVE_SIGNATURES) | set(_lib.DEINTERLACE_SIGNATURES)
              | set(_lib.MEDIAN_SIGNATURES) | set(_lib.TEMPORAL_SIGNATURES) | set(_lib.YCC422_SIGNATURES) | set(_lib.PRIMARY_SIGNATURES))
    assert not set(_lib.YCC420_SIGNATURES) & others
    hip_h = open(os.path.join(ROOT, "include", "canvas_hip.h")).read()
    assert "cvs_reconstruct_420" not in hip_h and "NV12" not in hip_h and "REC2020" not in hip_h          # the entries live in the new header
    assert (_lib.YCC420_PLANAR8, _lib.YCC420_PLANAR10, _lib.YCC420_NV12, _lib.YCC420_P010) == tuple(ym.LAYOUTS[n] for n in LAYOUTS) == (0, 1, 2, 3)
    assert (_lib.YCC_REC709, _lib.YCC_REC2020, _lib.YCC_FULL_RANGE, _lib.YCC_SITING_CENTER, _lib.YCC_SITING_TOPLEFT, _lib.YCC_NO_TRANSFER) == (
        ym.MATRIX_FLAGS["709"], ym.MATRIX_FLAGS["2020"], ym.RANGE_FLAGS["full"], ym.SITING_FLAGS["center"], ym.SITING_FLAGS["topleft"], ym.TRANSFER_FLAGS["none"])
    # one launcher per direction, one arithmetic flavour
    symbols = subprocess.run(["nm", _lib.LIB_PATH], stdout=subprocess.PIPE, text=True).stdout
    for name in ("cvk_ycc420_reconstruct", "cvk_ycc420_subsample"):
        assert (" " + name + "\n") in symbols and name + "_fma" not in symbols, name


def test_the_header_compiles_as_c_and_as_cpp():
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "t.c")
        with open(src, "w") as f:
            f.write('#include "%s"\nint main(void) { return CVS_420_PLANAR8 == 0 && CVS_420_PLANAR10 == 1 && CVS_420_NV12 == 2 && CVS_420_P010 == 3 && '
                    'CVS_YCC_PROGRESSIVE == 1 && CVS_YCC_REC709 == 2 && CVS_YCC_REC2020 == 4 && CVS_YCC_FULL_RANGE == 8 && CVS_YCC_SITING_CENTER == 16 && '
                    'CVS_YCC_SITING_TOPLEFT == 32 && CVS_YCC_NO_TRANSFER == 64 ? 0 : 1; }\n' % HEADER)
        for cc, std, lang in (("gcc", "-std=c99", "c"), ("g++", "-std=c++14", "c++")):
            exe = os.path.join(tmp, "t_" + cc)
            subprocess.run([cc, std, "-Wall", "-Werror", "-x", lang, src, "-I", os.path.join(ROOT, "include"), "-o", exe], check=True)
            assert subprocess.run([exe]).returncode == 0


@pytest.mark.parametrize("obj,kernel", [("ycc420_recon_ops.hip.o", "k_ycc420_reconstruct"), ("ycc420_ops.hip.o", "k_ycc420_subsample")])
def test_code_objects_hold_the_twelve_instances_without_scratch(obj, kernel):
    """One build for both arithmetic flavours; four layouts x (table in LDS, table in L2, no table); range, matrix and siting are
    arguments, not instances; no private segment, no spills."""
    assert os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"), "the ROCm LLVM tools the build itself needs are missing"
    found = _kernels(obj)
    assert len(found) == 12 and all(kernel in n for n in found), sorted(found)
    for layout in range(4):
        for table, lanes in ((0, 1024), (1, 256), (2, 256)):
            assert any("%sILi%dELi%dELi%dEEE" % (kernel, layout, table, lanes) in n for n in found), (layout, table, sorted(found))
    for name, (scratch, spills) in found.items():
        assert scratch == 0 and spills == 0, (name, scratch, spills)
    assert not os.path.exists(os.path.join(ROOT, "canvas_amd", "csrc", "build", obj.replace(".hip.o", ".fma.hip.o")))


# ---------------------------------------------------------------- cvs_ycc420_layout (host only)

def _layout(lib, layout, width, height):
    strides, lines = (C.c_int * 3)(-7, -7, -7), (C.c_int * 3)(-7, -7, -7)
    lib.cvs_clear_last_error()
    return lib.cvs_ycc420_layout(layout, width, height, strides, lines), list(strides), list(lines)


def test_layout_values(lib):
    for width, height in [(2, 2), (4, 6), (6, 2), (8, 4), (10, 10), (14, 2), (720, 486), (1920, 1080), (3840, 2160), (4096, 2160), (7680, 4320)]:
        w2, h2 = width // 2, height // 2
        assert _layout(lib, 0, width, height) == (3, [width, w2, w2], [height, h2, h2])
        assert _layout(lib, 1, width, height) == (3, [2 * width, width, width], [height, h2, h2])
        assert _layout(lib, 2, width, height) == (2, [width, width, 0], [height, h2, 0])
        assert _layout(lib, 3, width, height) == (2, [2 * width, 2 * width, 0], [height, h2, 0])
        for name in LAYOUTS:
            strides, lines = ym.least(name, width, height)
            planes, s, n = _layout(lib, ym.LAYOUTS[name], width, height)
            assert planes == ym.PLANES[name] == len(strides) and s[:planes] == strides and n[:planes] == lines
    # either array may be left out
    assert lib.cvs_ycc420_layout(2, 1920, 1080, None, None) == 2


def test_layout_refusals(lib):
    from canvas_amd import _lib
    for layout, width, height, word in [(-1, 16, 16, "layout"), (4, 16, 16, "layout"), (99, 16, 16, "layout"), (0, 0, 16, "width"), (1, 1, 16, "width"),
                                        (2, 15, 16, "width"), (3, 721, 486, "width"), (3, -6, 4, "width"), (0, 16, 0, "height"), (3, 16, -2, "height"),
                                        (2, 16, 1, "height"), (0, 16, 7, "height"), (1, 2 ** 30, 2, "width")]:
        rc, strides, lines = _layout(lib, layout, width, height)
        assert rc == -1 and strides == [-7] * 3 and lines == [-7] * 3, (layout, width, height)
        assert "cvs_ycc420_layout" in _lib.last_error() and word in _lib.last_error(), _lib.last_error()


# ---------------------------------------------------------------- the refusals: before the device is touched, nothing written

def _host_image(layout, width, height):
    from canvas_amd import _lib
    strides, lines = ym.least(layout, width, height)
    arrays = [np.full(s * n + 64, 0xA5, np.uint8) for s, n in zip(strides, lines)]
    # (numpy's allocations are aligned well beyond 2)
    assert all(a.ctypes.data % 16 == 0 for a in arrays)

    def image(keep=None):
        img = _lib.coded_image()
        for p, (a, s, n) in enumerate(zip(arrays, strides, lines)):
            img.data[p], img.stride[p], img.line_count[p] = a.ctypes.data, s, n
        return img
    return arrays, strides, lines, image


@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_refusal_by_its_message_and_nothing_is_written(lib, layout):
    from canvas_amd import _lib
    from canvas_amd.abi import HostFrame
    from tests.entry_cases import SENT16
    width, height, lid = 24, 4, ym.LAYOUTS[layout]
    full = (0, 0, width - 1, height - 1)
    arrays, strides, lines, good = _host_image(layout, width, height)
    before = np.broadcast_to(SENT16, (height, width, 4)).copy()
    frame = HostFrame(full, np.uint16, before.copy(), full)
    lim = _lib.MAX_COORD

    def refused(img, w, h, lay, flags, word, entries=("reconstruct", "subsample"), fr=frame):
        for entry in entries:
            if fr is not None:
                fr.c.current_window = _lib.box2i.of(*full)
            lib.cvs_clear_last_error()
            ref = fr.ref() if fr is not None else None
            if entry == "reconstruct":
                rc = lib.cvs_reconstruct_420_dev(ref, C.byref(img) if img is not None else None, w, h, lay, flags, None)
                assert fr is None or fr.current_window.is_empty(), (entry, word)
            else:
                rc = lib.cvs_subsample_420_dev(C.byref(img) if img is not None else None, ref, w, h, lay, flags, None)
            assert rc == -1 and word in _lib.last_error(), (entry, word, rc, _lib.last_error())
            assert ("4:2:0 " + entry in _lib.last_error()) or ("cvs_%s_420_dev" % entry in _lib.last_error()), _lib.last_error()

    refused(good(), width, height, lid, 0, "need a frame", fr=None)
    refused(None, width, height, lid, 0, "need an image")
    for w in (23, 25, 1, 0, -2):
        refused(good(), w, height, lid, 0, "must be even and at least 2")
    for h in (0, -2, 1, 3, 5):
        refused(good(), width, h, lid, 0, "must be even and at least 2")
    for flags in (_lib.YCC_PROGRESSIVE, _lib.YCC_PROGRESSIVE | _lib.YCC_REC709, 128, 256, 1 << 20, -1):
        refused(good(), width, height, lid, flags, "unknown flags")
    refused(good(), width, height, lid, _lib.YCC_REC709 | _lib.YCC_REC2020, "two matrices")
    refused(good(), width, height, lid, _lib.YCC_SITING_CENTER | _lib.YCC_SITING_TOPLEFT | _lib.YCC_FULL_RANGE, "two sitings")
    for lay in (-1, 4, 17):
        refused(good(), width, height, lay, 0, "unknown layout")
    for p in range(len(arrays)):
        img = good()
        img.data[p] = None
        refused(img, width, height, lid, 0, "plane %d is missing" % p)
        img = good()
        img.stride[p] -= ym.ALIGN[layout]
        refused(img, width, height, lid, 0, "too short")
        img = good()
        img.line_count[p] -= 1
        refused(img, width, height, lid, 0, "too short")
        if ym.ALIGN[layout] > 1:
            img = good()
            img.data[p] = arrays[p].ctypes.data + 1
            refused(img, width, height, lid, 0, "misaligned")
            img = good()
            img.stride[p] += 1
            refused(img, width, height, lid, 0, "misaligned")
    # a semi-planar layout's image handed to a planar layout and the other way round: the third plane is missing, or not looked at
    if ym.PLANES[layout] == 3:
        img = good()
        img.data[2] = None
        refused(img, width, height, lid, 0, "takes 3 planes")
    # coordinates beyond the bound
    for box in ((0, 0, lim + 1, 3), (-lim - 1, 0, 3, 3)):
        far = HostFrame((0, 0, 0, 0), np.uint16, np.zeros((1, 1, 4), np.uint16), (0, 0, -1, -1))
        far.c.full_window = _lib.box2i.of(*box)
        for entry in ("reconstruct", "subsample"):
            far.c.current_window = _lib.box2i.of(0, 0, -1, -1)
            lib.cvs_clear_last_error()
            if entry == "reconstruct":
                rc = lib.cvs_reconstruct_420_dev(far.ref(), C.byref(good()), width, height, lid, 0, None)
            else:
                rc = lib.cvs_subsample_420_dev(C.byref(good()), far.ref(), width, height, lid, 0, None)
            assert rc == -1 and "beyond" in _lib.last_error() and "cvs_%s_420_dev" % entry in _lib.last_error(), _lib.last_error()
    # export: a current window outside the buffer
    frame.c.current_window = _lib.box2i.of(0, 0, width, height - 1)
    lib.cvs_clear_last_error()
    assert lib.cvs_subsample_420_dev(C.byref(good()), frame.ref(), width, height, lid, 0, None) == -1 and "outside the buffer" in _lib.last_error()
    assert all((a == 0xA5).all() for a in arrays), "a refused call wrote a plane"
    assert np.array_equal(frame.array, before), "a refused call wrote the frame"


# ---------------------------------------------------------------- the model: layouts

def _samples(rng, width, height, bits):
    top = 1 << bits
    return rng.integers(0, top, (height, width)), rng.integers(0, top, (height // 2, width // 2)), rng.integers(0, top, (height // 2, width // 2))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("width", [2, 6, 14, 254])
def test_pack_and_unpack_are_inverses(layout, width):
    """unpack(pack(x)) == x and, on buffers with padding, pack writes the least stride's bytes of each plane's lines and no other."""
    rng = np.random.default_rng(width)
    height = 6
    y, cb, cr = _samples(rng, width, height, ym.BITS[layout])
    planes = ym.pack(layout, y, cb, cr)
    strides, lines = ym.least(layout, width, height)
    assert [p.shape for p in planes] == [(n, s) for n, s in zip(lines, strides)]
    for a, b in zip(ym.unpack(layout, planes, width, height), (y, cb, cr)):
        assert np.array_equal(a, b)
    wide = ym.pack(layout, y, cb, cr, [s + 4 * (k + 1) for k, s in enumerate(strides)], [n + k + 1 for k, n in enumerate(lines)], fill=0xA5)
    for p, q, s, n in zip(wide, planes, strides, lines):
        assert np.array_equal(p[:n, :s], q) and (p[:n, s:] == 0xA5).all() and (p[n:] == 0xA5).all()
    for a, b in zip(ym.unpack(layout, wide, width, height), (y, cb, cr)):
        assert np.array_equal(a, b)


def test_the_layouts_by_hand():
    y = np.array([[1, 2], [3, 4]])
    cb, cr = np.array([[5]]), np.array([[6]])
    assert [p.tolist() for p in ym.pack("planar8", y, cb, cr)] == [[[1, 2], [3, 4]], [[5]], [[6]]]
    assert [p.tolist() for p in ym.pack("nv12", y, cb, cr)] == [[[1, 2], [3, 4]], [[5, 6]]]
    y10, b10, r10 = y + 0x300, cb + 0x200, cr + 0x100
    assert [p.tolist() for p in ym.pack("planar10", y10, b10, r10)] == [[[1, 3, 2, 3], [3, 3, 4, 3]], [[5, 2]], [[6, 1]]]
    # P010: the code in bits 6-15: 0x301 << 6 = 0xC040
    assert [p.tolist() for p in ym.pack("p010", y10, b10, r10)] == [[[0x40, 0xC0, 0x80, 0xC0], [0xC0, 0xC0, 0x00, 0xC1]], [[0x40, 0x81, 0x80, 0x41]]]


def test_the_ignored_bits_of_the_10_bit_layouts():
    rng = np.random.default_rng(3)
    y, cb, cr = _samples(rng, 8, 4, 10)
    for layout, dirt_shift, width in (("planar10", 10, 6), ("p010", 0, 6)):
        planes = ym.pack(layout, y, cb, cr)
        words = [p.view("<u2") for p in planes]
        assert all(not ((w >> dirt_shift) & 0x3F).any() for w in words)                  # written as 0
        dirty = [np.ascontiguousarray((w | (rng.integers(1, 64, w.shape).astype(np.uint16) << dirt_shift)).astype("<u2")).view(np.uint8) for w in words]
        for a, b in zip(ym.unpack(layout, dirty, 8, 4), (y, cb, cr)):
            assert np.array_equal(a, b)
        assert not np.array_equal(ym.unpack(layout, dirty, 8, 4, rules=dict(ym.RULES, mask=False))[0], y)


# ---------------------------------------------------------------- the model: weights by hand

def test_import_vertical_weights_by_hand():
    """Six luma rows over three chroma rows 8, 16, 32: the first row, an interior pair and the last row of every siting."""
    p = np.array([[8.0], [16.0], [32.0]], F)
    left = ym.vertical(p, "left")[:, 0].tolist()
    assert left == [8.0, 0.75 * 8 + 0.25 * 16, 0.75 * 16 + 0.25 * 8, 0.75 * 16 + 0.25 * 32, 0.75 * 32 + 0.25 * 16, 32.0] == [8.0, 10.0, 14.0, 20.0, 28.0, 32.0]
    assert ym.vertical(p, "center")[:, 0].tolist() == left
    assert ym.vertical(p, "topleft")[:, 0].tolist() == [8.0, 12.0, 16.0, 24.0, 32.0, 32.0]
    # height 2: both clamps meet in one chroma row
    one = np.array([[5.0]], F)
    for siting in ym.SITING_FLAGS:
        assert ym.vertical(one, siting)[:, 0].tolist() == [5.0, 5.0]


def test_import_horizontal_weights_by_hand():
    v = np.array([[8.0, 16.0, 32.0]], F)
    left = ym.horizontal(v, "left")[0].tolist()
    assert left == [8.0, 12.0, 16.0, 24.0, 32.0, 32.0]
    assert ym.horizontal(v, "topleft")[0].tolist() == left
    assert ym.horizontal(v, "center")[0].tolist() == [8.0, 10.0, 14.0, 20.0, 28.0, 32.0]
    one = np.array([[5.0]], F)
    for siting in ym.SITING_FLAGS:
        assert ym.horizontal(one, siting)[0].tolist() == [5.0, 5.0]


def test_export_weights_by_hand():
    """E = 16 * row + column over 6 x 6: every siting's first, interior and last block."""
    e = (16.0 * np.arange(6)[:, None] + np.arange(6)[None, :]).astype(F)
    # left: V = mean of rows 2c, 2c+1 = 8 + 32c + x; C = V(2k) - 0.25 + 0.25 = ... at k = 0 column -1 reads column 0: 0.25*0 + 0.5*0 + 0.25*1
    v0 = 8.0
    assert ym.filter_chroma(e, "left").tolist() == [[v0 + 32 * c + (0.25 if k == 0 else 2 * k) for k in range(3)] for c in range(3)]
    assert ym.filter_chroma(e, "center").tolist() == [[v0 + 32 * c + 2 * k + 0.5 for k in range(3)] for c in range(3)]
    # top-left: V = 0.25 E(2c-1) + 0.5 E(2c) + 0.25 E(2c+1) = 32c + x (row -1 reading row 0 at c = 0: 0.25 * 16 = 4)
    assert ym.filter_chroma(e, "topleft").tolist() == [[(4.0 if c == 0 else 32 * c) + (0.25 if k == 0 else 2 * k) for k in range(3)] for c in range(3)]
    flat = np.full((2, 2), F(0.25))
    for siting in ym.SITING_FLAGS:
        assert ym.filter_chroma(flat, siting).tolist() == [[0.25]]
    assert ym.filter_chroma(flat, "left", dict(ym.RULES, left_clamp=False)).tolist() == [[0.1875]]
    assert ym.filter_chroma(flat, "topleft", dict(ym.RULES, top_clamp=False, left_clamp=True)).tolist() == [[0.1875]]


def test_decode_and_quantise_by_hand():
    assert ym.decode_luma(np.array([16, 235]), 8).tolist() == [0.0, 1.0] and ym.decode_luma(np.array([64, 940]), 10).tolist() == [0.0, 1.0]
    assert ym.decode_luma(np.array([0, 255]), 8, "full").tolist() == [0.0, 1.0] and ym.decode_luma(np.array([0, 1023]), 10, "full").tolist() == [0.0, 1.0]
    assert ym.decode_chroma(np.array([128, 240, 16]), 8).tolist() == [0.0, 0.5, -0.5] and ym.decode_chroma(np.array([512, 960]), 10).tolist() == [0.0, 0.5]
    assert ym.decode_chroma(np.array([128]), 8, "full").tolist() == [0.0] and ym.decode_chroma(np.array([512, 1023]), 10, "full")[1] == F(511.0) / F(1023.0)
    v = np.array([0.0, 1.0, -1.0, 2.0, np.nan, np.inf, -np.inf], F)
    assert ym.quantise(v, 8, False).tolist() == [16, 235, 0, 255, 0, 255, 0]
    assert ym.quantise(v, 10, False).tolist() == [64, 940, 4, 1019, 4, 1019, 4]
    assert ym.quantise(v, 10, False, rules=dict(ym.RULES, sdi_clamp=False)).tolist() == [64, 940, 0, 1023, 0, 1023, 0]
    assert ym.quantise(v, 8, False, "full").tolist() == [0, 255, 0, 255, 0, 255, 0]
    assert ym.quantise(v, 10, False, "full").tolist() == [0, 1023, 0, 1023, 0, 1023, 0]
    c = np.array([0.0, 0.5, -0.5], F)
    assert ym.quantise(c, 8, True).tolist() == [128, 240, 16] and ym.quantise(c, 10, True).tolist() == [512, 960, 64]
    # full range: 128s + max * C (0.5 lands on 255.5 and 1023.5, beyond the clamp; -0.25 on 64.25 and 256.25)
    c = np.array([0.0, 0.5, -0.25, -1.0], F)
    assert ym.quantise(c, 8, True, "full").tolist() == [128, 255, 64, 0] and ym.quantise(c, 10, True, "full").tolist() == [512, 1023, 256, 0]
    # half to even: 0.5 / 255 lies between codes 0 and 1
    assert ym.quantise(np.array([0.5 / 255, 1.5 / 255, 2.5 / 255], F), 8, False, "full").tolist() == [0, 2, 2]


def test_the_matrices_are_inverses_and_rec2020_is_the_stated_one():
    for name in ym.MATRICES:
        prod = np.array(ym.MATRICES[name]) @ np.array(ym.RGB_MATRICES[name])
        assert np.abs(prod - np.eye(3)).max() < 2e-5, (name, prod)
        assert abs(sum(ym.RGB_MATRICES[name][0]) - 1) < 1e-6 and abs(sum(ym.RGB_MATRICES[name][1])) < 1e-6 and abs(sum(ym.RGB_MATRICES[name][2])) < 1e-6
    kr, kb = 0.2627, 0.0593
    assert ym.RGB_MATRICES["2020"][0] == [kr, 0.6780, kb] and abs(ym.MATRICES["2020"][0][2] - 2 * (1 - kr)) < 1e-6 and abs(ym.MATRICES["2020"][2][1] - 2 * (1 - kb)) < 1e-6


# ---------------------------------------------------------------- anchors

def _solid(tables, rgbv, transfer):
    one = tables[2](np.array([1.0], F))[0]
    px = np.zeros((2, 4, 4), np.uint16)
    for i in range(3):
        px[..., i] = one if rgbv[i] else 0
    px[..., 3] = one
    return px


ANCHORS = {
    (8, "601", "studio"): {"white": (235, 128, 128), "black": (16, 128, 128), "red": (81, 90, 240), "green": (145, 54, 34), "blue": (41, 240, 110)},
    (8, "709", "studio"): {"white": (235, 128, 128), "black": (16, 128, 128), "red": (63, 102, 240), "green": (173, 42, 26), "blue": (32, 240, 118)},
    (10, "709", "studio"): {"white": (940, 512, 512), "black": (64, 512, 512), "red": (250, 409, 960), "green": (691, 167, 105), "blue": (127, 960, 471)},
    (8, "2020", "studio"): {"white": (235, 128, 128), "black": (16, 128, 128), "red": (74, 97, 240), "green": (164, 47, 25), "blue": (29, 240, 119)},
    (10, "2020", "studio"): {"white": (940, 512, 512), "black": (64, 512, 512), "red": (294, 387, 960), "green": (658, 189, 100), "blue": (116, 960, 476)},
    (8, "709", "full"): {"white": (255, 128, 128), "black": (0, 128, 128), "red": (54, 99, 255), "green": (182, 30, 12), "blue": (18, 255, 116)},
    (10, "2020", "full"): {"white": (1023, 512, 512), "black": (0, 512, 512), "red": (269, 369, 1023), "green": (694, 143, 42), "blue": (61, 1023, 471)},
}
COLOURS = {"white": (1, 1, 1), "black": (0, 0, 0), "red": (1, 0, 0), "green": (0, 1, 0), "blue": (0, 0, 1)}


@pytest.mark.parametrize("bits,matrix,range_", sorted(ANCHORS))
def test_export_anchors(tables, bits, matrix, range_):
    """Solid colours, from the matrices in exact arithmetic: Y = 16s + 219s*Ky (studio) or max*Ky (full), C likewise; every siting
    and both transfer settings give them (1.0 and 0.0 are fixed points of the table)."""
    full = (0, 0, 3, 1)
    m = np.array(ym.RGB_MATRICES[matrix])
    s, top = 1 << (bits - 8), (1 << bits) - 1
    for name, want in ANCHORS[(bits, matrix, range_)].items():
        ycc = m @ np.array(COLOURS[name], float)
        exact = (16 * s + 219 * s * ycc[0], 128 * s + 224 * s * ycc[1], 128 * s + 224 * s * ycc[2]) if range_ == "studio" else (
            top * ycc[0], 128 * s + top * ycc[1], 128 * s + top * ycc[2])
        assert want == tuple(int(np.clip(np.rint(v), 0, top)) for v in exact), (name, exact)
        for siting in ym.SITING_FLAGS:
            for transfer in ym.TRANSFER_FLAGS:
                y, cb, cr = ym.subsample_samples(_solid(tables, COLOURS[name], transfer), full, full, 4, 2, bits, tables[1], matrix, range_, siting, transfer)
                assert (y == want[0]).all() and (cb == want[1]).all() and (cr == want[2]).all(), (name, siting, transfer, y, cb, cr)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("range_", ["studio", "full"])
def test_import_anchors(tables, layout, range_):
    """Legal black and white come out as 0.0 and 1.0 (through the table, or as they are), alpha as 1.0, in every matrix and siting."""
    dec, _enc, f2h = tables
    bits = ym.BITS[layout]
    s, top = 1 << (bits - 8), (1 << bits) - 1
    one = f2h(np.array([1.0], F))[0]
    assert dec[0] == 0 and np.float16(dec[one:one + 1].view(np.float16)[0]) == np.float16(1.0)
    for luma, code in (((16 * s) if range_ == "studio" else 0, 0), ((235 * s) if range_ == "studio" else top, one)):
        planes = ym.pack(layout, np.full((2, 6), luma), np.full((1, 3), 128 * s), np.full((1, 3), 128 * s))
        for matrix in ym.MATRICES:
            for siting in ym.SITING_FLAGS:
                got = ym.reconstruct_model(layout, planes, 6, 2, dec, f2h, matrix, range_, siting, "709")
                assert (got[..., :3] == dec[code]).all() and (got[..., 3] == dec[one]).all()
                raw = ym.reconstruct_model(layout, planes, 6, 2, dec, f2h, matrix, range_, siting, "none")
                assert (raw[..., :3] == code).all() and (raw[..., 3] == one).all()


# ---------------------------------------------------------------- cross-checks that need no device

@pytest.mark.parametrize("matrix", ["601", "709"])
@pytest.mark.parametrize("width,height", [(2, 2), (6, 4), (26, 10), (130, 6)])
def test_planar8_left_studio_is_the_progressive_mpeg2_imports_model(tables, matrix, width, height):
    rng = np.random.default_rng(47 + width)
    planes = [rng.integers(0, 256, (height + 1, width + 3), dtype=np.uint8), rng.integers(0, 256, (height // 2 + 2, width // 2 + 5), dtype=np.uint8),
              rng.integers(0, 256, (height // 2, width // 2), dtype=np.uint8)]
    got = ym.reconstruct_model("planar8", planes, width, height, tables[0], tables[2], matrix)
    want = mpeg2_reconstruct_model(planes, width, height, tables[0], tables[2], interlaced=False, matrix=matrix)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("siting", list(ym.SITING_FLAGS))
def test_the_semi_planar_layouts_are_the_planar_ones_in_another_order(tables, siting):
    """NV12 de-interleaved is PLANAR8, P010 shifted down by 6 is PLANAR10: same pixels in, same codes out."""
    from tests.entry_cases import px16
    dec, enc, f2h = tables
    rng = np.random.default_rng(59)
    width, height = 14, 6
    for semi, planar in (("nv12", "planar8"), ("p010", "planar10")):
        y, cb, cr = _samples(rng, width, height, ym.BITS[semi])
        a = ym.reconstruct_model(semi, ym.pack(semi, y, cb, cr), width, height, dec, f2h, "2020", "full", siting)
        b = ym.reconstruct_model(planar, ym.pack(planar, y, cb, cr), width, height, dec, f2h, "2020", "full", siting)
        assert np.array_equal(a, b)
        full = (0, 0, width - 1, height - 1)
        frame = px16(rng, full).array
        sp = ym.subsample_model(semi, frame, full, full, width, height, enc, "601", "studio", siting)
        pp = ym.subsample_model(planar, frame, full, full, width, height, enc, "601", "studio", siting)
        for u, v in zip(ym.unpack(semi, sp, width, height), ym.unpack(planar, pp, width, height)):
            assert np.array_equal(u, v)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("matrix,range_,siting", [("601", "studio", "left"), ("709", "full", "center"), ("2020", "studio", "topleft"), ("2020", "full", "left")])
def test_model_against_a_float64_restatement_import(tables, layout, matrix, range_, siting):
    """The model's halves before the table against the contract restated in float64 with interpolation matrices.  Only the
    rounding differs: every truncated half lies within one half ulp of the float64 value."""
    rng = np.random.default_rng(41)
    width, height, bits = 22, 10, ym.BITS[layout]
    s, top = 1 << (bits - 8), (1 << bits) - 1
    y, cb, cr = _samples(rng, width, height, bits)
    got = ym.reconstruct_halves(layout, ym.pack(layout, y, cb, cr), width, height, tables[2], matrix, range_, siting)[..., :3].view(np.float16).astype(np.float64)
    yf = y / top if range_ == "full" else (y - 16.0 * s) / (219 * s)

    def taps(n, kind):
        """(2n, n) interpolation matrix: 'mid' (between samples 2c and 2c+1: 3/4, 1/4) or 'co' (on sample 2c: 1; halfway: 1/2, 1/2)"""
        m = np.zeros((2 * n, n))
        for i in range(2 * n):
            c = i // 2
            if kind == "mid":
                far = min(max(c - 1 if i % 2 == 0 else c + 1, 0), n - 1)
                m[i, c] += 0.75
                m[i, far] += 0.25
            elif i % 2 == 0:
                m[i, c] = 1.0
            else:
                m[i, c] += 0.5
                m[i, min(c + 1, n - 1)] += 0.5
        return m
    mv = taps(height // 2, "co" if siting == "topleft" else "mid")
    mh = taps(width // 2, "mid" if siting == "center" else "co")
    chroma = [mv @ ((c - 128.0 * s) / (top if range_ == "full" else 224 * s)) @ mh.T for c in (cb, cr)]
    m = np.array(ym.MATRICES[matrix])
    want = np.stack([m[i, 0] * yf + m[i, 1] * chroma[0] + m[i, 2] * chroma[1] for i in range(3)], axis=-1)
    ulp = np.maximum(np.abs(want), 2.0 ** -14) * 2.0 ** -10
    assert (np.abs(got - want) <= ulp * 1.001).all()


@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("matrix,range_,siting", [("601", "studio", "left"), ("709", "full", "center"), ("2020", "studio", "topleft")])
def test_model_against_a_float64_restatement_export(tables, bits, matrix, range_, siting):
    """The same for the export edge: no code differs by more than one, and fewer than one in a hundred differ at all."""
    rng = np.random.default_rng(43)
    width, height = 64, 16
    full = (0, 0, width - 1, height - 1)
    px = rng.integers(0, 0x3C01, (height, width, 4), dtype=np.uint16)
    got = ym.subsample_samples(px, full, full, width, height, bits, tables[1], matrix, range_, siting)
    rgbv = [tables[1][px[..., c]].view(np.float16).astype(np.float64) for c in range(3)]
    m = np.array(ym.RGB_MATRICES[matrix])
    yv, cbv, crv = (m[i, 0] * rgbv[0] + m[i, 1] * rgbv[1] + m[i, 2] * rgbv[2] for i in range(3))
    s, top = 1 << (bits - 8), (1 << bits) - 1
    c, k = np.arange(height // 2), np.arange(width // 2)

    def filt(e):
        v = 0.25 * e[np.maximum(2 * c - 1, 0)] + 0.5 * e[2 * c] + 0.25 * e[2 * c + 1] if siting == "topleft" else 0.5 * (e[2 * c] + e[2 * c + 1])
        if siting == "center":
            return 0.5 * (v[:, 2 * k] + v[:, 2 * k + 1])
        return 0.25 * v[:, np.maximum(2 * k - 1, 0)] + 0.5 * v[:, 2 * k] + 0.25 * v[:, 2 * k + 1]

    def quant(v, scale, offset):
        q = v + (offset * s / top if offset == 128 else 0) if range_ == "full" else v * scale * s / top + offset * s / top
        code = np.rint(np.clip(q, 0, 1) * top)
        return np.clip(code, 4, 1019) if bits == 10 and range_ == "studio" else code
    want = quant(yv, 219, 16), quant(filt(cbv), 224, 128), quant(filt(crv), 224, 128)
    for a, b in zip(got, want):
        d = np.abs(a - b)
        assert d.max() <= 1 and (d != 0).mean() < 0.01, (d.max(), (d != 0).mean())


# ---------------------------------------------------------------- the round trip: samples -> import -> export

def _round_trip(tables, layout, matrix, range_, siting, transfer, y, cb, cr):
    dec, enc, f2h = tables
    height, width = y.shape
    full = (0, 0, width - 1, height - 1)
    frame = ym.reconstruct_model(layout, ym.pack(layout, y, cb, cr), width, height, dec, f2h, matrix, range_, siting, transfer)
    return ym.subsample_samples(frame, full, full, width, height, ym.BITS[layout], enc, matrix, range_, siting, transfer)


def grey_round_trip_inputs(layout, range_):
    """Every legal luma code over neutral chroma, as a raster of two rows (DESIGN's first round-trip claim)."""
    bits = ym.BITS[layout]
    s, top = 1 << (bits - 8), (1 << bits) - 1
    codes = np.arange(16 * s, 235 * s + 1) if range_ == "studio" else np.arange(0, top + 1)
    width = 2 * ((len(codes) + 1) // 2)
    y = np.resize(codes, (2, width))
    return y, np.full((1, width // 2), 128 * s), np.full((1, width // 2), 128 * s)


def flat_round_trip_inputs(layout, range_):
    """400 colours, each flat over a 6 x 4 raster stacked below the last: Y' in [60s, 200s), Cb and Cr in [118s, 138s), in gamut in
    every matrix, so no clamp takes part (DESIGN's second claim).  Chroma is flat over the whole stack's columns only within a
    colour, so each colour is its own raster: returned as a list."""
    s = 1 << (ym.BITS[layout] - 8)
    rng = np.random.default_rng(53)
    return [(np.full((4, 6), rng.integers(60 * s, 200 * s)), np.full((2, 3), rng.integers(118 * s, 138 * s)), np.full((2, 3), rng.integers(118 * s, 138 * s)))
            for _ in range(400)]


def check_grey_round_trip(layout, range_, transfer, y, back):
    """8-bit: every code comes back.  10-bit through the transfer tables: luma within one code (the truncation to a half's 11-bit
    significand, stretched by the table's slope); 10-bit without them: every code comes back (the truncation alone moves a value
    by less than 2^-11 of itself, under half a code).  Chroma exactly."""
    y2, cb2, cr2 = back
    s = 1 << (ym.BITS[layout] - 8)
    assert (cb2 == 128 * s).all() and (cr2 == 128 * s).all()
    d = np.abs(y2 - y)
    if s == 1 or transfer == "none":
        assert d.max() == 0
    else:
        assert d.max() == 1 and 0.2 < (d != 0).mean() < 0.5, (d.max(), (d != 0).mean())


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("range_", ["studio", "full"])
@pytest.mark.parametrize("transfer", ["709", "none"])
def test_round_trip_of_every_legal_grey_code(tables, layout, range_, transfer):
    y, cb, cr = grey_round_trip_inputs(layout, range_)
    for matrix, siting in (("601", "left"), ("709", "center"), ("2020", "topleft")):
        check_grey_round_trip(layout, range_, transfer, y, _round_trip(tables, layout, matrix, range_, siting, transfer, y, cb, cr))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("matrix,range_,siting", [("601", "studio", "left"), ("709", "studio", "center"), ("2020", "studio", "topleft"), ("709", "full", "left")])
def test_round_trip_of_flat_in_gamut_colours(tables, layout, matrix, range_, siting):
    """Flat chroma survives every siting's interpolation and filter exactly, so the colour comes back as a grey does: 8-bit
    exactly, 10-bit luma within one code, chroma exactly."""
    s = 1 << (ym.BITS[layout] - 8)
    for y, cb, cr in flat_round_trip_inputs(layout, range_)[:100]:
        r, g, b = ym.rgb(layout, ym.pack(layout, y, cb, cr), 6, 4, matrix, range_, siting)
        assert min(r.min(), g.min(), b.min()) >= 0 and max(r.max(), g.max(), b.max()) <= 1
        y2, cb2, cr2 = _round_trip(tables, layout, matrix, range_, siting, "709", y, cb, cr)
        assert np.array_equal(cb2, cb) and np.array_equal(cr2, cr)
        assert np.abs(y2 - y).max() <= (0 if s == 1 else 1)
        if s == 4:
            y3, cb3, cr3 = _round_trip(tables, layout, matrix, range_, siting, "none", y, cb, cr)
            assert np.array_equal(y3, y) and np.array_equal(cb3, cb) and np.array_equal(cr3, cr)


def test_varying_chroma_does_not_round_trip(tables):
    """What DESIGN does not claim: interpolating and filtering again is a low-pass, so chroma that varies from sample to sample
    comes back changed, in every siting."""
    rng = np.random.default_rng(61)
    y = np.full((8, 16), 120)
    cb, cr = rng.integers(100, 156, (4, 8)), rng.integers(100, 156, (4, 8))
    for siting in ym.SITING_FLAGS:
        _y2, cb2, cr2 = _round_trip(tables, "nv12", "709", "studio", siting, "709", y, cb, cr)
        assert not np.array_equal(cb2, cb) and not np.array_equal(cr2, cr)


# ---------------------------------------------------------------- the catalogue

def test_the_device_entries_of_the_header_have_their_catalogue_cases():
    """Every case calls ONE of the header's two entries, once, handing it the factory's stream; asks for the same operands every
    time; the planes are buffers of class "plane" (8-bit) or "bytes" (10-bit) and the frame a frame; one output frame, or every
    plane an output.  Both entries are called by every layout's group."""
    from tests.test_entry_cases_cpu import HostOnly, Recorder
    names, stream = [], 0x5EED
    for (gid, build), layout in zip(yc.GROUPS, LAYOUTS):
        rec, called = Recorder(), set()
        for (what, case), spec in zip(build(rec), yc.specs(layout)):
            assert what == yc.name(spec)
            before = len(rec.calls)
            fac = HostOnly(rec, stream)
            assert case(fac) == 0
            made = rec.calls[before:]
            assert len(made) == 1 and made[0] == ("cvs_%s_420_dev" % spec["direction"], stream), (gid, what, made)
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
    run = 63 * yc.LANE_PIXELS
    assert set(yc.widths()) >= {2, 4, 6, 8, 10, 14, run - 2, run, run + 2, 2 * run - 2, 2 * run, 2 * run + 2}
    assert set(yc.widths()) >= {run - 4, run - 2, run, 2 * (run - 2) - 2, 2 * (run - 2), 2 * (run - 2) + 2}        # the 62-lane run of centre siting
    for layout in LAYOUTS:
        specs = yc.specs(layout)
        for direction in ("reconstruct", "subsample"):
            mine = [s for s in specs if s["direction"] == direction]
            assert set(yc.widths()) == {s["width"] for s in mine}
            assert {2, 4, 6, 10, yc.STRIP_ROWS - 2, yc.STRIP_ROWS, yc.STRIP_ROWS + 2} == {s["height"] for s in mine}
            # every value of every flag meets this layout in this direction
            assert {s["siting"] for s in mine} == set(ym.SITING_FLAGS) and {s["range"] for s in mine} == set(ym.RANGE_FLAGS)
            assert {s["matrix"] for s in mine} == set(ym.MATRIX_FLAGS) and {s["transfer"] for s in mine} == set(ym.TRANSFER_FLAGS)
            # every siting on both sides of its run (the import's is 62 lanes at centre siting), one wave's and two waves'
            for siting in ym.SITING_FLAGS:
                assert {s["width"] for s in mine if s["siting"] == siting} >= set(yc.widths()[6:])
            least = [ym.least(layout, s["width"], s["height"]) for s in mine]
            assert any(s["strides"] == l[0] and s["lines"] == l[1] for s, l in zip(mine, least))
            assert any(s["strides"][0] > l[0][0] for s, l in zip(mine, least)) and any(s["lines"][0] > l[1][0] for s, l in zip(mine, least))
            assert any(s["strides"][1] > l[0][1] for s, l in zip(mine, least)) and any(s["lines"][1] > l[1][1] for s, l in zip(mine, least))
            boxes = [(s["full"], s["width"], s["height"]) for s in mine]
            assert any(f == (0, 0, w - 1, h - 1) for f, w, h in boxes)                                    # the raster's own
            assert any(f[0] < 0 and f[1] < 0 and f[2] >= w and f[3] >= h for f, w, h in boxes)              # larger
            assert any(f[0] > 0 and f[2] < w - 1 for f, w, h in boxes)                                     # inside
            assert any(f[0] < 0 and f[2] < w - 1 for f, w, h in boxes)                                     # partly off, negative origin
        tall = yc.tall_specs(layout)
        assert {(s["direction"], s["siting"]) for s in tall} == {(d, s) for d in ("reconstruct", "subsample") for s in ym.SITING_FLAGS}
        assert all(s["height"] // 2 > 2 * 256 * 6 * 4 and s["width"] * s["height"] <= 1 << 20 for s in tall)


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
    both = {(l, d) for l in LAYOUTS for d in ("reconstruct", "subsample")}
    if rule in ("matrix", "range", "siting_v", "siting_h", "transfer", "top_clamp", "left_clamp"):
        assert set(moved) == both, (rule, sorted(both - set(moved)))          # every layout's own cases exercise it, in both directions
    if rule in ("bottom_clamp", "right_clamp"):
        assert set(moved) == {(l, "reconstruct") for l in LAYOUTS}, moved
    if rule == "black_outside":
        assert set(moved) == {(l, "subsample") for l in LAYOUTS}, moved
    if rule == "mask":
        assert set(moved) == {("planar10", "reconstruct"), ("p010", "reconstruct")}, moved
    if rule == "sdi_clamp":
        assert set(moved) == {("planar10", "subsample"), ("p010", "subsample")}, moved


# ---------------------------------------------------------------- the nodes, as far as they go without a device

@pytest.fixture(scope="module")
def process():
    from fluggo.media import process
    return process


def _coded_source(process):
    class Planes(process.CodedImageSource):
        def get_frame(self, frame):
            return [process.CodedImage(bytearray(64 * 4), 64, 4), process.CodedImage(bytearray(64 * 2), 64, 2)]
    return Planes()


def test_node_surface(process):
    from fluggo.media.basetypes import v2i
    src, solid = _coded_source(process), process.SolidColorVideoSource((0.2, 0.3, 0.4, 1.0))
    R, S = process.YCbCr420ReconstructionFilter, process.YCbCr420SubsampleFilter
    assert issubclass(R, process.VideoSource) and issubclass(S, process.CodedImageSource)
    assert type(R(src, (16, 4))._video_frame_source_funcs).__name__ == "PyCapsule"
    assert type(S(solid, (16, 4))._coded_image_source_funcs).__name__ == "PyCapsule"
    for layout in LAYOUTS:
        for matrix in ym.MATRIX_FLAGS:
            for range_ in ym.RANGE_FLAGS:
                for siting in ym.SITING_FLAGS:
                    R(src, v2i(1920, 1080), layout, matrix, range_, siting, "none")
                    S(source=solid, size=(1920, 2), layout=layout, matrix=matrix, range=range_, siting=siting, transfer="709")
    R(src, size=(2, 2))
    S(solid, size=(7680, 4320), layout="p010", transfer="none")


def test_nodes_refuse_bad_sources_sizes_and_keywords_naming_the_choices(process):
    src, solid = _coded_source(process), process.SolidColorVideoSource((0.2, 0.3, 0.4, 1.0))
    choices = {"layout": ("planar8", "planar10", "nv12", "p010"), "matrix": ("601", "709", "2020"), "range": ("studio", "full"),
               "siting": ("left", "center", "topleft"), "transfer": ("709", "none")}
    bad_values = {"layout": ["yuv420p", "NV12", "", 2, None, b"nv12", "uyvy", "v210"], "matrix": ["bt2020", "", "rec709", 601, 2020, None, b"601"],
                  "range": ["limited", "tv", "", 0, None, "Full"], "siting": ["centre", "top-left", "", 1, None, "mpeg2"],
                  "transfer": ["pq", "hlg", "", 709, None, "linear"]}
    for node, good, bad in ((process.YCbCr420ReconstructionFilter, src, solid), (process.YCbCr420SubsampleFilter, solid, src)):
        with pytest.raises(Exception):
            node(bad, (16, 4))
        with pytest.raises(Exception):
            node(object(), (16, 4))
        with pytest.raises(TypeError):
            node(good)                                                            # no default raster
        for size in [(721, 486), (0, 4), (16, 0), (-2, 4), (1, 1), (16, -2), (16, 5), (16, 1)]:
            with pytest.raises(ValueError, match="even and at least 2"):
                node(good, size)
        for key, values in bad_values.items():
            for value in values:
                with pytest.raises(ValueError) as info:
                    node(good, (16, 4), **{key: value})
                assert key in str(info.value) and all('"%s"' % c in str(info.value) for c in choices[key]), str(info.value)


def test_a_pull_gives_the_raster_or_without_a_gpu_is_empty_or_loud(process):
    from canvas_amd import _lib
    from fluggo.media.basetypes import box2i
    node = process.YCbCr420ReconstructionFilter(_coded_source(process), size=(16, 4), layout="nv12")
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
