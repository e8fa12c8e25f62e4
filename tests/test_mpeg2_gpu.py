"""MPEG-2 4:2:0 subsample on the GPU, byte for byte against the numpy model of the contract (tests/mpeg2_model.py,
DESIGN.md "MPEG-2 4:2:0 subsample"): the device entry at three rasters, odd windows, padded planes, the host entry,
both arithmetic flavours, and the encode scripts' node chains."""
import ctypes as C

import numpy as np
import pytest

from canvas_amd import _lib
from canvas_amd.abi import HostFrame
from tests.mpeg2_model import mpeg2_subsample_model

pytestmark = pytest.mark.gpu

PAD = 0xA5


@pytest.fixture(scope="module")
def table(orc):
    return orc.transfer_table(2)


def _frame_codes(rng, height, width):
    """Half RGBA codes, mostly in [0, 1), with whole rows of negative, > 1, +-Inf, NaN and arbitrary codes."""
    codes = rng.uniform(0.0, 1.0, (height, width, 4)).astype(np.float16).view(np.uint16)
    special = [rng.uniform(-2.0, 0.0, (width, 4)).astype(np.float16).view(np.uint16),
               rng.uniform(1.0, 300.0, (width, 4)).astype(np.float16).view(np.uint16),
               np.tile(np.array([0x7C00, 0xFC00, 0x7C00, 0x3C00], np.uint16), (width, 1)),
               np.tile(np.array([0x7E00, 0x3800, 0xFE01, 0x3C00], np.uint16), (width, 1)),
               rng.integers(0, 65536, (width, 4), dtype=np.uint16),
               np.tile(np.array([0x789B, 0x789B, 0x789C, 0x3C00], np.uint16), (width, 1))]   # the code where the two flavours' tables differ
    for i, row in enumerate(range(1, height, max(1, height // 12))):
        codes[row] = special[i % len(special)]
    if width > 8:
        codes[:, 3, 0] = 0x7E00                                # a NaN column too
    return codes


def _subsample_dev(cvs, codes, full, cur, width, height, pads=(0, 0, 0), extra_lines=(0, 0, 0)):
    """cvs_subsample_mpeg2_dev on a device frame and padded device planes pre-filled with PAD; returns the whole planes
    (line_count x stride) as numpy arrays."""
    strides = [width + pads[0], width // 2 + pads[1], width // 2 + pads[2]]
    lines = [height + extra_lines[0], height // 2 + extra_lines[1], height // 2 + extra_lines[2]]
    frame = HostFrame(full, np.uint16, codes, cur)
    from canvas_amd.device import DeviceFrame
    dframe = DeviceFrame.from_host(frame)
    ptrs = [cvs.cvs_malloc(s * n) for s, n in zip(strides, lines)]
    try:
        img = _lib.coded_image()
        for p in range(3):
            assert ptrs[p]
            _lib.check(cvs.cvs_memset(ptrs[p], PAD, strides[p] * lines[p], None), "memset")
            img.data[p], img.stride[p], img.line_count[p] = ptrs[p], strides[p], lines[p]
        _lib.check(cvs.cvs_subsample_mpeg2_dev(C.byref(img), dframe.ref(), width, height, None), "cvs_subsample_mpeg2_dev")
        out = []
        for p in range(3):
            a = np.empty((lines[p], strides[p]), np.uint8)
            _lib.check(cvs.cvs_memcpy_d2h(a.ctypes.data, ptrs[p], a.nbytes, None), "d2h")
            out.append(a)
        assert np.array_equal(dframe.download().array, frame.array), "the device frame was modified"
        return out
    finally:
        for p in ptrs:
            if p:
                cvs.cvs_free(p)
        dframe.free()


def _assert_planes(got, want, width, height, what):
    sizes = [(height, width), (height // 2, width // 2), (height // 2, width // 2)]
    for p, (h, w) in enumerate(sizes):
        g = got[p][:h, :w]
        if not np.array_equal(g, want[p]):
            bad = np.argwhere(g != want[p])
            y, x = bad[0]
            raise AssertionError("%s plane %d: %d of %d bytes differ; first at (%d, %d): got %d want %d" % (
                what, p, len(bad), g.size, x, y, g[y, x], want[p][y, x]))
        assert (got[p][:, w:] == PAD).all() and (got[p][h:] == PAD).all(), "%s plane %d: padding written" % (what, p)


@pytest.mark.parametrize("width,height", [(720, 480), (1920, 1080), (3840, 2160)])
def test_device_entry_whole_raster(cvs, table, width, height):
    rng = np.random.default_rng(width)
    codes = _frame_codes(rng, height, width)
    full = (0, 0, width - 1, height - 1)
    got = _subsample_dev(cvs, codes, full, full, width, height)
    _assert_planes(got, mpeg2_subsample_model(codes, full, full, width, height, table), width, height, "%dx%d" % (width, height))


@pytest.mark.parametrize("full,cur", [((0, 0, 719, 479), (37, 21, 601, 302)),         # not aligned to 2 or 4
                                      ((-5, -3, 800, 500), (-5, -3, 800, 500)),       # a buffer larger than the raster
                                      ((-5, -3, 800, 500), (1, 2, 799, 498)),
                                      ((0, 0, 719, 479), (101, 77, 101, 77)),         # a single pixel
                                      ((0, 0, 719, 479), (0, 0, 0, 479)),             # column 0 alone: the clamp at -1
                                      ((0, 0, 719, 479), (0, 0, -1, -1)),             # empty: black planes
                                      ((200, 100, 300, 200), (200, 100, 300, 200)),   # a buffer inside the raster
                                      ((700, 470, 760, 520), (700, 470, 760, 520))])  # the bottom-right corner
def test_device_entry_windows(cvs, table, full, cur):
    rng = np.random.default_rng(sum(full) + 7 * sum(cur))
    codes = _frame_codes(rng, full[3] - full[1] + 1, full[2] - full[0] + 1)
    got = _subsample_dev(cvs, codes, full, cur, 720, 480)
    _assert_planes(got, mpeg2_subsample_model(codes, full, cur, 720, 480, table), 720, 480, "%r %r" % (full, cur))
    if cur[2] < cur[0]:
        assert [int(np.unique(got[p][:(480, 240, 240)[p], :(720, 360, 360)[p]])[0]) for p in range(3)] == [16, 128, 128]


@pytest.mark.parametrize("width,height", [(720, 480), (2, 4), (130, 8), (128, 12), (1920, 1080)])
def test_device_entry_padded_planes(cvs, table, width, height):
    rng = np.random.default_rng(height)
    codes = _frame_codes(rng, height, width)
    full = (0, 0, width - 1, height - 1)
    got = _subsample_dev(cvs, codes, full, full, width, height, pads=(13, 5, 64), extra_lines=(2, 1, 3))
    _assert_planes(got, mpeg2_subsample_model(codes, full, full, width, height, table), width, height, "padded %dx%d" % (width, height))


def test_device_entry_refuses(cvs):
    img = _lib.coded_image()
    frame = HostFrame((0, 0, 7, 7), np.uint16)
    for w, h in [(721, 480), (720, 482), (0, 480), (720, 0), (1, 4), (2, 2)]:
        assert cvs.cvs_subsample_mpeg2_dev(C.byref(img), frame.ref(), w, h, None) == -1
        assert _lib.last_error()
    ptrs = [cvs.cvs_malloc(720 * 480) for _ in range(3)]
    try:
        for p in range(3):
            img.data[p], img.stride[p], img.line_count[p] = ptrs[p], 360, 240
        img.stride[0], img.line_count[0] = 719, 480              # luma stride too short
        assert cvs.cvs_subsample_mpeg2_dev(C.byref(img), frame.ref(), 720, 480, None) == -1
        img.stride[0], img.line_count[2] = 720, 239               # chroma plane too short
        assert cvs.cvs_subsample_mpeg2_dev(C.byref(img), frame.ref(), 720, 480, None) == -1
        img.line_count[2] = 240
        bad = HostFrame((0, 0, 7, 7), np.uint16, current_window=(0, 0, 8, 7))    # window outside the buffer
        assert cvs.cvs_subsample_mpeg2_dev(C.byref(img), bad.ref(), 720, 480, None) == -1
    finally:
        for p in ptrs:
            cvs.cvs_free(p)


def test_host_entry_matches_device_entry_and_leaves_the_frame(cvs, table):
    rng = np.random.default_rng(11)
    full, cur = (-3, -2, 730, 485), (5, 3, 700, 470)
    codes = _frame_codes(rng, full[3] - full[1] + 1, full[2] - full[0] + 1)
    frame = HostFrame(full, np.uint16, codes.copy(), cur)
    img = cvs.video_subsample_mpeg2(frame.ref())
    assert img, _lib.last_error()
    try:
        got = []
        for p, (h, w) in enumerate([(480, 720), (240, 360), (240, 360)]):
            assert (img.contents.stride[p], img.contents.line_count[p]) == (w, h)
            got.append(np.ctypeslib.as_array(C.cast(img.contents.data[p], C.POINTER(C.c_uint8)), shape=(h, w)).copy())
    finally:
        C.CFUNCTYPE(None, C.c_void_p)(img.contents.free_func)(C.cast(img, C.c_void_p))
    assert np.array_equal(frame.array, codes), "the caller's frame was modified"
    assert (frame.current_window.min.x, frame.current_window.max.y) == (5, 470)
    want = mpeg2_subsample_model(codes, full, cur, 720, 480, table)
    for p in range(3):
        assert np.array_equal(got[p], want[p]), "host entry plane %d" % p
    dev = _subsample_dev(cvs, codes, full, cur, 720, 480)
    for p in range(3):
        assert np.array_equal(dev[p], got[p]), "device vs host entry plane %d" % p
    empty = HostFrame((0, 0, 3, 3), np.uint16, current_window=(0, 0, -1, -1))
    img = cvs.video_subsample_mpeg2(empty.ref())
    assert img, _lib.last_error()
    try:
        y = np.ctypeslib.as_array(C.cast(img.contents.data[0], C.POINTER(C.c_uint8)), shape=(480, 720))
        assert (y == 16).all()
    finally:
        C.CFUNCTYPE(None, C.c_void_p)(img.contents.free_func)(C.cast(img, C.c_void_p))


def test_same_bytes_in_both_arithmetic_flavours(cvs, table):
    rng = np.random.default_rng(5)
    width, height = 1920, 1080
    codes = _frame_codes(rng, height, width)
    full = (0, 0, width - 1, height - 1)
    want = mpeg2_subsample_model(codes, full, full, width, height, table)
    before = cvs.cvs_set_arithmetic(_lib.ARITH_CONTRACTED)
    try:
        got_fma = _subsample_dev(cvs, codes, full, full, width, height)
        cvs.cvs_set_arithmetic(_lib.ARITH_SEPARATE)
        got_sep = _subsample_dev(cvs, codes, full, full, width, height)
    finally:
        cvs.cvs_set_arithmetic(before if before >= 0 else _lib.ARITH_SEPARATE)
    _assert_planes(got_fma, want, width, height, "contracted")
    _assert_planes(got_sep, want, width, height, "separate")


def test_flavour_independent_where_the_flavours_tables_differ(cvs, orc, table):
    """Linear -> Rec.709 built with a fused a * pow - b (the contracted flavour's table) differs from the separate one at code
    0x789b; the filter always reads the separate table, so pixels made of that code encode the same in both flavours."""
    with orc.flavour("fma"):
        fused = orc.transfer_table(2)
    assert (fused != table).any()
    width, height = 64, 8
    codes = np.zeros((height, width, 4), np.uint16)
    codes[...] = np.array([0x789B, 0x789B, 0x789C, 0x3C00], np.uint16)
    codes[:, 40:] = np.array([0x789C, 0x789B, 0x789B, 0x3C00], np.uint16)
    full = (0, 0, width - 1, height - 1)
    want = mpeg2_subsample_model(codes, full, full, width, height, table)
    assert any((a != b).any() for a, b in zip(want, mpeg2_subsample_model(codes, full, full, width, height, fused))), \
        "the frame does not tell the two tables apart"
    before = cvs.cvs_set_arithmetic(_lib.ARITH_CONTRACTED)
    try:
        got_fma = _subsample_dev(cvs, codes, full, full, width, height)
        cvs.cvs_set_arithmetic(_lib.ARITH_SEPARATE)
        got_sep = _subsample_dev(cvs, codes, full, full, width, height)
    finally:
        cvs.cvs_set_arithmetic(before if before >= 0 else _lib.ARITH_SEPARATE)
    _assert_planes(got_fma, want, width, height, "contracted")
    _assert_planes(got_sep, want, width, height, "separate")


# ---------------------------------------------------------------- the node, as the encode scripts build it

@pytest.fixture(scope="module")
def process():
    from fluggo.media import process
    return process


def _planes_of(coded):
    return [np.frombuffer(bytes(p.data), np.uint8).reshape(p.line_count, p.stride) for p in coded]


@pytest.mark.parametrize("size", [None, (1920, 1080), (64, 36)])
def test_node_solid_colour_with_a_window(process, orc, table, size):
    from fluggo.media import basetypes as bt
    colour = (0.2, 0.45, 0.7, 1.0)
    solid = process.SolidColorVideoSource(colour, bt.box2i(40, 30, 650, 400))
    node = process.MPEG2SubsampleFilter(solid) if size is None else process.MPEG2SubsampleFilter(solid, size=size)
    width, height = size or (720, 480)
    coded = node.get_frame(0)
    assert [(p.stride, p.line_count) for p in coded] == [(width, height), (width // 2, height // 2), (width // 2, height // 2)]
    full = (0, 0, width - 1, height - 1)
    codes = np.zeros((height, width, 4), np.uint16)
    codes[...] = orc.float_to_half(np.array(colour, np.float32))
    cur = (40, 30, min(650, width - 1), min(400, height - 1))
    want = mpeg2_subsample_model(codes, full, cur, width, height, table)
    for p, plane in enumerate(_planes_of(coded)):
        assert np.array_equal(plane, want[p]), "plane %d" % p


def test_node_after_dv_reconstruction(process, orc, table):
    """The chain of the reference's encode scripts: coded DV planes -> DVReconstructionFilter -> MPEG2SubsampleFilter."""
    from canvas_amd.abi import HostFrame as HF
    rng = np.random.default_rng(3)
    dv = [np.ascontiguousarray(rng.integers(0, 256, (480, s), dtype=np.uint8)) for s in (720, 180, 180)]

    class Tape(process.CodedImageSource):
        def get_frame(self, frame):
            return [process.CodedImage(bytearray(p.tobytes()), p.shape[1], 480) for p in dv]

    recon = process.DVReconstructionFilter(Tape())
    coded = process.MPEG2SubsampleFilter(recon, size=(720, 480)).get_frame(0)
    assert coded is not None, _lib.last_error()
    # the frame the node pulls: (0,0)-(719,479) from the reconstruction, as the oracle renders it
    theirs = HF((0, 0, 719, 479), np.uint16)
    orc.lib().orc_reconstruct_dv(theirs.ref(), (C.c_void_p * 3)(*[p.ctypes.data for p in dv]), (C.c_int * 3)(720, 180, 180))
    cw = theirs.current_window
    want = mpeg2_subsample_model(theirs.array, (0, 0, 719, 479), (cw.min.x, cw.min.y, cw.max.x, cw.max.y), 720, 480, table)
    for p, plane in enumerate(_planes_of(coded)):
        assert np.array_equal(plane, want[p]), "plane %d" % p
