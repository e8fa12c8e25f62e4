"""MPEG-2 4:2:0 reconstruction on the GPU, bit for bit against the numpy model of the contract (tests/mpeg2_reconstruct_model.py,
DESIGN.md "MPEG-2 4:2:0 reconstruction"): the device entry at three rasters in both sitings and both matrices, windows, padded
planes, small rasters, refusals, the host entry, both arithmetic flavours, the node (alone, in a workspace pulled by a queue) and
the chain back through MPEG2SubsampleFilter."""
import ctypes as C
import threading

import numpy as np
import pytest

from canvas_amd import _lib
from canvas_amd.abi import HostFrame
from canvas_amd.device import DeviceFrame
from tests.mpeg2_model import mpeg2_subsample_model
from tests.mpeg2_reconstruct_model import expected_frame, reconstruct_model

pytestmark = pytest.mark.gpu

SENTINEL = np.array([0x7E17, 0x1234, 0xFBCD, 0x0001], np.uint16)     # codes the filter never stores (a NaN among them)
MODES = [(True, "601"), (True, "709"), (False, "601"), (False, "709")]


@pytest.fixture(scope="module")
def table(orc):
    return orc.transfer_table(0)


def _flags(interlaced, matrix):
    return (0 if interlaced else _lib.YCC_PROGRESSIVE) | (_lib.YCC_REC709 if matrix == "709" else 0)


def _random_planes(rng, width, height, pads=(0, 0, 0), extra_lines=(0, 0, 0)):
    """Y', Cb, Cr as (line_count, stride) uint8 arrays: random bytes over 0..255 and a 0..255 ramp row in each plane."""
    shapes = [(height + extra_lines[0], width + pads[0]), (height // 2 + extra_lines[1], width // 2 + pads[1]),
              (height // 2 + extra_lines[2], width // 2 + pads[2])]
    planes = [rng.integers(0, 256, s, dtype=np.uint8) for s in shapes]
    for p in planes:
        p[min(1, p.shape[0] - 1)] = np.arange(p.shape[1]) % 256
    return planes


def _upload_planes(cvs, planes):
    ptrs = []
    img = _lib.coded_image()
    for p, a in enumerate(planes):
        a = np.ascontiguousarray(a)
        ptr = cvs.cvs_malloc(a.nbytes)
        assert ptr
        ptrs.append(ptr)
        _lib.check(cvs.cvs_memcpy_h2d(ptr, a.ctypes.data, a.nbytes, None), "h2d")
        img.data[p], img.stride[p], img.line_count[p] = ptr, a.shape[1], a.shape[0]
    return img, ptrs


def _reconstruct_dev(cvs, planes, width, height, flags, full):
    """cvs_reconstruct_mpeg2_dev into a device frame over `full` pre-filled with SENTINEL: (rc, frame codes, window or None)."""
    before = np.broadcast_to(SENTINEL, (full[3] - full[1] + 1, full[2] - full[0] + 1, 4)).copy()
    dframe = DeviceFrame.from_host(HostFrame(full, np.uint16, before))
    img, ptrs = _upload_planes(cvs, planes)
    try:
        rc = cvs.cvs_reconstruct_mpeg2_dev(dframe.ref(), C.byref(img), width, height, flags, None)
        _lib.check(cvs.cvs_stream_sync(None), "sync")
        got = dframe.download()
        w = got.current_window
        return rc, got.array, (None if w.is_empty() else (w.min.x, w.min.y, w.max.x, w.max.y))
    finally:
        for p in ptrs:
            cvs.cvs_free(p)
        dframe.free()


def _assert_frame(cvs_out, planes, width, height, interlaced, matrix, full, table, orc, what):
    rc, got, window = cvs_out
    assert rc == 0, "%s: %s" % (what, _lib.last_error())
    raster = reconstruct_model(planes, width, height, table, orc.float_to_half, interlaced, matrix)
    before = np.broadcast_to(SENTINEL, got.shape).copy()
    want, want_window = expected_frame(before, full, raster, width, height)
    assert window == want_window, "%s: window %r, want %r" % (what, window, want_window)
    if not np.array_equal(got, want):
        bad = np.argwhere((got != want).any(axis=-1))
        y, x = bad[0]
        raise AssertionError("%s: %d of %d pixels differ; first at frame (%d, %d): got %s want %s" % (
            what, len(bad), got.shape[0] * got.shape[1], x + full[0], y + full[1], got[y, x], want[y, x]))


@pytest.mark.parametrize("interlaced,matrix", MODES)
@pytest.mark.parametrize("width,height", [(720, 480), (1920, 1080), (3840, 2160)])
def test_device_entry_whole_raster(cvs, orc, table, width, height, interlaced, matrix):
    rng = np.random.default_rng(width + height + 2 * interlaced + (matrix == "709"))
    planes = _random_planes(rng, width, height)
    full = (0, 0, width - 1, height - 1)
    _assert_frame(_reconstruct_dev(cvs, planes, width, height, _flags(interlaced, matrix), full), planes, width, height, interlaced, matrix,
                  full, table, orc, "%dx%d %s %s" % (width, height, "interlaced" if interlaced else "progressive", matrix))


@pytest.mark.parametrize("interlaced", [True, False])
@pytest.mark.parametrize("full", [(-5, -3, 800, 500),         # a buffer larger than the raster, negative origin
                                  (200, 100, 300, 200),       # a buffer inside the raster
                                  (37, 21, 601, 302),         # odd corners
                                  (101, 77, 101, 77),         # a single pixel (odd column)
                                  (100, 76, 100, 76),         # a single pixel (even column)
                                  (719, 479, 719, 479),       # the bottom-right pixel
                                  (700, 470, 760, 520),       # the bottom-right corner and beyond
                                  (-9, -9, -1, 40),           # left of the raster: empty
                                  (720, 0, 800, 10)])         # right of it: empty
def test_device_entry_windows(cvs, orc, table, full, interlaced):
    rng = np.random.default_rng(sum(full) + interlaced)
    planes = _random_planes(rng, 720, 480)
    _assert_frame(_reconstruct_dev(cvs, planes, 720, 480, _flags(interlaced, "601"), full), planes, 720, 480, interlaced, "601", full,
                  table, orc, "window %r" % (full,))


@pytest.mark.parametrize("width,height,interlaced", [(720, 480, True), (720, 480, False), (2, 4, True), (130, 8, True), (130, 8, False),
                                                    (2, 2, False), (6, 6, False), (128, 12, True), (1920, 1080, False)])
def test_device_entry_padded_planes_and_small_rasters(cvs, orc, table, width, height, interlaced):
    rng = np.random.default_rng(width * height)
    for pads, extra in [((0, 0, 0), (0, 0, 0)), ((13, 5, 64), (2, 1, 3)), ((1, 1, 0), (0, 0, 1))]:
        planes = _random_planes(rng, width, height, pads, extra)
        full = (0, 0, width - 1, height - 1)
        for matrix in ("601", "709"):
            _assert_frame(_reconstruct_dev(cvs, planes, width, height, _flags(interlaced, matrix), full), planes, width, height, interlaced,
                          matrix, full, table, orc, "%dx%d pads %r lines %r" % (width, height, pads, extra))


def test_device_entry_refuses(cvs):
    planes = [np.zeros((480, 720), np.uint8), np.zeros((240, 360), np.uint8), np.zeros((240, 360), np.uint8)]
    img, ptrs = _upload_planes(cvs, planes)
    frame = DeviceFrame((0, 0, 7, 7), np.uint16)
    try:
        def refused(w, h, flags=0):
            frame.c.current_window.min.x, frame.c.current_window.max.x = 0, 7
            rc = cvs.cvs_reconstruct_mpeg2_dev(frame.ref(), C.byref(img), w, h, flags, None)
            return rc == -1 and bool(_lib.last_error()) and frame.current_window.is_empty()

        for w, h in [(721, 480), (720, 482), (720, 478), (0, 480), (720, 0), (1, 4), (2, 2), (-2, 4)]:
            assert refused(w, h), (w, h)
        for w, h in [(721, 480), (720, 481), (0, 2), (2, 0), (1, 2)]:
            assert refused(w, h, _lib.YCC_PROGRESSIVE), (w, h)
        assert refused(720, 480, 4)                                 # an unknown flag bit
        img.stride[0] = 719                                         # luma stride too short
        assert refused(720, 480)
        img.stride[0], img.line_count[0] = 720, 479                 # luma too few lines
        assert refused(720, 480)
        img.line_count[0], img.stride[2] = 480, 359                 # chroma stride too short
        assert refused(720, 480)
        img.stride[2], img.line_count[1] = 360, 239                 # chroma too few lines
        assert refused(720, 480, _lib.YCC_PROGRESSIVE)
        img.line_count[1] = 240
        missing = _lib.coded_image()
        missing.data[0], missing.stride[0], missing.line_count[0] = img.data[0], 720, 480
        frame.c.current_window.min.x, frame.c.current_window.max.x = 0, 7
        assert cvs.cvs_reconstruct_mpeg2_dev(frame.ref(), C.byref(missing), 720, 480, 0, None) == -1
        assert frame.current_window.is_empty()
        assert cvs.cvs_reconstruct_mpeg2_dev(frame.ref(), C.byref(img), 720, 480, 0, None) == 0       # the same planes, right sizes
        assert not frame.current_window.is_empty()
    finally:
        for p in ptrs:
            cvs.cvs_free(p)
        frame.free()


def test_host_entry_matches_device_entry(cvs, orc, table):
    rng = np.random.default_rng(17)
    planes = _random_planes(rng, 720, 480, pads=(8, 0, 4))
    for full in [(-3, -2, 730, 485), (5, 3, 700, 470), (0, 0, 719, 479)]:
        before = np.broadcast_to(SENTINEL, (full[3] - full[1] + 1, full[2] - full[0] + 1, 4)).copy()
        frame = HostFrame(full, np.uint16, before.copy(), (0, 0, -1, -1))
        img = _lib.coded_image()
        keep = [np.ascontiguousarray(p) for p in planes]
        for p, a in enumerate(keep):
            img.data[p], img.stride[p], img.line_count[p] = a.ctypes.data, a.shape[1], a.shape[0]
        cvs.video_reconstruct_mpeg2(frame.ref(), C.byref(img))
        w = frame.current_window
        assert not w.is_empty(), _lib.last_error()
        dev = _reconstruct_dev(cvs, planes, 720, 480, 0, full)
        assert dev[0] == 0 and dev[2] == (w.min.x, w.min.y, w.max.x, w.max.y)
        assert np.array_equal(frame.array, dev[1]), "host entry vs device entry, %r" % (full,)
        _assert_frame(dev, planes, 720, 480, True, "601", full, table, orc, "host entry %r" % (full,))
    short = _lib.coded_image()
    small = [np.zeros((480, 720), np.uint8), np.zeros((240, 360), np.uint8), np.zeros((239, 360), np.uint8)]
    for p, a in enumerate(small):
        short.data[p], short.stride[p], short.line_count[p] = a.ctypes.data, a.shape[1], a.shape[0]
    frame = HostFrame((0, 0, 7, 7), np.uint16)
    cvs.video_reconstruct_mpeg2(frame.ref(), C.byref(short))
    assert frame.current_window.is_empty() and _lib.last_error()


def test_same_bits_in_both_arithmetic_flavours(cvs, orc, table):
    rng = np.random.default_rng(5)
    width, height = 1920, 1080
    planes = _random_planes(rng, width, height)
    full = (-4, -4, width + 3, height - 9)
    for interlaced, matrix in MODES:
        before = cvs.cvs_set_arithmetic(_lib.ARITH_CONTRACTED)
        try:
            got_fma = _reconstruct_dev(cvs, planes, width, height, _flags(interlaced, matrix), full)
            cvs.cvs_set_arithmetic(_lib.ARITH_SEPARATE)
            got_sep = _reconstruct_dev(cvs, planes, width, height, _flags(interlaced, matrix), full)
        finally:
            cvs.cvs_set_arithmetic(before if before >= 0 else _lib.ARITH_SEPARATE)
        for name, got in (("contracted", got_fma), ("separate", got_sep)):
            _assert_frame(got, planes, width, height, interlaced, matrix, full, table, orc, "%s %s %s" % (name, interlaced, matrix))


# ---------------------------------------------------------------- the node

@pytest.fixture(scope="module")
def process():
    from fluggo.media import process
    return process


def _tape(process, planes):
    class Tape(process.CodedImageSource):
        def get_frame(self, frame):
            return [process.CodedImage(bytearray(np.ascontiguousarray(p).tobytes()), p.shape[1], p.shape[0]) for p in planes]
    return Tape()


def _assert_pulled(frame, want, full, what):
    """A pulled RgbaFrameF16 against model codes over `full`: pixel() gives the halfs as floats (NaN-free here)."""
    w = frame.current_window
    assert (w.min.x, w.min.y, w.max.x, w.max.y) == full, what
    floats = want.view(np.float16).astype(np.float64)
    for y in range(full[1], full[3] + 1):
        row = np.array([frame.pixel(x, y) for x in range(full[0], full[2] + 1)])
        assert np.array_equal(row, floats[y - full[1]]), "%s: row %d" % (what, y)


@pytest.mark.parametrize("size,interlaced,matrix", [(None, True, "601"), ((130, 24), False, "709"), ((64, 36), True, "709"),
                                                    ((6, 6), False, "601")])
def test_node_equals_the_model(process, orc, table, size, interlaced, matrix):
    from fluggo.media import basetypes as bt
    width, height = size or (720, 480)
    rng = np.random.default_rng(width + height)
    planes = _random_planes(rng, width, height, pads=(3, 1, 0), extra_lines=(0, 2, 0))
    kw = {} if size is None else {"size": size, "interlaced": interlaced, "matrix": matrix}
    node = process.MPEG2ReconstructionFilter(_tape(process, planes), **kw)
    raster = reconstruct_model(planes, width, height, table, orc.float_to_half, interlaced, matrix)
    full = (0, 0, width - 1, min(height - 1, 23))
    got = node.get_frame_f16(0, bt.box2i(-2, -1, width + 1, full[3]))
    _assert_pulled(got, raster[:full[3] + 1], full, "node %r" % (size,))


def test_node_short_planes_give_an_empty_window(process):
    from fluggo.media import basetypes as bt
    planes = [np.zeros((480, 720), np.uint8), np.zeros((240, 360), np.uint8), np.zeros((240, 359), np.uint8)]
    node = process.MPEG2ReconstructionFilter(_tape(process, planes))
    got = node.get_frame_f16(0, bt.box2i(0, 0, 15, 15))
    assert got.current_window.empty()
    assert process.last_error()


def test_node_in_a_workspace_through_a_pull_queue(process, orc, table):
    from fluggo.media import basetypes as bt
    width, height = 130, 24
    rng = np.random.default_rng(77)
    frames = [_random_planes(rng, width, height) for _ in range(4)]

    class Tape(process.CodedImageSource):
        def get_frame(self, frame):
            return [process.CodedImage(bytearray(p.tobytes()), p.shape[1], p.shape[0]) for p in frames[frame % 4]]

    node = process.MPEG2ReconstructionFilter(Tape(), size=(width, height), interlaced=False, matrix="709")
    ws = process.VideoWorkspace()
    ws.add(source=node, x=0, length=100, z=0, offset=0)
    q = process.VideoPullQueue(workers=2)
    done, seen, lock = threading.Event(), {}, threading.Lock()
    full = (0, 0, width - 1, height - 1)

    def callback(frame_index, frame, user_data):
        with lock:
            try:
                _assert_pulled(frame, reconstruct_model(frames[frame_index % 4], width, height, table, orc.float_to_half, False, "709"), full,
                               "queue frame %d" % frame_index)
                seen[frame_index] = True
            except AssertionError as e:
                seen[frame_index] = str(e)
            if len(seen) == 8:
                done.set()

    items = [q.enqueue(source=ws, frame_index=i, window=bt.box2i(*full), callback=callback, user_data=None) for i in range(8)]
    assert done.wait(60), "callbacks did not arrive"
    assert all(v is True for v in seen.values()), seen
    del items


@pytest.mark.parametrize("size,interlaced", [((720, 480), True), ((1920, 1080), True), ((64, 36), False)])
def test_subsample_of_reconstruction_equals_the_chained_models(process, orc, table, size, interlaced):
    width, height = size
    rng = np.random.default_rng(width)
    planes = _random_planes(rng, width, height)
    recon = process.MPEG2ReconstructionFilter(_tape(process, planes), size=size, interlaced=interlaced)
    coded = process.MPEG2SubsampleFilter(recon, size=size).get_frame(0)
    assert coded is not None, _lib.last_error()
    full = (0, 0, width - 1, height - 1)
    codes = reconstruct_model(planes, width, height, table, orc.float_to_half, interlaced)
    want = mpeg2_subsample_model(codes, full, full, width, height, orc.transfer_table(2))
    for p, plane in enumerate(coded):
        got = np.frombuffer(bytes(plane.data), np.uint8).reshape(plane.line_count, plane.stride)
        assert np.array_equal(got, want[p]), "plane %d" % p
