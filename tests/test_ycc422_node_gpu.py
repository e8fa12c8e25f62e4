"""YCbCr422ReconstructionFilter and YCbCr422SubsampleFilter on the GPU: both nodes against the model (tests/ycc422_model.py) in
every layout, planes that are too short or missing, the constructors' ValueErrors, the import node under a workspace through a
VideoPullQueue, and the export of an import against the chained models."""
import threading

import numpy as np
import pytest

from canvas_amd import _lib
from tests import ycc422_model as ym

pytestmark = pytest.mark.gpu

LAYOUTS = list(ym.LAYOUTS)


@pytest.fixture(scope="module")
def process(cvs):
    from fluggo.media import process
    return process


@pytest.fixture(scope="module")
def tables(orc):
    return orc.transfer_table(0), orc.transfer_table(2), orc.float_to_half


def _random_planes(rng, layout, width, height, pads=(0, 0, 0), extra=(0, 0, 0)):
    strides, lines = ym.least(layout, width, height)
    return [rng.integers(0, 256, (n + e, s + p), dtype=np.uint8) for s, n, p, e in zip(strides, lines, pads, extra)]


def _tape(process, planes):
    class Tape(process.CodedImageSource):
        def get_frame(self, frame):
            return [process.CodedImage(bytearray(np.ascontiguousarray(p).tobytes()), p.shape[1], p.shape[0]) for p in planes]
    return Tape()


def _assert_pulled(frame, want, full, what):
    """A pulled RgbaFrameF16 against model codes over `full`: pixel() gives the halfs as floats (NaNs compared as such)."""
    w = frame.current_window
    assert (w.min.x, w.min.y, w.max.x, w.max.y) == full, what
    floats = want.view(np.float16).astype(np.float64)
    for y in range(full[1], full[3] + 1):
        row = np.array([frame.pixel(x, y) for x in range(full[0], full[2] + 1)])
        assert np.array_equal(row, floats[y - full[1]], equal_nan=True), "%s: row %d" % (what, y)


PADS = {"planar8": (3, 1, 0), "planar10": (6, 2, 0), "uyvy": (5, 0, 0), "v210": (12, 0, 0)}


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("size,matrix", [((130, 9), "709"), ((14, 3), "601"), ((382, 2), None)])
def test_import_node_equals_the_model(process, tables, layout, size, matrix):
    from fluggo.media import basetypes as bt
    width, height = size
    planes = _random_planes(np.random.default_rng(width + height), layout, width, height, PADS[layout], (0, 2, 0))
    kw = {} if matrix is None else {"matrix": matrix}
    node = process.YCbCr422ReconstructionFilter(_tape(process, planes), size, layout, **kw)
    raster = ym.reconstruct_model(layout, planes, width, height, tables[0], tables[2], matrix or "709")
    full = (0, 0, width - 1, height - 1)
    got = node.get_frame_f16(0, bt.box2i(-2, -1, width + 1, height))
    _assert_pulled(got, raster, full, "import node %s %r" % (layout, size))


def _solid_codes(orc, colour, full):
    codes = orc.float_to_half(np.array(colour, np.float32))
    return np.broadcast_to(codes, (full[3] - full[1] + 1, full[2] - full[0] + 1, 4)).copy()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("matrix", ["601", "709"])
def test_export_node_equals_the_model(process, orc, tables, layout, matrix):
    """A solid colour over part of the raster: the planes have the least strides of cvs_ycc422_layout, the model's bytes, and black
    where the source has no pixels."""
    from fluggo.media import basetypes as bt
    width, height = 34, 5
    cur = (3, 1, 20, 3)
    colour = (0.25, 0.5, 0.125, 1.0)
    node = process.YCbCr422SubsampleFilter(process.SolidColorVideoSource(colour, bt.box2i(*cur)), (width, height), layout=layout, matrix=matrix)
    coded = node.get_frame(0)
    assert coded is not None, _lib.last_error()
    strides, lines = ym.least(layout, width, height)
    assert [(p.stride, p.line_count) for p in coded] == list(zip(strides, lines))
    want = ym.subsample_model(layout, _solid_codes(orc, colour, cur), cur, cur, width, height, tables[1], matrix)
    for p, plane in enumerate(coded):
        got = np.frombuffer(bytes(plane.data), np.uint8).reshape(plane.line_count, plane.stride)
        assert np.array_equal(got, want[p]), "%s %s plane %d" % (layout, matrix, p)
    y, cb, cr = ym.unpack(layout, want, width, height)
    s = 1 << (ym.BITS[layout] - 8)
    assert (y[0] == 16 * s).all() and (y[2, 4:20] != 16 * s).all() and (cb[0] == 128 * s).all()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_short_or_missing_planes_give_an_empty_window(process, layout):
    from fluggo.media import basetypes as bt
    width, height = 24, 4
    strides, lines = ym.least(layout, width, height)
    last = len(strides) - 1
    shapes = [[(n, s) for n, s in zip(lines, strides)] for _ in range(3)]
    shapes[0][last] = (lines[last], strides[last] - ym.ALIGN[layout])       # a stride too short
    shapes[1][last] = (lines[last] - 1, strides[last])                        # a line too few
    shapes[2] = shapes[2][:last]                                              # a plane too few (none at all for the packed layouts)
    for shape in shapes:
        node = process.YCbCr422ReconstructionFilter(_tape(process, [np.zeros(s, np.uint8) for s in shape]), (width, height), layout)
        got = node.get_frame_f16(0, bt.box2i(0, 0, 15, 3))
        assert got.current_window.empty(), (layout, shape)
    good = process.YCbCr422ReconstructionFilter(_tape(process, [np.zeros(s, np.uint8) for s in zip(lines, strides)]), (width, height), layout)
    assert not good.get_frame_f16(0, bt.box2i(0, 0, 15, 3)).current_window.empty()


def test_value_errors(process):
    src, solid = _tape(process, [np.zeros((4, 64), np.uint8)]), process.SolidColorVideoSource((0.2, 0.3, 0.4, 1.0))
    for node, source in ((process.YCbCr422ReconstructionFilter, src), (process.YCbCr422SubsampleFilter, solid)):
        for size in [(25, 4), (0, 4), (24, 0), (-2, 4), (1, 1)]:
            with pytest.raises(ValueError):
                node(source, size)
        for layout in ["yuv422p10", "V210", "", 3, None]:
            with pytest.raises(ValueError):
                node(source, (24, 4), layout=layout)
        for matrix in ["2020", "", 709, None]:
            with pytest.raises(ValueError):
                node(source, (24, 4), matrix=matrix)


def test_import_node_in_a_workspace_through_a_pull_queue(process, tables):
    from fluggo.media import basetypes as bt
    width, height, layout = 130, 24, "v210"
    rng = np.random.default_rng(77)
    frames = [_random_planes(rng, layout, width, height) for _ in range(4)]

    class Tape(process.CodedImageSource):
        def get_frame(self, frame):
            return [process.CodedImage(bytearray(p.tobytes()), p.shape[1], p.shape[0]) for p in frames[frame % 4]]

    node = process.YCbCr422ReconstructionFilter(Tape(), size=(width, height))
    ws = process.VideoWorkspace()
    ws.add(source=node, x=0, length=100, z=0, offset=0)
    q = process.VideoPullQueue(workers=2)
    done, seen, lock = threading.Event(), {}, threading.Lock()
    full = (0, 0, width - 1, height - 1)
    want = [ym.reconstruct_model(layout, f, width, height, tables[0], tables[2], "709") for f in frames]

    def callback(frame_index, frame, user_data):
        with lock:
            try:
                _assert_pulled(frame, want[frame_index % 4], full, "queue frame %d" % frame_index)
                seen[frame_index] = True
            except AssertionError as e:
                seen[frame_index] = str(e)
            if len(seen) == 8:
                done.set()

    items = [q.enqueue(source=ws, frame_index=i, window=bt.box2i(*full), callback=callback, user_data=None) for i in range(8)]
    assert done.wait(60), "callbacks did not arrive"
    assert all(v is True for v in seen.values()), seen
    del items


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("size,matrix", [((720, 486), "709"), ((1920, 1080), "601"), ((62, 5), "709")])
def test_export_of_import_equals_the_chained_models(process, tables, layout, size, matrix):
    """The import node's frame is NOT the input's colours again (codes outside the legal range, chroma that is not flat): the
    chained models say what comes back, bit for bit.  The export node may lay the same layout out with the least strides only."""
    width, height = size
    planes = _random_planes(np.random.default_rng(width), layout, width, height)
    recon = process.YCbCr422ReconstructionFilter(_tape(process, planes), size, layout, matrix)
    coded = process.YCbCr422SubsampleFilter(recon, size, layout, matrix).get_frame(0)
    assert coded is not None, _lib.last_error()
    full = (0, 0, width - 1, height - 1)
    codes = ym.reconstruct_model(layout, planes, width, height, tables[0], tables[2], matrix)
    want = ym.subsample_model(layout, codes, full, full, width, height, tables[1], matrix)
    for p, plane in enumerate(coded):
        got = np.frombuffer(bytes(plane.data), np.uint8).reshape(plane.line_count, plane.stride)
        assert np.array_equal(got, want[p]), "%s plane %d" % (layout, p)
