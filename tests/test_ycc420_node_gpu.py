"""YCbCr420ReconstructionFilter and YCbCr420SubsampleFilter on the GPU: both nodes at 16 x 8 and 130 x 6 against the model
(tests/ycc420_model.py) through get_frame, in every layout and with every keyword's values; an NV12 source with a decoder-style
pitch; import followed by export as a graph against the chained models; planes that are too short or missing; each keyword's bad
values."""
import numpy as np
import pytest

from canvas_amd import _lib
from tests import ycc420_model as ym

pytestmark = pytest.mark.gpu

LAYOUTS = list(ym.LAYOUTS)
SIZES = [(16, 8), (130, 6)]
# keyword sets that between them name every value of every keyword
KEYWORDS = [dict(), dict(matrix="601", range="full", siting="center", transfer="none"), dict(matrix="2020", range="studio", siting="topleft", transfer="709"),
            dict(matrix="709", range="full", siting="left", transfer="709")]


@pytest.fixture(scope="module")
def process(cvs):
    from fluggo.media import process
    return process


@pytest.fixture(scope="module")
def tables(orc):
    return orc.transfer_table(0), orc.transfer_table(2), orc.float_to_half


def _model_args(kw):
    return kw.get("matrix", "709"), kw.get("range", "studio"), kw.get("siting", "left"), kw.get("transfer", "709")


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


PADS = {"planar8": (3, 1, 0), "planar10": (6, 2, 0), "nv12": (5, 3), "p010": (6, 2)}


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("size", SIZES)
def test_import_node_equals_the_model(process, tables, layout, size):
    from fluggo.media import basetypes as bt
    width, height = size
    planes = _random_planes(np.random.default_rng(width + height), layout, width, height, PADS[layout], (0, 2, 0))
    full = (0, 0, width - 1, height - 1)
    for kw in KEYWORDS:
        node = process.YCbCr420ReconstructionFilter(_tape(process, planes), size, layout, **kw)
        raster = ym.reconstruct_model(layout, planes, width, height, tables[0], tables[2], *_model_args(kw))
        got = node.get_frame_f16(0, bt.box2i(-2, -1, width + 1, height))
        _assert_pulled(got, raster, full, "import node %s %r %r" % (layout, size, kw))


def test_the_default_layout_is_nv12_and_a_decoder_pitch_is_fine(process, tables):
    """130 columns in surfaces of pitch 256, as a hardware decoder hands them out, with lines beyond the picture's."""
    from fluggo.media import basetypes as bt
    width, height = 130, 6
    rng = np.random.default_rng(256)
    planes = [rng.integers(0, 256, (8, 256), dtype=np.uint8), rng.integers(0, 256, (4, 256), dtype=np.uint8)]
    node = process.YCbCr420ReconstructionFilter(_tape(process, planes), (width, height))
    raster = ym.reconstruct_model("nv12", planes, width, height, tables[0], tables[2])
    _assert_pulled(node.get_frame_f16(0, bt.box2i(0, 0, width - 1, height - 1)), raster, (0, 0, width - 1, height - 1), "NV12, pitch 256")


def _solid_codes(orc, colour, full):
    codes = orc.float_to_half(np.array(colour, np.float32))
    return np.broadcast_to(codes, (full[3] - full[1] + 1, full[2] - full[0] + 1, 4)).copy()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("size", SIZES)
def test_export_node_equals_the_model(process, orc, tables, layout, size):
    """A solid colour over part of the raster: the planes have the least strides of cvs_ycc420_layout, the model's bytes, and black
    where the source has no pixels."""
    from fluggo.media import basetypes as bt
    width, height = size
    cur = (3, 1, width - 5, height - 2)
    colour = (0.25, 0.5, 0.125, 1.0)
    strides, lines = ym.least(layout, width, height)
    for kw in KEYWORDS:
        node = process.YCbCr420SubsampleFilter(process.SolidColorVideoSource(colour, bt.box2i(*cur)), size, layout=layout, **kw)
        coded = node.get_frame(0)
        assert coded is not None, _lib.last_error()
        assert [(p.stride, p.line_count) for p in coded] == list(zip(strides, lines))
        want = ym.subsample_model(layout, _solid_codes(orc, colour, cur), cur, cur, width, height, tables[1], *_model_args(kw))
        for p, plane in enumerate(coded):
            got = np.frombuffer(bytes(plane.data), np.uint8).reshape(plane.line_count, plane.stride)
            assert np.array_equal(got, want[p]), "%s %r plane %d" % (layout, kw, p)
        y, cb, cr = ym.unpack(layout, want, width, height)
        s = 1 << (ym.BITS[layout] - 8)
        black = 0 if kw.get("range") == "full" else 16 * s
        assert (y[0] == black).all() and (y[2, 4:width - 6] != black).all() and (cb[0, -1] == 128 * s).all()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("size", SIZES)
def test_export_of_import_as_a_graph_equals_the_chained_models(process, tables, layout, size):
    """The import node's frame is NOT the input's colours again (codes outside the legal range, chroma that is not flat): the
    chained models say what comes back, bit for bit."""
    width, height = size
    planes = _random_planes(np.random.default_rng(width), layout, width, height)
    full = (0, 0, width - 1, height - 1)
    for kw in KEYWORDS:
        recon = process.YCbCr420ReconstructionFilter(_tape(process, planes), size, layout, **kw)
        coded = process.YCbCr420SubsampleFilter(recon, size, layout, **kw).get_frame(0)
        assert coded is not None, _lib.last_error()
        codes = ym.reconstruct_model(layout, planes, width, height, tables[0], tables[2], *_model_args(kw))
        want = ym.subsample_model(layout, codes, full, full, width, height, tables[1], *_model_args(kw))
        for p, plane in enumerate(coded):
            got = np.frombuffer(bytes(plane.data), np.uint8).reshape(plane.line_count, plane.stride)
            assert np.array_equal(got, want[p]), "%s %r plane %d" % (layout, kw, p)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_short_or_missing_planes_give_an_empty_window(process, layout):
    from fluggo.media import basetypes as bt
    width, height = 24, 4
    strides, lines = ym.least(layout, width, height)
    last = len(strides) - 1
    shapes = [[(n, s) for n, s in zip(lines, strides)] for _ in range(3)]
    shapes[0][last] = (lines[last], strides[last] - ym.ALIGN[layout])       # a stride too short
    shapes[1][last] = (lines[last] - 1, strides[last])                        # a line too few
    shapes[2] = shapes[2][:last]                                              # a plane too few
    for shape in shapes:
        node = process.YCbCr420ReconstructionFilter(_tape(process, [np.zeros(s, np.uint8) for s in shape]), (width, height), layout)
        got = node.get_frame_f16(0, bt.box2i(0, 0, 15, 3))
        assert got.current_window.empty(), (layout, shape)
    good = process.YCbCr420ReconstructionFilter(_tape(process, [np.zeros(s, np.uint8) for s in zip(lines, strides)]), (width, height), layout)
    assert not good.get_frame_f16(0, bt.box2i(0, 0, 15, 3)).current_window.empty()


def test_each_keywords_bad_values(process):
    src, solid = _tape(process, [np.zeros((4, 64), np.uint8), np.zeros((2, 64), np.uint8)]), process.SolidColorVideoSource((0.2, 0.3, 0.4, 1.0))
    bad = {"layout": ["yuv420p10", "NV12", "", 3, None, "v210"], "matrix": ["bt709", "", 709, None], "range": ["limited", "", 1, None],
           "siting": ["centre", "", 0, None], "transfer": ["pq", "", 709, None]}
    for node, source in ((process.YCbCr420ReconstructionFilter, src), (process.YCbCr420SubsampleFilter, solid)):
        for size in [(25, 4), (0, 4), (24, 0), (-2, 4), (1, 1), (24, 5)]:
            with pytest.raises(ValueError):
                node(source, size)
        for key, values in bad.items():
            for value in values:
                with pytest.raises(ValueError, match=key):
                    node(source, (24, 4), **{key: value})
