"""MPEG2SubsampleFilter without a GPU: the node's surface and argument checks, and the numpy model of the contract
(DESIGN.md "MPEG-2 4:2:0 subsample") pinned against textbook BT.601 bytes and against the interlaced chroma siting."""
import numpy as np
import pytest

from tests.mpeg2_model import encode, mpeg2_subsample_model, subsample_encoded


@pytest.fixture(scope="module")
def process():
    try:
        from fluggo.media import process
    except ImportError:
        import __graft_entry__
        __graft_entry__.build()
        from fluggo.media import process
    return process


@pytest.fixture(scope="module")
def table(orc):
    return orc.transfer_table(2)            # linear -> Rec.709 (CVS_LUT_LINEAR_TO_REC709)


def test_node_surface(process):
    from fluggo.media.basetypes import v2i
    solid = process.SolidColorVideoSource((0.2, 0.3, 0.4, 1.0))
    node = process.MPEG2SubsampleFilter(solid)
    assert issubclass(process.MPEG2SubsampleFilter, process.CodedImageSource)
    cap = node._coded_image_source_funcs
    assert type(cap).__name__ == "PyCapsule" and '"_coded_image_source_funcs"' in repr(cap)
    process.MPEG2SubsampleFilter(solid, size=(1920, 1080))
    process.MPEG2SubsampleFilter(solid, size=v2i(2, 4))
    process.MPEG2SubsampleFilter(source=solid, size=(3840, 2160))


def test_node_refuses_bad_sources_and_sizes(process):
    class Planes(process.CodedImageSource):
        def get_frame(self, frame):
            return None

    solid = process.SolidColorVideoSource((0.2, 0.3, 0.4, 1.0))
    with pytest.raises(Exception):
        process.MPEG2SubsampleFilter(Planes())               # a coded-image source is not a video source
    with pytest.raises(Exception):
        process.MPEG2SubsampleFilter(object())
    for size in [(721, 480), (720, 482), (720, 478), (0, 480), (720, 0), (-2, 4), (2, 2), (1, 4)]:
        with pytest.raises(ValueError):
            process.MPEG2SubsampleFilter(solid, size=size)
    with pytest.raises(Exception):
        process.MPEG2SubsampleFilter(solid, size=(720,))


def test_without_a_gpu_the_pull_is_none_or_loud(process):
    from canvas_amd import _lib
    if _lib.load().cvs_device_count() > 0:
        pytest.skip("a GPU is present")
    node = process.MPEG2SubsampleFilter(process.SolidColorVideoSource((0.2, 0.3, 0.4, 1.0)))
    try:
        got = node.get_frame(0)
    except Exception:
        return
    assert got is None
    assert _lib.last_error()


@pytest.mark.parametrize("rgb,want", [((1, 1, 1), (235, 128, 128)), ((0, 0, 0), (16, 128, 128)), ((1, 0, 0), (81, 90, 240)),
                                      ((0, 1, 0), (145, 54, 34)), ((0, 0, 1), (41, 240, 110))])
def test_model_bt601_anchors(table, rgb, want):
    rgba = np.array(list(rgb) + [1], np.float32).astype(np.float16).view(np.uint16)
    codes = np.broadcast_to(rgba, (8, 6, 4)).copy()
    planes = mpeg2_subsample_model(codes, (0, 0, 5, 7), (0, 0, 5, 7), 6, 8, table)
    assert [p.shape for p in planes] == [(8, 6), (4, 3), (4, 3)]
    assert tuple(int(np.unique(p)[0]) for p in planes) == want and all(np.unique(p).size == 1 for p in planes)


def test_model_undefined_pixels_are_black(table):
    codes = np.full((8, 8, 4), 0x3C00, np.uint16)             # white everywhere in the buffer ...
    planes = mpeg2_subsample_model(codes, (0, 0, 7, 7), (0, 0, -1, -1), 8, 8, table)     # ... but an empty window
    assert [int(np.unique(p)[0]) for p in planes] == [16, 128, 128] and all(np.unique(p).size == 1 for p in planes)


def test_model_interlaced_siting(table):
    """Every luma row its own colour: chroma row 0 must mix luma rows {0 near, 2 far}, chroma row 1 rows {3 near, 1 far}
    (and so on in every group of four) -- not the progressive {0, 1} / {2, 3}."""
    height, width = 8, 4
    rng = np.random.default_rng(7)
    colours = rng.uniform(0.0, 1.0, (height, 3)).astype(np.float16)
    codes = np.zeros((height, width, 4), np.uint16)
    codes[..., :3] = colours.view(np.uint16)[:, None, :]
    planes = mpeg2_subsample_model(codes, (0, 0, width - 1, height - 1), (0, 0, width - 1, height - 1), width, height, table)
    _, cb, cr = encode(codes[:, 0], table)                   # per row (columns are equal)
    f = np.float32

    def mix(plane, near, far):                               # the contract's six taps, left to right, on column-constant rows
        acc = f(3) / f(16) * plane[near]
        for wgt, row in [(f(6) / f(16), near), (f(3) / f(16), near), (f(1) / f(16), far), (f(2) / f(16), far), (f(1) / f(16), far)]:
            acc = f(acc + wgt * plane[row])
        q = f(f(acc * (f(224) / f(255))) + f(128) / f(255))
        return int(np.rint(f(min(max(q, f(0)), f(1))) * f(255)))

    for cy, (near, far, prog_a, prog_b) in enumerate([(0, 2, 0, 1), (3, 1, 2, 3), (4, 6, 4, 5), (7, 5, 6, 7)]):
        for p, plane in ((1, cb), (2, cr)):
            assert (planes[p][cy] == mix(plane, near, far)).all(), (cy, p)
        assert (mix(cb, near, far), mix(cr, near, far)) != (mix(cb, prog_a, prog_b), mix(cr, prog_a, prog_b))


def test_model_left_column_clamps_to_column_zero():
    """Chroma column 0 takes column 0 for its tap at -1: a frame whose column 0 differs from column 1 shows it."""
    y = np.zeros((4, 4), np.float32)
    cb = np.zeros((4, 4), np.float32)
    cb[:, 0] = np.float32(0.5)
    _, got, _ = subsample_encoded(y, cb, cb)
    # taps -1 and 0 both read column 0: (3 + 6)/16 near + (1 + 2)/16 far of 0.5 = 0.375
    want = int(np.rint((np.float32(0.375) * (np.float32(224) / 255) + np.float32(128) / 255) * np.float32(255)))
    assert (got[:, 0] == want).all()


def test_model_against_a_float64_field_restatement(table):
    """The model against the filter stated another way, in float64: a matrix product for the colour, then per field a vertical
    3:1 mix of the field's two lines (the near one on top in field 0, at the bottom in field 1: MPEG-2's interlaced 4:2:0
    siting) and a horizontal [1 2 1] / 4 with the edge clamped.  Only the rounding differs, so bytes agree within one."""
    rng = np.random.default_rng(19)
    height, width = 16, 24
    codes = rng.uniform(0.0, 1.0, (height, width, 4)).astype(np.float16).view(np.uint16)
    got = mpeg2_subsample_model(codes, (0, 0, width - 1, height - 1), (0, 0, width - 1, height - 1), width, height, table)
    rgb = table[codes[..., :3]].view(np.float16).astype(np.float64)
    m = np.array([[0.299, 0.587, 0.114], [-0.168736, -0.331264, 0.5], [0.5, -0.418688, -0.081312]])
    ycc = rgb @ m.T

    def q(v, scale, offset):
        return np.rint(np.clip(v * scale + offset, 0.0, 1.0) * 255.0)

    want = [q(ycc[..., 0], 219 / 255, 16 / 255)]
    for c in (1, 2):
        plane = np.empty((height // 2, width // 2))
        for field in (0, 1):
            lines = ycc[field::2, :, c]                           # the field's own lines
            upper, lower = lines[0::2], lines[1::2]
            v = 0.75 * upper + 0.25 * lower if field == 0 else 0.25 * upper + 0.75 * lower
            left = np.concatenate([v[:, :1], v[:, 1:-1:2]], axis=1)
            plane[field::2] = (left + 2 * v[:, 0::2] + v[:, 1::2]) / 4
        want.append(q(plane, 224 / 255, 128 / 255))
    for g, w in zip(got, want):
        assert g.shape == w.shape and np.abs(g.astype(np.int64) - w.astype(np.int64)).max() <= 1
        assert (g == w).mean() > 0.95
