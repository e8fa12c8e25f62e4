"""MPEG2ReconstructionFilter without a GPU: the node's surface and argument checks, the two C entry points in the header and the
library, and the numpy model of the contract (DESIGN.md "MPEG-2 4:2:0 reconstruction") pinned against studio-range anchors,
the two chroma sitings, a float64 restatement and a round trip through the subsample's model."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.mpeg2_model import mpeg2_subsample_model
from tests.mpeg2_reconstruct_model import (MATRICES, decode_chroma, reconstruct_halves, reconstruct_model, rgb, vertical)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    return orc.transfer_table(0)            # Rec.709 -> linear (scene) (CVS_LUT_REC709_TO_LINEAR_SCENE)


def _planes(y, cb, cr):
    return [np.asarray(p, np.uint8) for p in (y, cb, cr)]


def _coded_source(process):
    class Planes(process.CodedImageSource):
        def get_frame(self, frame):
            return [process.CodedImage(bytearray(16 * 16), 16, 16)] * 3
    return Planes()


def test_node_surface(process):
    from fluggo.media.basetypes import v2i
    src = _coded_source(process)
    node = process.MPEG2ReconstructionFilter(src)
    assert issubclass(process.MPEG2ReconstructionFilter, process.VideoSource)
    cap = node._video_frame_source_funcs
    assert type(cap).__name__ == "PyCapsule" and '"_video_frame_source_funcs"' in repr(cap)
    process.MPEG2ReconstructionFilter(src, size=(1920, 1080))
    process.MPEG2ReconstructionFilter(src, size=v2i(2, 4))
    process.MPEG2ReconstructionFilter(src, size=(2, 2), interlaced=False)
    process.MPEG2ReconstructionFilter(src, size=(1920, 1082), interlaced=False, matrix="709")
    process.MPEG2ReconstructionFilter(source=src, size=(3840, 2160), interlaced=True, matrix="601")


def test_node_refuses_bad_sources_sizes_and_matrices(process):
    src = _coded_source(process)
    with pytest.raises(Exception):
        process.MPEG2ReconstructionFilter(process.SolidColorVideoSource((0.2, 0.3, 0.4, 1.0)))   # a video source is not coded
    with pytest.raises(Exception):
        process.MPEG2ReconstructionFilter(object())
    for size in [(721, 480), (720, 482), (720, 478), (0, 480), (720, 0), (-2, 4), (2, 2), (1, 4)]:
        with pytest.raises(ValueError):
            process.MPEG2ReconstructionFilter(src, size=size)
    for size in [(721, 480), (720, 481), (0, 2), (2, 0), (-2, 2), (1, 2)]:
        with pytest.raises(ValueError):
            process.MPEG2ReconstructionFilter(src, size=size, interlaced=False)
    for matrix in ["2020", "", "rec709", 601, 709, None, b"601"]:
        with pytest.raises(ValueError):
            process.MPEG2ReconstructionFilter(src, matrix=matrix)
    with pytest.raises(Exception):
        process.MPEG2ReconstructionFilter(src, size=(720,))


def test_without_a_gpu_the_pull_is_empty_or_loud(process):
    from canvas_amd import _lib
    if _lib.load().cvs_device_count() > 0:
        pytest.skip("a GPU is present")
    node = process.MPEG2ReconstructionFilter(_coded_source(process), size=(16, 16))
    from fluggo.media.basetypes import box2i
    try:
        frame = node.get_frame_f16(0, box2i(0, 0, 15, 15))
    except Exception:
        return
    assert frame.current_window.empty()
    assert process.last_error()


def test_entry_points_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "canvas_hip.h")).read()
    assert re.search(r"CVS_EXPORT int cvs_reconstruct_mpeg2_dev\(rgba_frame_f16 \*frame, const coded_image \*planar, int width, int height, "
                     r"int flags, cvs_stream_t stream\);", header)
    assert re.search(r"CVS_EXPORT void video_reconstruct_mpeg2\(rgba_frame_f16 \*frame, coded_image \*planar\);", header)
    assert re.search(r"CVS_YCC_PROGRESSIVE = 1, CVS_YCC_REC709 = 2", header)
    from canvas_amd import _lib
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("cvs_reconstruct_mpeg2_dev", "video_reconstruct_mpeg2"):
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES
    assert (_lib.YCC_PROGRESSIVE, _lib.YCC_REC709) == (1, 2)


def test_without_a_gpu_the_device_entry_refuses_or_is_empty():
    from canvas_amd import _lib
    from canvas_amd.abi import HostFrame
    lib = _lib.load()
    frame = HostFrame((0, 0, 7, 7), np.uint16)
    img = _lib.coded_image()
    assert lib.cvs_reconstruct_mpeg2_dev(frame.ref(), C.byref(img), 7, 8, 0, None) == -1     # odd width: refused in any case
    w = frame.current_window
    assert w.max.x < w.min.x


# ---------------------------------------------------------------- the model

@pytest.mark.parametrize("matrix", ["601", "709"])
@pytest.mark.parametrize("interlaced", [True, False])
def test_model_black_and_white_anchors(orc, table, matrix, interlaced):
    for luma, want in ((16, 0.0), (235, 1.0)):
        planes = _planes(np.full((8, 6), luma), np.full((4, 3), 128), np.full((4, 3), 128))
        halves = reconstruct_halves(planes, 6, 8, orc.float_to_half, interlaced, matrix)
        assert (halves[..., :3] == orc.float_to_half(np.array([want], np.float32))[0]).all()
        got = reconstruct_model(planes, 6, 8, table, orc.float_to_half, interlaced, matrix)
        assert (got[..., 3] == table[0x3C00]).all()
        if luma == 16:
            assert (got[..., :3] == table[0]).all() and table[0] == 0
        else:
            assert (got[..., :3] == table[0x3C00]).all()
            assert np.float16(table[0x3C00:0x3C01].view(np.float16)[0]) == np.float16(1.0)


def test_model_interlaced_siting():
    """Chroma plane row 2 (field 0, field row 1) alone non-zero: it reaches luma rows 4 (7/8) and 6 (5/8) as the near row, rows
    2 (3/8) and 8 (1/8) as the far one, and no row of field 1."""
    height = 16
    plane = np.zeros((8, 3), np.float32)
    plane[2] = 0.5
    v = vertical(plane, height, True)[:, 0]
    want = np.zeros(height, np.float32)
    want[[4, 6, 2, 8]] = [0.5 * 7 / 8, 0.5 * 5 / 8, 0.5 * 3 / 8, 0.5 * 1 / 8]
    assert np.array_equal(v, want)
    plane[2], plane[3] = 0, 0.5                                # field 1, field row 1: rows 7 (7/8), 5 (5/8), 9 (3/8), 3 (1/8)
    v = vertical(plane, height, True)[:, 0]
    want[:] = 0
    want[[7, 5, 9, 3]] = [0.5 * 7 / 8, 0.5 * 5 / 8, 0.5 * 3 / 8, 0.5 * 1 / 8]
    assert np.array_equal(v, want)


def test_model_progressive_siting():
    height = 16
    plane = np.zeros((8, 3), np.float32)
    plane[3] = 0.5                                              # rows 6, 7 near (3/4); 5 and 8 far (1/4)
    v = vertical(plane, height, False)[:, 0]
    want = np.zeros(height, np.float32)
    want[[6, 7, 5, 8]] = [0.375, 0.375, 0.125, 0.125]
    assert np.array_equal(v, want)


def test_model_edges_clamp():
    plane = np.zeros((4, 2), np.float32)
    plane[0] = 1.0                                              # field 0, field row 0: row 0 takes it near and, clamped, far
    assert vertical(plane, 8, True)[0, 0] == 1.0
    assert vertical(plane, 8, False)[0, 0] == 1.0               # progressive row 0: c = 0 near, c - 1 clamped to 0
    planes = _planes(np.full((4, 4), 128), np.array([[128, 240], [128, 240]]), np.full((2, 2), 128))
    r, g, b = rgb(planes, 4, 4)
    assert b[0, 3] == b[0, 2]                                   # the last odd column averages column W/2 - 1 with itself


def test_model_flat_planes_do_not_depend_on_the_siting(orc, table):
    rng = np.random.default_rng(4)
    y = rng.integers(0, 256, (16, 12))
    planes = _planes(y, np.full((8, 6), 77), np.full((8, 6), 201))
    for matrix in ("601", "709"):
        a = reconstruct_model(planes, 12, 16, table, orc.float_to_half, True, matrix)
        b = reconstruct_model(planes, 12, 16, table, orc.float_to_half, False, matrix)
        assert np.array_equal(a, b)
    cb = rng.integers(0, 256, (8, 6))
    planes[1] = cb.astype(np.uint8)
    assert not np.array_equal(reconstruct_model(planes, 12, 16, table, orc.float_to_half, True),
                              reconstruct_model(planes, 12, 16, table, orc.float_to_half, False))


@pytest.mark.parametrize("matrix", ["601", "709"])
@pytest.mark.parametrize("interlaced", [True, False])
def test_model_against_a_float64_restatement(orc, matrix, interlaced):
    """The model's halves before the table against the contract restated in float64: per field (or per frame) a two-row linear
    interpolation at the chroma sample's position, a horizontal average between even-column samples, a matrix product.  Only the
    rounding differs: every truncated half lies within one half ulp of the float64 value."""
    rng = np.random.default_rng(23 + interlaced)
    height, width = 24, 20
    planes = _planes(rng.integers(0, 256, (height, width)), rng.integers(0, 256, (height // 2, width // 2)),
                     rng.integers(0, 256, (height // 2, width // 2)))
    got = reconstruct_halves(planes, width, height, orc.float_to_half, interlaced, matrix)[..., :3]
    got = got.view(np.float16).astype(np.float64)
    yf = (planes[0].astype(np.float64) - 16) / 219
    chroma = []
    for p in planes[1:]:
        c = (p.astype(np.float64) - 128) / 224
        v = np.empty((height, width // 2))
        if interlaced:
            for f in (0, 1):
                rows = c[f::2]                                  # the field's chroma rows, at field lines 2j + 1/4 (f0), 2j + 3/4 (f1)
                pos = 2 * np.arange(rows.shape[0]) + (0.25 if f == 0 else 0.75)
                for line in range(height // 2):
                    v[2 * line + f] = _interp(rows, pos, line)
        else:
            pos = 2 * np.arange(c.shape[0]) + 0.5               # chroma row c between luma rows 2c and 2c + 1
            for y in range(height):
                v[y] = _interp(c, pos, y)
        h = np.empty((height, width))
        h[:, 0::2] = v
        h[:, 1::2] = (v + np.concatenate([v[:, 1:], v[:, -1:]], axis=1)) / 2
        chroma.append(h)
    m = np.array(MATRICES[matrix])
    want = np.stack([m[i, 0] * yf + m[i, 1] * chroma[0] + m[i, 2] * chroma[1] for i in range(3)], axis=-1)
    ulp = np.maximum(np.abs(want), 2.0 ** -14) * 2.0 ** -10
    assert (np.abs(got - want) <= ulp * 1.001).all()


def _interp(rows, pos, line):
    """Linear interpolation between the two sample rows around `line` (clamped at the ends), in float64."""
    if line <= pos[0]:
        return rows[0]
    if line >= pos[-1]:
        return rows[-1]
    k = np.searchsorted(pos, line) - 1
    t = (line - pos[k]) / (pos[k + 1] - pos[k])
    return rows[k] * (1 - t) + rows[k + 1] * t


@pytest.mark.parametrize("interlaced", [True, False])
def test_model_round_trip_through_the_subsample_model(orc, table, interlaced):
    """planes -> this model -> the subsample's model: with flat chroma and in-gamut colours every byte comes back.  The two tables
    are inverses on these codes and the half truncation stays far inside a byte's step, so the round trip is exact (pinned: a
    tolerance of one byte would hide a siting or matrix slip that moves a few bytes)."""
    rng = np.random.default_rng(31)
    height, width = 32, 24
    encode = orc.transfer_table(2)                              # linear -> Rec.709, the subsample's table
    worst = 0
    for cb, cr in [(128, 128), (120, 136), (140, 118), (110, 126)]:
        planes = _planes(rng.integers(64, 190, (height, width)), np.full((height // 2, width // 2), cb), np.full((height // 2, width // 2), cr))
        r, g, b = rgb(planes, width, height, interlaced)
        assert min(r.min(), g.min(), b.min()) >= 0 and max(r.max(), g.max(), b.max()) <= 1
        codes = reconstruct_model(planes, width, height, table, orc.float_to_half, interlaced)
        full = (0, 0, width - 1, height - 1)
        back = mpeg2_subsample_model(codes, full, full, width, height, encode)
        for p, q in zip(planes, back):
            d = np.abs(p.astype(int) - q.astype(int))
            worst = max(worst, int(d.max()))
    assert worst == 0
