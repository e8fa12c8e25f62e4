"""Field conversions without a GPU: the 2:3 pulldown addition arithmetic and its inverse property against the removal's, the
argument errors the three device entries decide before any device call, the surface of the five nodes, and self-checks of the
numpy model of the contract (tests/fields_model.py, DESIGN.md "Field conversions")."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import fields_model as fm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODES = ["DeinterlaceFilter", "BobDeinterlaceFilter", "WeaveInterlaceFilter", "BobInterlaceFilter", "Pulldown23AdditionFilter"]


@pytest.fixture(scope="module")
def lib():
    from canvas_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def process():
    from fluggo.media import process
    return process


# ---------------------------------------------------------------- 2:3 pulldown addition

def _add(lib, offset, i):
    e, o = C.c_int(-99), C.c_int(-99)
    rc = lib.cvs_pulldown23_add_frames(offset, i, C.byref(e), C.byref(o))
    return rc, e.value, o.value


def test_pulldown_add_table(lib):
    table = [(0, 0), (1, 1), (1, 2), (2, 3), (3, 3)]
    shift = [0, 1, 2, 3, 3]
    for offset in range(5):
        for i in range(-40, 41):
            k, r = divmod(i + offset, 5)                       # floor, not truncation
            want = (4 * k + table[r][0] - shift[offset], 4 * k + table[r][1] - shift[offset])
            rc, e, o = _add(lib, offset, i)
            assert (e, o) == want == fm.pulldown23_add(offset, i), (offset, i)
            assert rc == (1 if e != o else 0), (offset, i)


def test_pulldown_add_refuses_other_offsets(lib):
    from canvas_amd import _lib
    for offset in (-1, 5):
        rc, e, o = _add(lib, offset, 3)
        assert rc == -1 and (e, o) == (-99, -99)
        assert "offset" in _lib.last_error()


def test_pulldown_add_inverts_the_removal(lib):
    """For every output frame j of the removal: a whole frame `first` is a cadence frame that shows j on both fields; a woven one
    takes its odd rows from `first` and its even rows from `second`, so those must show j on their odd / even rows.  Offset 4
    where j & 3 != 0 only: there the reference's own offset-4 formula reads another source frame (its slip, left alone)."""
    first, second = C.c_int(), C.c_int()
    checked = 0
    for offset in range(5):
        for j in range(-40, 40):
            if offset == 4 and (j & 3) == 0:
                continue
            mixed = lib.cvs_pulldown23_frames(offset, j, C.byref(first), C.byref(second))
            if mixed:
                assert _add(lib, offset, first.value)[2] == j, (offset, j)
                assert _add(lib, offset, second.value)[1] == j, (offset, j)
            else:
                assert _add(lib, offset, first.value)[1:] == (j, j), (offset, j)
            checked += 1
    assert checked == 4 * 80 + 60


# ---------------------------------------------------------------- the device entries' refusals

def test_entry_points_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "canvas_hip.h")).read()
    for decl in [r"int cvs_field_to_frame_f16_dev\(rgba_frame_f16 \*out, const rgba_frame_f16 \*in, int field, cvs_stream_t stream\);",
                 r"int cvs_soften_fields_f16_dev\(rgba_frame_f16 \*out, const rgba_frame_f16 \*in, cvs_stream_t stream\);",
                 r"int cvs_interlace_fields_f16_dev\(rgba_frame_f16 \*out, const rgba_frame_f16 \*even, const rgba_frame_f16 \*odd, cvs_stream_t stream\);",
                 r"int cvs_pulldown23_add_frames\(int offset, int frame_index, int \*even_source, int \*odd_source\);"]:
        assert re.search(r"CVS_EXPORT " + decl, header), decl
    assert "do not depend on cvs_set_arithmetic" in header          # the flavours are bit-equal, and the header says so
    from canvas_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("cvs_field_to_frame_f16_dev", "cvs_soften_fields_f16_dev", "cvs_interlace_fields_f16_dev", "cvs_pulldown23_add_frames"):
        assert hasattr(raw, name) and name in _lib.SIGNATURES, name


def _calls(lib):
    return [("field", lambda out, a, b: lib.cvs_field_to_frame_f16_dev(out, a, 0, None)),
            ("soften", lambda out, a, b: lib.cvs_soften_fields_f16_dev(out, a, None)),
            ("interlace", lambda out, a, b: lib.cvs_interlace_fields_f16_dev(out, a, b, None))]


def _refused(rc, out):
    from canvas_amd import _lib
    return rc == -1 and bool(_lib.last_error()) and out.current_window.is_empty()


def test_device_entries_refuse_bad_arguments(lib):
    from canvas_amd import _lib
    from canvas_amd.abi import HostFrame
    full = (0, 0, 7, 7)
    for name, call in _calls(lib):
        out, a, b = HostFrame(full, np.uint16), HostFrame(full, np.uint16), HostFrame(full, np.uint16)
        lib.cvs_clear_last_error()
        assert _refused(call(out.ref(), out.ref(), out.ref()), out), name + ": out == in"
        out = HostFrame(full, np.uint16)
        lib.cvs_clear_last_error()
        assert _refused(call(out.ref(), None, None), out), name + ": NULL input"
        lib.cvs_clear_last_error()
        assert call(None, a.ref(), b.ref()) == -1 and _lib.last_error(), name + ": NULL output"
        out, outside = HostFrame(full, np.uint16), HostFrame(full, np.uint16, current_window=(0, 0, 8, 7))
        lib.cvs_clear_last_error()
        assert _refused(call(out.ref(), outside.ref(), outside.ref()), out), name + ": current_window outside the buffer"
    for field in (-1, 2, 7):
        out, a = HostFrame(full, np.uint16), HostFrame(full, np.uint16)
        lib.cvs_clear_last_error()
        assert _refused(lib.cvs_field_to_frame_f16_dev(out.ref(), a.ref(), field, None), out), field
        assert "field" in _lib.last_error()
    out, a, outside = HostFrame(full, np.uint16), HostFrame(full, np.uint16), HostFrame(full, np.uint16, current_window=(-1, 0, 3, 3))
    lib.cvs_clear_last_error()
    assert _refused(lib.cvs_interlace_fields_f16_dev(out.ref(), a.ref(), outside.ref(), None), out)       # the odd input alone


# ---------------------------------------------------------------- the nodes' surface

def _make(process, name, source, **kw):
    if name == "Pulldown23AdditionFilter":
        kw.setdefault("offset", 0)
    return getattr(process, name)(source, **kw)


@pytest.mark.parametrize("name", NODES)
def test_node_surface(process, name):
    red = process.SolidColorVideoSource((1, 0, 0, 1))
    cls = getattr(process, name)
    assert issubclass(cls, process.VideoSource)
    node = _make(process, name, red)
    cap = node._video_frame_source_funcs
    assert type(cap).__name__ == "PyCapsule" and '"_video_frame_source_funcs"' in repr(cap)
    assert node.source is red
    other = process.SolidColorVideoSource((0, 1, 0, 1))
    node.set_source(other)
    assert node.source is other
    node.source = red
    assert node.source is red
    node.set_source(None)
    assert node.source is None
    for bad in (object(), 3, "source"):
        with pytest.raises(Exception):
            _make(process, name, bad)
        with pytest.raises(Exception):
            node.set_source(bad)


def test_node_arguments(process):
    red = process.SolidColorVideoSource((1, 0, 0, 1))
    assert process.DeinterlaceFilter(red).field == 0 and process.DeinterlaceFilter(red, field=1).field == 1
    assert process.BobDeinterlaceFilter(red).first_field == 0 and process.BobDeinterlaceFilter(red, first_field=1).first_field == 1
    assert process.BobInterlaceFilter(red).first_field == 0 and process.BobInterlaceFilter(red, 1).first_field == 1
    assert [process.Pulldown23AdditionFilter(red, o).offset for o in range(5)] == list(range(5))
    for cls, kw in [(process.DeinterlaceFilter, "field"), (process.BobDeinterlaceFilter, "first_field"), (process.BobInterlaceFilter, "first_field")]:
        for bad in (-1, 2):
            with pytest.raises(ValueError):
                cls(red, **{kw: bad})
    for bad in (-1, 5):
        with pytest.raises(ValueError):
            process.Pulldown23AdditionFilter(red, bad)
    with pytest.raises(TypeError):
        process.Pulldown23AdditionFilter(red)                      # the cadence phase has no default
    with pytest.raises(TypeError):
        process.WeaveInterlaceFilter(red, 1)


# ---------------------------------------------------------------- the model

def _codes(rng, h, w):
    """Finite half codes of both signs, subnormals and zeros among them."""
    codes = rng.integers(0, 0x7C00, (h, w, 4), dtype=np.uint16)
    codes |= (rng.integers(0, 2, (h, w, 4), dtype=np.uint16) << 15)
    codes[rng.uniform(size=(h, w, 4)) < 0.05] = 0
    codes[rng.uniform(size=(h, w, 4)) < 0.05] = 0x8000
    codes[rng.uniform(size=(h, w, 4)) < 0.05] = 0x0001
    return codes


@pytest.mark.parametrize("y0", [0, 1, -1, -6])
def test_model_kept_rows_are_identical(orc, y0):
    rng = np.random.default_rng(30 + y0)
    cur = _codes(rng, 9, 5)
    cur[2, 1] = [0x7C00, 0xFC00, 0x7E01, 0xFFFF]                    # Inf, -Inf and two NaNs travel unchanged on a kept row
    for field in (0, 1):
        out = fm.field_to_frame(cur, y0, field, orc.float_to_half)
        kept = ((np.arange(y0, y0 + 9) & 1) == field)
        assert np.array_equal(out[kept], cur[kept])
        assert not np.array_equal(out[~kept], cur[~kept])


def test_model_edge_rows_copy_their_only_neighbour(orc):
    rng = np.random.default_rng(5)
    cur = _codes(rng, 4, 3)
    out = fm.field_to_frame(cur, 0, 1, orc.float_to_half)           # rows 0, 2 made; row 0 has only row 1 below it
    assert np.array_equal(out[0], cur[1])
    out = fm.field_to_frame(cur, 0, 0, orc.float_to_half)           # rows 1, 3 made; row 3 has only row 2 above it
    assert np.array_equal(out[3], cur[2])
    one = _codes(rng, 1, 3)
    assert not fm.field_to_frame(one, 4, 1, orc.float_to_half).any()        # a one-row window of the other parity: zeros
    assert np.array_equal(fm.field_to_frame(one, 4, 0, orc.float_to_half), one)


def test_model_flat_frames_come_back_unchanged(orc):
    rng = np.random.default_rng(7)
    row = _codes(rng, 1, 6)
    row[row == 0x8000] = 0                                          # (-0 * 0.25 + ...) keeps its sign too, but keep the check plain
    flat = np.repeat(row, 8, axis=0)
    for y0 in (0, -3):
        for field in (0, 1):
            assert np.array_equal(fm.field_to_frame(flat, y0, field, orc.float_to_half), flat)
    assert np.array_equal(fm.soften(flat, orc.float_to_half), flat)
    full = (2, -3, 7, 4)
    frame = (flat, full, full)
    assert np.array_equal(fm.interlace(frame, frame, full), flat)


@pytest.mark.parametrize("y0", [0, -5])
def test_model_fields_woven_back_give_the_frame(orc, y0):
    rng = np.random.default_rng(11)
    cur = _codes(rng, 10, 7)
    full = (3, y0, 9, y0 + 9)
    even = (fm.field_to_frame(cur, y0, 0, orc.float_to_half), full, full)
    odd = (fm.field_to_frame(cur, y0, 1, orc.float_to_half), full, full)
    assert np.array_equal(fm.interlace(even, odd, full), cur)


def test_model_interpolated_values_lie_between_their_inputs(orc):
    rng = np.random.default_rng(13)
    cur = _codes(rng, 64, 16)
    out = fm.field_to_frame(cur, 0, 0, orc.float_to_half)
    up, lo, got = fm.widen(cur[0:-2:2]), fm.widen(cur[2::2]), fm.widen(out[1:-1:2])
    assert (got >= np.minimum(up, lo)).all() and (got <= np.maximum(up, lo)).all()


def test_model_soften_weights(orc):
    cur = np.zeros((5, 1, 4), np.uint16)
    cur[2] = 0x3C00                                                 # 1.0 on one row
    got = fm.widen(fm.soften(cur, orc.float_to_half))[:, 0, 0]
    assert got.tolist() == [0.0, 0.25, 0.5, 0.25, 0.0]
    cur[:] = 0
    cur[0] = 0x3C00                                                 # the top row stands in for its missing neighbour: 1/4 + 1/2
    assert fm.widen(fm.soften(cur, orc.float_to_half))[:, 0, 0].tolist() == [0.75, 0.25, 0.0, 0.0, 0.0]


def test_model_interlace_windows():
    full = (0, 0, 5, 5)
    a = (np.full((6, 6, 4), 0x1111, np.uint16), full, (1, 1, 3, 4))
    b = (np.full((6, 6, 4), 0x2222, np.uint16), full, (2, 0, 5, 2))
    before = np.full((8, 8, 4), 0x7E17, np.uint16)
    after, window = fm.expected_interlace(before, (-1, -1, 6, 6), a, b)
    assert window == (1, 0, 5, 4)
    got = after[..., 0]
    assert got[1 + 2, 1 + 1] == 0x1111 and got[1 + 1, 1 + 2] == 0x2222        # (1, 2) from a, (2, 1) from b
    assert got[1 + 0, 1 + 2] == 0 and got[1 + 3, 1 + 2] == 0                  # row 0 is even: a has no row 0; row 3 odd: b ends at 2
    assert got[0, 0] == 0x7E17 and got[1 + 5, 1 + 1] == 0x7E17                # outside the window: kept
    empty = (a[0], full, None)
    assert fm.expected_interlace(before, (-1, -1, 6, 6), empty, empty)[1] is None
    assert fm.expected_interlace(before, (-1, -1, 6, 6), empty, b)[1] == (2, 0, 5, 2)
