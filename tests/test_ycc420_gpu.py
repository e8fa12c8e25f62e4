"""The two device entries of include/canvas_ycc420.h on the GPU, bit for bit the model (tests/ycc420_model.py): the catalogue of
tests/ycc420_cases.py -- every layout, siting, range, matrix and transfer setting, the smallest shapes, the widths around a wave's
run and the heights around a strip, padded strides and extra lines, frames larger than, inside and partly off the raster -- in
both arithmetic flavours; tall rasters whose strips hold more than one chroma row; one raster above the table's switch per layout;
then the checks that need no model: PLANAR8 at left siting against cvs_reconstruct_mpeg2_dev, NV12 and P010 against the planar
layouts fed the same samples, and the round trips DESIGN claims.  An expectation covers every byte of every output: the padding
beyond a row's least stride, the lines beyond the least and the frame's pixels outside the raster keep what they held."""
import ctypes as C

import numpy as np
import pytest

from canvas_amd import _lib
from canvas_amd.device import DeviceFrame
from tests import ycc420_cases as yc
from tests import ycc420_model as ym
from tests.entry_cases import PAD, Twin, blank
from tests.test_ycc420_cpu import check_grey_round_trip, flat_round_trip_inputs, grey_round_trip_inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["separate", "contracted"])
def flavour(request, cvs):
    before = cvs.cvs_set_arithmetic(_lib.ARITH_CONTRACTED if request.param == "contracted" else _lib.ARITH_SEPARATE)
    yield request.param
    cvs.cvs_set_arithmetic(before if before >= 0 else _lib.ARITH_SEPARATE)


def _run(cvs, spec):
    """The spec's call on operands with allocations of their own -> (return code, every object's bytes, the frame's window)."""
    twin = Twin(cvs)
    try:
        rc = yc.make_case(cvs, spec)(twin)
        got = twin.collect()
        frame = [o.frame for o in twin.objects if o.frame is not None][0]
        return rc, got, (None if frame.current_window.is_empty() else frame.current_window.tuple())
    finally:
        twin.free()


def _assert_spec(cvs, orc, spec):
    what = yc.name(spec)
    rc, got, window = _run(cvs, spec)
    assert rc == 0, "%s: %s" % (what, _lib.last_error())
    want = yc.expected(spec, orc)
    if spec["direction"] == "reconstruct":
        frame, want_window = want
        assert window == want_window, "%s: window %r, the model's %r" % (what, window, want_window)
        a, b = got[-1].view(np.uint16), frame.reshape(-1)
        if not np.array_equal(a, b):
            bad = np.flatnonzero(a != b)
            raise AssertionError("%s: %d of %d codes differ, first at %d: 0x%04x, the model 0x%04x" % (what, bad.size, a.size, bad[0], a[bad[0]], b[bad[0]]))
        for g, p in zip(got[:-1], yc.planes_in(spec)):
            assert np.array_equal(g, p.reshape(-1)), what + ": an input plane was written"
    else:
        assert np.array_equal(got[0], yc.frame_in(spec).array.view(np.uint8).reshape(-1)), what + ": the frame was written"
        for k, (g, p) in enumerate(zip(got[1:], want)):
            b = p.reshape(-1)
            if not np.array_equal(g, b):
                bad = np.flatnonzero(g != b)
                line, col = divmod(int(bad[0]), spec["strides"][k])
                raise AssertionError("%s: plane %d: %d of %d bytes differ, first at line %d byte %d: 0x%02x, the model 0x%02x" % (
                    what, k, bad.size, g.size, line, col, g[bad[0]], b[bad[0]]))


@pytest.mark.parametrize("layout", yc.LAYOUT_NAMES)
def test_the_catalogue_bit_for_bit_the_model(cvs, orc, flavour, layout):
    """Both entries, every flag value; the same bytes in both arithmetic flavours (the model is one)."""
    for spec in yc.specs(layout):
        _assert_spec(cvs, orc, spec)


@pytest.mark.parametrize("layout", yc.LAYOUT_NAMES)
def test_strips_of_more_than_one_chroma_row(cvs, orc, layout):
    """Tall, narrow rasters (tests/ycc420_cases.py TALL): more row pairs than the launch has waves, so a wave's strip holds
    three chroma rows and the rows above and below move through the register ring; in every siting, both directions."""
    assert cvs.cvs_compute_units() * 6 * 4 * 2 < yc.TALL[1] // 2, "the device has more waves than the raster has row pairs: no strip longer than one row"
    for spec in yc.tall_specs(layout):
        _assert_spec(cvs, orc, spec)


@pytest.mark.parametrize("layout", yc.LAYOUT_NAMES)
def test_a_raster_above_the_switch_stages_the_table(cvs, orc, layout):
    """1280x820 is just above one megapixel: the half table comes from LDS, in 1024-lane workgroups (the catalogue's rasters gather
    it from L2); with the transfer off the placement plays no part and the raster is one more shape."""
    width, height = 1280, 820
    for i, direction in enumerate(("reconstruct", "subsample")):
        for transfer in ("709", "none"):
            spec = yc._spec(layout, direction, i, width, height, yc.PADS[layout][0], yc.EXTRA[0],
                            (-2, -1, width + 1, height) if direction == "subsample" else (0, 0, width - 1, height - 1), 4800 + i)
            _assert_spec(cvs, orc, dict(spec, transfer=transfer))


def test_a_frame_off_the_raster_gives_an_empty_window_and_black_planes(cvs, orc):
    """Reconstruct: 0, an empty window, the frame untouched.  Subsample: the planes of a frame without pixels (legal black)."""
    for layout in yc.LAYOUT_NAMES:
        for direction in ("reconstruct", "subsample"):
            spec = dict(yc.specs(layout)[0], direction=direction, width=14, height=4, full=(40, 2, 47, 6), range="studio")
            spec["strides"], spec["lines"] = ym.least(layout, 14, 4)
            _assert_spec(cvs, orc, spec)
            if direction == "subsample":
                y, cb, cr = ym.unpack(layout, yc.expected(spec, orc), 14, 4)
                s = 1 << (ym.BITS[layout] - 8)
                assert (y == 16 * s).all() and (cb == 128 * s).all() and (cr == 128 * s).all()


# ---------------------------------------------------------------- checks that need no model

def _upload(cvs, arrays):
    ptrs = []
    for a in arrays:
        a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        ptrs.append(cvs.cvs_malloc(max(a.size, 1)))
        assert ptrs[-1]
        _lib.check(cvs.cvs_memcpy_h2d(ptrs[-1], a.ctypes.data, a.size, None), "h2d")
    return ptrs


def _image(ptrs, planes):
    img = _lib.coded_image()
    for p, (ptr, a) in enumerate(zip(ptrs, planes)):
        img.data[p], img.stride[p], img.line_count[p] = ptr, a.shape[1], a.shape[0]
    return img


def _import(cvs, layout, planes, width, height, flags, full=None, entry=None):
    """The frame (codes over `full`, the sentinel where nothing is written) and its window after one import of `planes`."""
    full = (0, 0, width - 1, height - 1) if full is None else full
    ptrs = _upload(cvs, planes)
    frame = DeviceFrame.from_host(blank(True, full))
    try:
        if entry == "mpeg2":
            rc = cvs.cvs_reconstruct_mpeg2_dev(frame.ref(), C.byref(_image(ptrs, planes)), width, height, flags, None)
        else:
            rc = cvs.cvs_reconstruct_420_dev(frame.ref(), C.byref(_image(ptrs, planes)), width, height, ym.LAYOUTS[layout], flags, None)
        assert rc == 0, _lib.last_error()
        _lib.check(cvs.cvs_stream_sync(None), "sync")
        return frame.download().array.copy(), frame.current_window.tuple()
    finally:
        frame.free()
        for p in ptrs:
            cvs.cvs_free(p)


def _export(cvs, layout, codes, width, height, flags, strides=None, lines=None):
    """The planes (uint8 arrays (lines, stride), PAD where nothing is written) after one export of a frame over the raster."""
    from canvas_amd.abi import HostFrame
    full = (0, 0, width - 1, height - 1)
    ls, ll = ym.least(layout, width, height)
    strides, lines = strides or ls, lines or ll
    planes = [np.full((n, s), PAD, np.uint8) for n, s in zip(lines, strides)]
    ptrs = _upload(cvs, planes)
    frame = DeviceFrame.from_host(HostFrame(full, np.uint16, np.ascontiguousarray(codes), full))
    try:
        rc = cvs.cvs_subsample_420_dev(C.byref(_image(ptrs, planes)), frame.ref(), width, height, ym.LAYOUTS[layout], flags, None)
        assert rc == 0, _lib.last_error()
        _lib.check(cvs.cvs_stream_sync(None), "sync")
        for ptr, a in zip(ptrs, planes):
            _lib.check(cvs.cvs_memcpy_d2h(a.ctypes.data, ptr, a.size, None), "d2h")
        return planes
    finally:
        frame.free()
        for p in ptrs:
            cvs.cvs_free(p)


def test_planar8_left_studio_is_the_mpeg2_progressive_import_byte_for_byte(cvs, flavour):
    """On the catalogue's planar8 inputs, whatever flags their cases carry: PLANAR8, left siting, studio range, the transfer on,
    Rec.601 and Rec.709, against cvs_reconstruct_mpeg2_dev with CVS_YCC_PROGRESSIVE.  Code the project did not write for this
    feature says what the new kernel must give."""
    n = 0
    for spec in yc.specs("planar8") + yc.tall_specs("planar8")[:1]:
        if spec["direction"] != "reconstruct":
            continue
        planes, width, height, full = yc.planes_in(spec), spec["width"], spec["height"], spec["full"]
        for matrix_flag in (0, _lib.YCC_REC709):
            got, gw = _import(cvs, "planar8", planes, width, height, matrix_flag, full)
            want, ww = _import(cvs, None, planes, width, height, matrix_flag | _lib.YCC_PROGRESSIVE, full, entry="mpeg2")
            assert gw == ww and np.array_equal(got, want), yc.name(spec)
            n += 1
    assert n > 60


@pytest.mark.parametrize("semi,planar", [("nv12", "planar8"), ("p010", "planar10")])
def test_the_semi_planar_layouts_equal_the_planar_ones_fed_the_same_samples(cvs, semi, planar):
    """The catalogue's semi-planar inputs, de-interleaved (and, P010, shifted down by 6) into planar planes: the same pixels, in
    every case's own flags; and the other way round for the export, the same codes.  The layout paths differ only in addressing."""
    for spec in yc.specs(semi):
        width, height, flags = spec["width"], spec["height"], yc.flags(spec)
        if spec["direction"] == "reconstruct":
            planes = yc.planes_in(spec)
            y, cb, cr = ym.unpack(semi, planes, width, height)
            a, aw = _import(cvs, semi, planes, width, height, flags, spec["full"])
            b, bw = _import(cvs, planar, ym.pack(planar, y, cb, cr), width, height, flags, spec["full"])
            assert aw == bw and np.array_equal(a, b), yc.name(spec)
        elif spec["full"] == (0, 0, width - 1, height - 1):
            codes = yc.frame_in(spec).array
            a = ym.unpack(semi, _export(cvs, semi, codes, width, height, flags, spec["strides"], spec["lines"]), width, height)
            b = ym.unpack(planar, _export(cvs, planar, codes, width, height, flags), width, height)
            for u, v in zip(a, b):
                assert np.array_equal(u, v), yc.name(spec)


def _device_round_trip(cvs, layout, y, cb, cr, flags):
    height, width = y.shape
    codes, window = _import(cvs, layout, ym.pack(layout, y, cb, cr), width, height, flags)
    assert window == (0, 0, width - 1, height - 1)
    return ym.unpack(layout, _export(cvs, layout, codes, width, height, flags), width, height)


@pytest.mark.parametrize("layout", yc.LAYOUT_NAMES)
def test_round_trips_that_design_claims(cvs, layout):
    """samples -> import -> export on the device (DESIGN.md "4:2:0 Y'CbCr edges"): every legal grey code and flat in-gamut colours
    come back exactly in the 8-bit layouts, and in the 10-bit ones with the transfer off; with the tables, 10-bit luma comes back
    within one code and chroma exactly."""
    s = 1 << (ym.BITS[layout] - 8)
    for range_ in ym.RANGE_FLAGS:
        y, cb, cr = grey_round_trip_inputs(layout, range_)
        for transfer in ym.TRANSFER_FLAGS:
            for matrix, siting in (("601", "left"), ("709", "center"), ("2020", "topleft")):
                check_grey_round_trip(layout, range_, transfer, y, _device_round_trip(cvs, layout, y, cb, cr, ym.flags(matrix, range_, siting, transfer)))
    # the flat colours as one raster each would be 400 launches: twelve of them, in every siting
    for n, (y, cb, cr) in enumerate(flat_round_trip_inputs(layout, "studio")[:12]):
        for transfer in ym.TRANSFER_FLAGS:
            y2, cb2, cr2 = _device_round_trip(cvs, layout, y, cb, cr, ym.flags(yc.MATRIX_NAMES[n % 3], "studio", yc.SITINGS[n % 3], transfer))
            assert np.array_equal(cb2, cb) and np.array_equal(cr2, cr)
            assert np.abs(y2 - y).max() <= (0 if s == 1 or transfer == "none" else 1)
