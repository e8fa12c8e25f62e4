"""The two device entries of include/canvas_ycc422.h on the GPU, bit for bit the model (tests/ycc422_model.py): the catalogue of
tests/ycc422_cases.py -- every layout, both matrices, the smallest shapes and the widths around a wave's run, padded strides and
extra lines, frames larger than, inside and partly off the raster -- in both arithmetic flavours; one 1920x1080 and one 3840x2160
raster per layout and direction, so that both placements of the half table run; and the refusals, which launch nothing.  An
expectation covers every byte of every output: the padding beyond a row's least stride, the lines beyond the height and the
frame's pixels outside the raster keep what they held."""
import ctypes as C

import numpy as np
import pytest

from canvas_amd import _lib
from canvas_amd.device import DeviceFrame
from tests import ycc422_cases as yc
from tests import ycc422_model as ym
from tests.entry_cases import SENT16, Twin

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
        return rc, got, (None if frame.current_window.is_empty() else frame.current_window.tuple()), twin.objects
    finally:
        twin.free()


def _assert_spec(cvs, orc, spec):
    what = yc.name(spec)
    rc, got, window, objects = _run(cvs, spec)
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
    """Both entries, both matrices; the same bytes in both arithmetic flavours (the model is one)."""
    specs = yc.specs(layout)
    assert {s["direction"] for s in specs} == {"reconstruct", "subsample"} and {s["matrix"] for s in specs} == {"601", "709"}
    for spec in specs:
        _assert_spec(cvs, orc, spec)


def _big(layout, direction, width, height, matrix, seed):
    strides, lines = ym.least(layout, width, height)
    if layout == "v210":
        strides = [(strides[0] + 127) // 128 * 128]            # the stride capture cards use
    return dict(direction=direction, layout=layout, matrix=matrix, width=width, height=height, strides=strides, lines=lines,
                full=(-2, -1, width + 1, height) if direction == "subsample" else (0, 0, width - 1, height - 1), seed=seed)


@pytest.mark.parametrize("direction", ["reconstruct", "subsample"])
@pytest.mark.parametrize("layout", yc.LAYOUT_NAMES)
@pytest.mark.parametrize("width,height", [(1920, 1080), (3840, 2160)])
def test_whole_rasters_in_both_table_placements(cvs, orc, layout, direction, width, height):
    """1920x1080 takes the half table from LDS too (the switch is at one megapixel), so the gathered form runs on the catalogue's
    small rasters and the staged one here; 3840x2160 gives every workgroup more than one trip."""
    _assert_spec(cvs, orc, _big(layout, direction, width, height, "709" if width == 1920 else "601", 2300 + width))


@pytest.mark.parametrize("layout", yc.LAYOUT_NAMES)
def test_a_raster_below_the_switch_gathers_and_one_above_stages(cvs, orc, layout):
    """720x486 (gathered from L2, many workgroups per CU) and 1280x1024 (staged: just above one megapixel) give the model's bytes."""
    for width, height in ((720, 486), (1280, 1024)):
        for direction in ("reconstruct", "subsample"):
            _assert_spec(cvs, orc, _big(layout, direction, width, height, "709", 2400 + width))


# ---------------------------------------------------------------- refusals: nothing is launched, nothing is written

def _planes_dev(cvs, layout, width, height):
    strides, lines = ym.least(layout, width, height)
    ptrs = []
    for s, n in zip(strides, lines):
        ptrs.append(cvs.cvs_malloc(s * n + 64))
        a = np.full(s * n + 64, 0xA5, np.uint8)
        _lib.check(cvs.cvs_memcpy_h2d(ptrs[-1], a.ctypes.data, a.size, None), "h2d")
    return ptrs, strides, lines


def _image(ptrs, strides, lines):
    img = _lib.coded_image()
    for p, (ptr, s, n) in enumerate(zip(ptrs, strides, lines)):
        img.data[p], img.stride[p], img.line_count[p] = ptr, s, n
    return img


@pytest.mark.parametrize("layout", yc.LAYOUT_NAMES)
def test_refusals_launch_nothing(cvs, flavour, layout):
    width, height, lid = 24, 4, ym.LAYOUTS[layout]
    ptrs, strides, lines = _planes_dev(cvs, layout, width, height)
    full = (0, 0, width - 1, height - 1)
    before = np.broadcast_to(SENT16, (height, width, 4)).copy()
    frame = DeviceFrame(full, np.uint16)
    frame.upload(before)
    try:
        def planes_now():
            out = []
            for ptr, s, n in zip(ptrs, strides, lines):
                a = np.empty(s * n + 64, np.uint8)
                _lib.check(cvs.cvs_memcpy_d2h(a.ctypes.data, ptr, a.size, None), "d2h")
                out.append(a)
            return out

        def refused(img, w, h, lay, flags, word):
            for entry in ("reconstruct", "subsample"):
                frame.c.current_window = _lib.box2i.of(*full)
                cvs.cvs_clear_last_error()
                if entry == "reconstruct":
                    rc = cvs.cvs_reconstruct_422_dev(frame.ref(), C.byref(img) if img is not None else None, w, h, lay, flags, None)
                    assert frame.current_window.is_empty(), (entry, word)
                else:
                    rc = cvs.cvs_subsample_422_dev(C.byref(img) if img is not None else None, frame.ref(), w, h, lay, flags, None)
                assert rc == -1 and word in _lib.last_error(), (entry, word, rc, _lib.last_error())

        good = lambda: _image(ptrs, strides, lines)
        for w in (23, 25, 1, 0, -2):
            refused(good(), w, height, lid, 0, "width")
        for h in (0, -1):
            refused(good(), width, h, lid, 0, "height")
        for flags in (_lib.YCC_PROGRESSIVE, _lib.YCC_PROGRESSIVE | _lib.YCC_REC709, 4, -1):
            refused(good(), width, height, lid, flags, "unknown flags")
        for lay in (-1, 4, 17):
            refused(good(), width, height, lay, 0, "unknown layout")
        refused(None, width, height, lid, 0, "need an image")
        for p in range(len(ptrs)):
            img = good()
            img.data[p] = None
            refused(img, width, height, lid, 0, "missing")
            img = good()
            img.stride[p] -= ym.ALIGN[layout]
            refused(img, width, height, lid, 0, "too short")
            img = good()
            img.line_count[p] -= 1
            refused(img, width, height, lid, 0, "too short")
            if ym.ALIGN[layout] > 1:
                img = good()
                img.data[p] = ptrs[p] + 1
                refused(img, width, height, lid, 0, "misaligned")
                img = good()
                img.stride[p] += 1
                refused(img, width, height, lid, 0, "misaligned")
                if ym.ALIGN[layout] == 4:
                    img = good()
                    img.data[p] = ptrs[p] + 2
                    refused(img, width, height, lid, 0, "misaligned")
        if len(ptrs) == 3:                      # a planar layout handed one plane: too few planes
            img = _image(ptrs[:1], strides[:1], lines[:1])
            refused(img, width, height, lid, 0, "missing")
        # a current window outside the buffer (export only reads it)
        frame.c.current_window = _lib.box2i.of(0, 0, width, height - 1)
        assert cvs.cvs_subsample_422_dev(C.byref(good()), frame.ref(), width, height, lid, 0, None) == -1 and "outside" in _lib.last_error()
        _lib.check(cvs.cvs_stream_sync(None), "sync")
        assert all((a == 0xA5).all() for a in planes_now()), "a refused call wrote a plane"
        assert np.array_equal(frame.download().array, before), "a refused call wrote the frame"
        # the same operands, nothing wrong: both succeed
        frame.c.current_window = _lib.box2i.of(*full)
        assert cvs.cvs_subsample_422_dev(C.byref(good()), frame.ref(), width, height, lid, 0, None) == 0, _lib.last_error()
        assert cvs.cvs_reconstruct_422_dev(frame.ref(), C.byref(good()), width, height, lid, 0, None) == 0, _lib.last_error()
        assert frame.current_window.tuple() == full
        _lib.check(cvs.cvs_stream_sync(None), "sync")
        for a, s, n in zip(planes_now(), strides, lines):
            assert (a[s * n:] == 0xA5).all(), "bytes beyond the last line were written"
    finally:
        for p in ptrs:
            cvs.cvs_free(p)
        frame.free()


def test_a_frame_off_the_raster_gives_an_empty_window_and_black_planes(cvs, orc):
    """Reconstruct: 0, an empty window, the frame untouched.  Subsample: the planes of a frame without pixels (legal black)."""
    for layout in yc.LAYOUT_NAMES:
        for direction in ("reconstruct", "subsample"):
            spec = dict(yc.specs(layout)[0], direction=direction, width=14, height=3, full=(40, 2, 47, 6))
            spec["strides"], spec["lines"] = ym.least(layout, 14, 3)
            _assert_spec(cvs, orc, spec)
            if direction == "subsample":
                y, cb, cr = ym.unpack(layout, yc.expected(spec, orc), 14, 3)
                s = 1 << (ym.BITS[layout] - 8)
                assert (y == 16 * s).all() and (cb == 128 * s).all() and (cr == 128 * s).all()
