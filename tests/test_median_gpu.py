"""The median on the GPU, bit for bit against the numpy model of the contract (tests/median_model.py, DESIGN.md "Median") in both
arithmetic flavours, which must give equal bytes.  Every output code is a copy of an input code, so RAW BYTES are compared:
zero signs and NaN payloads are not folded.  The target is pre-filled with a sentinel so that untouched pixels are proven
untouched, and the source is checked unwritten.  Pixels are bit patterns: uint16 for half frames, uint32 for f32 frames.

Shapes: a wave makes 64 - 2 H columns of lanes; with two half pixels per lane (H = 1) that is 124 columns at both radii, with
one pixel per lane (f16 where a pitch is odd or a base unaligned, and f32; H = radius) 62 columns at radius 1 and 60 at radius 2.
Segments are at least 8 rows.  A buffer one column wider than the window forces either f16 form on any width (the pair form
needs even pitches)."""
import ctypes as C

import numpy as np
import pytest

from canvas_amd import _lib
from canvas_amd.abi import HostFrame
from canvas_amd.device import DeviceFrame
from tests import median_model as mm
from tests.test_fields_gpu import FLAVOURS, _box, _empty_box, _window

pytestmark = pytest.mark.gpu

SENTINELS = {np.uint16: np.array([0x7E17, 0x1234, 0xFBCD, 0x0001], np.uint16), np.uint32: np.array([0x7FC01234, 0x449A5000, 0xBF800001, 0x00000001], np.uint32)}
# form: (pixel type, two pixels per lane)
FORMS = {"f16-pairs": (np.uint16, True), "f16-single": (np.uint16, False), "f32": (np.uint32, False)}
SETTINGS = [(t, c) for t in (0.0, mm.THRESHOLD) for c in ("rgba", "rgb", "a", "ga")]


def made(form, radius):
    """the columns one wave makes"""
    return 124 if FORMS[form][1] else 64 - 2 * radius


def _host(bits, full, cur):
    return HostFrame(full, np.uint16 if bits.dtype == np.uint16 else np.float32, bits if bits.dtype == np.uint16 else bits.view(np.float32), _empty_box(cur))


def _bits(array, dtype):
    return array if dtype == np.uint16 else np.ascontiguousarray(array).view(np.uint32)


def run(cvs, out_full, source, p, call=None):
    """One call into a target over out_full pre-filled with the sentinel, in both flavours: (rc, bits, window) and the target
    beforehand.  source: (bits, full, current or None)."""
    bits, sfull, scur = source
    dtype = bits.dtype.type
    entry = cvs.cvs_median_f16_dev if dtype == np.uint16 else cvs.cvs_median_f32_dev
    before = np.broadcast_to(SENTINELS[dtype], _box(out_full) + (4,)).copy()
    results = []
    for _name, mode in FLAVOURS:
        out = DeviceFrame.from_host(_host(before, out_full, None))
        src = DeviceFrame.from_host(_host(bits, sfull, scur))
        prev = cvs.cvs_set_arithmetic(mode)
        try:
            rc = call(out, src) if call else entry(out.ref(), src.ref(), C.byref(p), None)
            _lib.check(cvs.cvs_stream_sync(None), "sync")
        finally:
            cvs.cvs_set_arithmetic(prev if prev >= 0 else _lib.ARITH_SEPARATE)
        results.append((rc, _bits(out.download().array, dtype), _window(out)))
        assert np.array_equal(_bits(src.download().array, dtype), bits), "the source was written"
        src.free()
        out.free()
    assert results[0][0] == results[1][0] and results[0][2] == results[1][2]
    assert np.array_equal(results[0][1], results[1][1]), "the two arithmetic flavours differ"
    return results[0], before


def check(cvs, out_full, source, radius, threshold, channels, what):
    bits, sfull, scur = source
    (rc, got, window), before = run(cvs, out_full, source, _lib.median(radius, threshold, mm.mask_of(channels)))
    what = "%s, radius %d threshold %g channels %s" % (what, radius, threshold, channels)
    assert rc == 0, "%s: %s" % (what, _lib.last_error())
    want, want_window = mm.expected(before, out_full, bits, sfull, scur, radius, threshold, channels)
    assert window == want_window, "%s: window %r, want %r" % (what, window, want_window)
    if not np.array_equal(got, want):
        bad = np.argwhere((got != want).any(axis=-1))
        y, x = bad[0]
        raise AssertionError("%s: %d pixels differ; first at buffer row %d column %d: got %s want %s" % (
            what, len(bad), y, x, [hex(v) for v in got[y, x]], [hex(v) for v in want[y, x]]))


def picture(seed, form, cw, margin=(0, 0, 0, 0), specials=True):
    """(bits, full, cw): the speck picture over cw in a buffer `margin` (left, top, right, bottom) larger, junk outside cw; one
    more junk column on the right where the form's pitch parity asks for it"""
    dtype, pairs = FORMS[form]
    rng = np.random.default_rng(seed)
    full = [cw[0] - margin[0], cw[1] - margin[1], cw[2] + margin[2], cw[3] + margin[3]]
    if form != "f32" and ((full[2] - full[0] + 1) & 1) == (1 if pairs else 0):
        full[2] += 1
    full = tuple(full)
    bits = rng.integers(0, 0x10000 if dtype == np.uint16 else 2 ** 32, _box(full) + (4,)).astype(dtype)
    mm.crop(bits, full, cw)[...] = mm.speck_picture(rng, cw[2] - cw[0] + 1, cw[3] - cw[1] + 1, dtype, specials)
    return bits, full, cw


@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("form", sorted(FORMS))
def test_whole_frames(cvs, form, radius):
    """widths one fewer than, exactly, one more than and twice plus one the columns a wave makes, and 1, 2, 3 columns; heights
    1, 2, 4 and one fewer than, exactly and one more than a segment"""
    m = made(form, radius)
    n = 0
    for width in (1, 2, 3, 33, m - 1, m, m + 1, 2 * m + 1):
        for height in (1, 2, 4, 7, 8, 9, 17):
            x0, y0 = [(0, 0), (2, -1), (-4, 3)][n % 3]
            cw = (x0, y0, x0 + width - 1, y0 + height - 1)
            src = picture(width * 131 + height * 7, form, cw)
            threshold, channels = SETTINGS[n % len(SETTINGS)]
            check(cvs, src[1], src, radius, threshold, channels, "%s %dx%d at (%d, %d)" % (form, width, height, x0, y0))
            n += 1


@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("form", sorted(FORMS))
def test_every_setting(cvs, form, radius):
    cw = (0, 0, 129, 20)
    src = picture(41, form, cw)
    for threshold, channels in SETTINGS + [(1e-30, "rgba"), (3e38, "rgba"), (0.5, "r"), (0.0, "b")]:
        check(cvs, src[1], src, radius, threshold, channels, "%s 130x21" % form)


@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("form", sorted(FORMS))
def test_windows_inside_the_buffer_and_targets_elsewhere(cvs, form, radius):
    """source.current_window strictly inside its buffer on all four sides: the junk around it is never read into a result
    (clamping is at the source's window, not at a buffer's edge); target.full_window larger than, smaller than and offset from it"""
    m = made(form, radius)
    for n, width in enumerate((m, m + 1, 37)):
        cw = (3, 2, 3 + width - 1, 2 + 12)
        src = picture(500 + width, form, cw, margin=(3, 2, 4, 3))
        for k, out_full in enumerate([src[1], (cw[0] - 5, cw[1] - 3, cw[2] + 6, cw[3] + 4), (cw[0] + 2, cw[1] + 1, cw[2] - 3, cw[3] - 2), (cw[0] + 1, cw[1] + 3, cw[2] - 1, cw[3] - 1),
                                      (cw[0] - 9, cw[1] - 7, cw[0] + 20, cw[1] + 5), (cw[0] + 30, cw[1] + 6, cw[2] + 30, cw[3] + 9), (cw[0] + 7, cw[1] + 5, cw[0] + 7, cw[1] + 5)]):
            threshold, channels = SETTINGS[(n + k) % len(SETTINGS)]
            check(cvs, out_full, src, radius, threshold, channels, "%s source %r in %r, target %r" % (form, cw, src[1], out_full))
        # the same picture in other junk gives the same bytes
        other = picture(900 + width, form, cw, margin=(3, 2, 4, 3))
        mm.crop(other[0], other[1], cw)[...] = mm.crop(src[0], src[1], cw)
        p = _lib.median(radius, mm.THRESHOLD)
        assert np.array_equal(run(cvs, cw, src, p)[0][1], run(cvs, cw, other, p)[0][1])


@pytest.mark.parametrize("radius", [1, 2])
def test_an_odd_first_column_an_odd_pitch_and_an_unaligned_base(cvs, radius):
    # an odd first column in buffers of even pitch: the pair form, its first pair cut by the window
    for cw in ((1, 0, 130, 9), (1, 0, 129, 9), (3, 1, 3, 9)):
        src = picture(61, "f16-pairs", cw, margin=(cw[0], 0, 0, 0))
        check(cvs, src[1], src, radius, mm.THRESHOLD, "rgba", "odd first column %r in %r" % (cw, src[1]))
    # pitches of different parity: one pixel per lane
    src = picture(62, "f16-pairs", (0, 0, 129, 9))
    check(cvs, (0, 0, 130, 9), src, radius, mm.THRESHOLD, "rgba", "an even and an odd pitch")
    # a source whose base is 8 bytes off a 16-byte boundary: a frame struct one pixel into a buffer
    w, h = 130, 9
    bits = picture(63, "f16-pairs", (0, 0, w - 1, h - 1))[0]
    flat = np.concatenate([np.full((1, 1, 4), 0x7C01, np.uint16), bits.reshape(1, w * h, 4)], axis=1)
    full = (0, 0, w - 1, h - 1)

    def call(out, buf):
        inner = _lib.rgba_frame_f16(buf.ptr + 8, _lib.box2i.of(*full), _lib.box2i.of(*full))
        return cvs.cvs_median_f16_dev(out.ref(), C.byref(inner), C.byref(_lib.median(radius, mm.THRESHOLD)), None)
    (rc, got, window), before = run(cvs, full, (flat, (0, 0, w * h, 0), (0, 0, w * h, 0)), None, call)
    assert rc == 0 and window == full
    assert np.array_equal(got, mm.expected(before, full, bits, full, full, radius, mm.THRESHOLD)[0])


@pytest.mark.parametrize("form", sorted(FORMS))
def test_flat_pictures_and_pictures_of_nans(cvs, form):
    dtype = FORMS[form][0]
    cw = (0, 0, 127 + (form == "f16-single"), 10)
    nan = [0x7E00, 0xFE00, 0x7C01, 0x7FFF] if dtype == np.uint16 else [0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF]
    flat = [0x3800, 0x8000, 0x0001, 0x7BFF] if dtype == np.uint16 else [0x3F000000, 0x80000000, 0x00000001, 0x7F7FFFFF]
    for radius in (1, 2):
        for codes in (nan, flat):
            bits = np.broadcast_to(np.array(codes, dtype), _box(cw) + (4,)).copy()
            for threshold in (0.0, mm.THRESHOLD):
                (rc, got, window), _ = run(cvs, cw, (bits, cw, cw), _lib.median(radius, threshold))
                assert rc == 0 and window == cw and np.array_equal(got, bits), (radius, codes, threshold)
        # NaNs of many payloads and both signs: the order on bit patterns decides
        rng = np.random.default_rng(7)
        bits = (rng.integers(1, 0x400, _box(cw) + (4,)) | 0x7C00 | (rng.integers(0, 2, _box(cw) + (4,)) << 15)).astype(np.uint16)
        if dtype == np.uint32:
            bits = (bits.astype(np.uint32) & 0x8000) << 16 | 0x7F800000 | rng.integers(1, 0x800000, bits.shape).astype(np.uint32)
        check(cvs, cw, (bits, cw, cw), radius, mm.THRESHOLD, "rgba", "%s NaNs" % form)


@pytest.mark.parametrize("form", sorted(FORMS))
def test_empty_windows_launch_nothing_and_write_nothing(cvs, form):
    cw = (0, 0, 33, 8)
    src = picture(71, form, cw)
    for source, out_full in (((src[0], src[1], None), src[1]), (src, (cw[2] + 1, 0, cw[2] + 8, 8)), (src, (0, cw[3] + 1, 33, cw[3] + 3))):
        (rc, got, window), before = run(cvs, out_full, source, _lib.median(2, mm.THRESHOLD))
        assert rc == 0 and window is None and np.array_equal(got, before)
