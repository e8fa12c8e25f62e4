"""The primary colour corrector on the GPU, bit for bit against the numpy model (tests/primary_model.py; DESIGN.md "Primary colour
correction"), every entry case under both cvs_set_arithmetic settings with identical bytes required.  Every operation of the
contract is a correctly rounded IEEE f32 operation or an exact conversion, so there is no tolerance anywhere: one differing code
fails.  What is folded before comparing is what tests/test_lut3d_gpu.py folds (tests/util.py canon_f16 / canon_f32): the sign of
zero and the payload of a NaN, which x86 and gfx950 choose differently.  Target pixels outside the window must keep a sentinel,
inputs and the tables must come back unwritten.  Pictures are tests/primary_model.py's, a few thousand pixels each; the one large
case is the column of test_persistent_workgroups."""
import ctypes as C

import numpy as np
import pytest

from canvas_amd import _lib
from canvas_amd.abi import HostFrame
from canvas_amd.device import DeviceFrame
from tests import primary_model as pm
from tests.test_unsharp_gpu import _in_flavour
from tests.util import canon_f16, canon_f32

pytestmark = pytest.mark.gpu

FLAVOURS = [("gcc", _lib.ARITH_SEPARATE), ("fma", _lib.ARITH_CONTRACTED)]
SENTINEL16 = np.array([0x7E17, 0x1234, 0xFBCD, 0x0001], np.uint16)
SENTINEL32 = np.array([1234.5, -7.25, 3.0e-5, 0.4375], np.float32)
SIZES = [2, 3, 17, 1024, 1025, 4097]
# (pre, matrix, post) present: every one of the seven
COMBOS = [(True, False, False), (False, True, False), (False, False, True), (True, True, False), (True, False, True), (False, True, True), (True, True, True)]
MATRIX = [0.75, 0.5, -0.25, 0.0625, 0.0, -1.0, 2.0, 0.0, 0.3, 0.3, 0.3, -0.2]        # zeros and negative entries
ROWS = [1, 2, 7, 8, 9, 17]
# the columns a wave makes: 64 where a lane holds one pixel (f32 frames, half frames that are not pair-aligned), 128 where it holds two
WIDTHS_ONE = [1, 2, 3, 63, 64, 65, 129]
WIDTHS_TWO = [1, 2, 3, 127, 128, 129, 257]
OVERFLOW_DOMAIN = ((-4.0, -4.0, -4.0), (4.0, 4.0, 4.0))          # the picture of the overflowing matrix: two nodes on it


def _box(full):
    return (full[3] - full[1] + 1, full[2] - full[0] + 1)


class Tables:
    """One device copy per curve set, made once and checked unwritten at the end of the module."""

    def __init__(self, cvs):
        self.cvs, self.held = cvs, {}

    def __call__(self, size, domain, seed=0):
        key = (size, domain, seed)
        if key not in self.held:
            cv = pm.distinct(size, domain, seed)
            flat = cv.planar()
            assert flat.nbytes == self.cvs.cvs_curves_bytes(size)
            dev = self.cvs.cvs_malloc(flat.nbytes)
            assert dev and dev % 16 == 0, _lib.last_error()
            _lib.check(self.cvs.cvs_memcpy_h2d(dev, flat.ctypes.data, flat.nbytes, None), "h2d")
            self.held[key] = (cv, dev, flat)
        return self.held[key][:2]

    def close(self):
        for cv, dev, flat in self.held.values():
            back = np.empty_like(flat)
            _lib.check(self.cvs.cvs_memcpy_d2h(back.ctypes.data, dev, flat.nbytes, None), "d2h")
            self.cvs.cvs_free(dev)
            assert back.tobytes() == flat.tobytes(), "a table was written"


@pytest.fixture(scope="module")
def tables(cvs):
    held = Tables(cvs)
    yield held
    held.close()


class Grade:
    """One configuration: the model's operands, the entry's struct and the two device pointers."""

    def __init__(self, tables, pre=None, matrix=None, post=None):
        self.pre, self.pre_dev = tables(*pre) if pre else (None, None)
        self.post, self.post_dev = tables(*post) if post else (None, None)
        self.matrix = matrix
        self.p = _lib.primary((self.pre.size,) + self.pre.domain if self.pre else None, matrix, (self.post.size,) + self.post.domain if self.post else None)
        self.name = "pre %s matrix %s post %s" % (self.pre.size if self.pre else "-", "yes" if matrix is not None else "-", self.post.size if self.post else "-")

    def first(self):
        """(size, domain) of the first curves the pixels meet, for the picture; a matrix alone: 17 nodes on SKEWED"""
        cv = self.pre or self.post
        return (cv.size, cv.domain) if cv else (17, pm.SKEWED)

    def model(self):
        return dict(pre=self.pre, matrix=self.matrix, post=self.post)


def _entry(cvs, half):
    return cvs.cvs_primary_f16_dev if half else cvs.cvs_primary_f32_dev


def _call(cvs, half, target, source, g, stream=None):
    return _entry(cvs, half)(target.ref(), source.ref(), C.byref(g.p), g.pre_dev, g.post_dev, stream)


def _same(got, want, half, what):
    g, w = (canon_f16(got), canon_f16(want)) if half else (canon_f32(got), canon_f32(want))
    g, w = g.reshape(got.shape), w.reshape(want.shape)
    if not np.array_equal(g, w):
        raw = (lambda a: a) if half else (lambda a: np.ascontiguousarray(a).view(np.uint32))
        bad = np.argwhere((g != w).any(axis=-1))
        y, x = bad[0]
        raise AssertionError("%s: %d pixels differ; first at buffer row %d column %d: got %s want %s" % (
            what, len(bad), y, x, [hex(int(v)) for v in raw(got)[y, x]], [hex(int(v)) for v in raw(want)[y, x]]))


def _once(cvs, half, tfull, sfull, scur, pixels, g, offset=0):
    """One out-of-place call on fresh device frames -> (target buffer, window or None, what the target held before).  offset:
    both frames start that many bytes into their allocations (an unaligned base)."""
    dtype, sentinel = (np.uint16, SENTINEL16) if half else (np.float32, SENTINEL32)
    before = np.broadcast_to(sentinel, _box(tfull) + (4,)).copy()
    blocks = []
    try:
        if offset:
            def place(host):
                block = cvs.cvs_malloc(host.array.nbytes + offset)
                assert block
                blocks.append(block)
                frame = DeviceFrame(host.full_window, host.dtype, host.current_window, ptr=block + offset)
                frame.upload(host.array)
                return frame
        else:
            place = DeviceFrame.from_host
        source = place(HostFrame(sfull, dtype, pixels, (0, 0, -1, -1) if scur is None else scur))
        target = place(HostFrame(tfull, dtype, before))
        rc = _call(cvs, half, target, source, g)
        _lib.check(cvs.cvs_stream_sync(None), "sync")
        assert rc == 0, _lib.last_error()
        got = target.download().array
        window = None if target.current_window.is_empty() else target.current_window.tuple()
        assert source.download().array.tobytes() == np.ascontiguousarray(pixels).tobytes(), "the input was written"
        source.free(); target.free()
    finally:
        for block in blocks:
            cvs.cvs_free(block)
    return got, window, before


def _in_place(cvs, half, full, cur, pixels, g):
    frame = DeviceFrame.from_host(HostFrame(full, np.uint16 if half else np.float32, pixels, cur))
    try:
        assert _call(cvs, half, frame, frame, g) == 0, _lib.last_error()
        _lib.check(cvs.cvs_stream_sync(None), "sync")
        return frame.download().array, (None if frame.current_window.is_empty() else frame.current_window.tuple())
    finally:
        frame.free()


def _check(cvs, g, half, tfull, sfull, scur, pixels, what, in_place=False, offset=0):
    """The call under both arithmetic settings: the model's codes, the model's window, and the same bytes from both; in place:
    also the bytes of the out-of-place call inside the window."""
    results = []
    want, win = pm.expected(np.broadcast_to(SENTINEL16 if half else SENTINEL32, _box(tfull) + (4,)).copy(), tfull, pixels, sfull, scur, **g.model())
    for flavour, mode in FLAVOURS:
        with _in_flavour(cvs, flavour, mode):
            got, window, _ = _once(cvs, half, tfull, sfull, scur, pixels, g, offset)
            again = _in_place(cvs, half, sfull, scur, pixels, g) if in_place else None
        label = "%s, %s, %s %s" % (what, g.name, "f16" if half else "f32", flavour)
        assert window == win, "%s: window %r, want %r" % (label, window, win)
        _same(got, want, half, label)
        if again:
            assert again[1] == scur, label
            both = pm.intersect(scur, tfull)
            assert pm.crop(again[0], sfull, both).tobytes() == pm.crop(got, tfull, both).tobytes(), label + ": in place differs from out of place"
            outside = np.ones(_box(sfull), bool)
            pm.crop(outside, sfull, scur)[...] = False
            assert np.array_equal(again[0][outside].view(np.uint8), np.ascontiguousarray(pixels)[outside].view(np.uint8)), label + ": in place wrote outside the window"
        results.append(got)
    assert results[0].tobytes() == results[1].tobytes(), what + ": the two arithmetic settings give different bytes"
    return results[0]


def _picture(seed, full, half, g):
    h, w = _box(full)
    size, domain = g.first()
    return pm.picture(np.random.default_rng(seed), w, h, half, size, domain)


def _grade(tables, combo, size, other):
    pre, mat, post = combo
    return Grade(tables, (size, pm.SKEWED, 1) if pre else None, MATRIX if mat else None, (other, pm.WIDE, 2) if post else None)


@pytest.mark.parametrize("size", SIZES)
def test_stage_combinations(cvs, tables, size):
    """Every one of the seven combinations with `size` nodes in the first curves and another size in the second, domains that
    differ per channel and between the stages (a negative start, a width of 2^-10), on the 131 x 9 picture, in and out of place."""
    other = SIZES[(SIZES.index(size) + 2) % len(SIZES)]
    full = (0, 0, 130, 8)
    for n, combo in enumerate(COMBOS):
        g = _grade(tables, combo, size, other) if combo != (False, False, True) else Grade(tables, post=(size, pm.SKEWED, 1))
        for half in (True, False):
            _check(cvs, g, half, full, full, full, _picture(100 * size + n, full, half, g), "combination", in_place=True)


def _geometries(width, rows):
    """(name, source full, source current, target full, pairs possible) for a window `width` wide: on an even and on an odd first
    column of an even-pitched buffer (the pair form, cut on the left, on the right, on both or on neither), as the whole of a
    buffer with an odd origin, in a buffer of odd pitch (the one-pixel form), with a target that is smaller than the source
    window, and one with an odd base column."""
    y1 = rows - 1
    out = []
    for x0 in (0, 1, 2):
        x1 = x0 + width - 1
        full = (0, 0, (x1 + 2) // 2 * 2 - 1, y1)                          # an even pitch from column 0
        out.append(("first column %d" % x0, full, (x0, 0, x1, y1), full, True))
    whole = (-3, -1, width - 4, y1 - 1)
    out.append(("whole buffer", whole, whole, whole, width % 2 == 0))
    odd = (0, 0, (width + 1) // 2 * 2, y1)                                # an odd pitch: no row but the first starts a pair
    out.append(("odd pitch", odd, (1, 0, width, y1), odd, False))
    if width > 4:
        full = (0, 0, width - 1, y1)
        out.append(("smaller target", full, full, (2, 0, width - 3, max(y1 - 1, 0)), width % 2 == 0))
        out.append(("odd target base", full, full, (-1, 0, width, y1), False))
        out.append(("larger target", full, full, (-2, -1, width + 1, y1 + 2), width % 2 == 0))
    return out


@pytest.mark.parametrize("form", ["f32", "f16 one pixel", "f16 two pixels"])
def test_widths_rows_and_placements(cvs, tables, form):
    """Each lane form at one fewer than, at, one past and twice plus one the columns a wave makes, and at 1, 2 and 3 columns; 1, 2,
    7, 8, 9 and 17 rows; every placement of _geometries that gives the form."""
    half, pairs = form != "f32", form == "f16 two pixels"
    full_grade = Grade(tables, (1025, pm.SKEWED, 1), MATRIX, (17, pm.WIDE, 2))
    small = Grade(tables, (3, pm.WIDE, 1), None, None)
    for wi, width in enumerate(WIDTHS_TWO if pairs else WIDTHS_ONE):
        for rows in (ROWS[wi % 6], ROWS[(wi + 3) % 6]):
            for gi, (gname, sfull, scur, tfull, can_pair) in enumerate(_geometries(width, rows)):
                if half and can_pair != pairs:
                    continue
                g = full_grade if (wi + gi) % 2 == 0 else small
                pixels = _picture(1000 * width + rows, sfull, half, g)
                _check(cvs, g, half, tfull, sfull, scur, pixels, "%s %dx%d %s" % (form, width, rows, gname), in_place=(tfull == sfull and gi % 2 == 0))


@pytest.mark.parametrize("half", [True, False], ids=["f16", "f32"])
def test_a_window_inside_junk_and_an_unaligned_base(cvs, tables, half):
    """A source window strictly inside its buffer with junk (the picture's specials among it) around; targets larger than,
    smaller than and offset from it; both frames 8 bytes into their allocations."""
    g = Grade(tables, (17, pm.SKEWED, 1), MATRIX, (1024, pm.WIDE, 2))
    sfull, scur = (-4, -3, 140, 12), (1, 0, 131, 8)
    pixels = _picture(31, sfull, half, g)
    for tfull in ((-9, -5, 150, 15), (10, 2, 99, 6), (64, 5, 200, 20), (-30, -3, 64, 3)):
        for offset in (0, 8):
            _check(cvs, g, half, tfull, sfull, scur, pixels, "window inside junk, target %r, base + %d" % (tfull, offset), offset=offset)
    _check(cvs, g, half, sfull, sfull, scur, pixels, "window inside junk", in_place=True)


def test_a_picture_of_nans(cvs, tables):
    full = (0, 0, 130, 2)
    for combo in ((True, True, True), (False, True, False), (False, True, True)):
        g = _grade(tables, combo, 17, 3)
        codes = np.full(_box(full) + (4,), 0x7E00, np.uint16)
        codes[1] = 0xFDFF                                               # signalling, negative
        got = _check(cvs, g, True, full, full, full, codes, "all NaN", in_place=True)
        assert np.array_equal(got[..., 3], codes[..., 3])
        s = np.full(_box(full) + (4,), np.nan, np.float32)
        _check(cvs, g, False, full, full, full, s, "all NaN", in_place=True)


def test_a_matrix_that_overflows_into_the_post_curves(cvs, tables):
    """The matrix sends values to +Inf, -Inf and (Inf - Inf) NaN; the post curves clamp them to their ends: the model says so, and
    every colour that comes out is finite."""
    big = [3.0e38, 3.0e38, 0.0, 0.0, -3.0e38, 0.0, -3.0e38, 0.0, 3.0e38, -3.0e38, 0.0, 0.0]
    full = (0, 0, 130, 8)
    g = Grade(tables, None, big, (17, pm.WIDE, 2))
    for half in (True, False):
        pixels = _picture(77, full, half, Grade(tables, (2, OVERFLOW_DOMAIN, 5)))
        s = pm.widen(pixels) if half else pixels
        into = pm.matrix_stage(big, s[..., :3])
        assert np.isposinf(into).any() and np.isneginf(into).any() and np.isnan(into).any()
        got = _check(cvs, g, half, full, full, full, pixels, "overflowing matrix", in_place=True)
        colours = (pm.widen(got) if half else got)[..., :3]
        assert np.isfinite(colours).all()
        ends = np.isinf(into) | np.isnan(into)
        want_ends = np.where(np.isposinf(into), g.post.table[-1], g.post.table[0])
        if not half:
            assert np.array_equal(colours[ends], want_ends[ends])


def test_persistent_workgroups(cvs, tables):
    """The launch arithmetic (kernels/primary_ops.hip launch, stream_common.hpp shape): one-wave blocks of 64 lanes x seg rows,
    seg at most 64, walked by 16 waves a CU.  A column of 64 * 16 * CUs + 321 rows makes more blocks than there are waves, so the
    persistent workgroups take a second block; the 131 x 9 picture makes fewer blocks (6) than one workgroup has waves."""
    cus = cvs.cvs_compute_units()
    assert cus > 0
    rows = 64 * 16 * cus + 321
    assert -(-rows // 64) > 16 * cus
    full = (5, -7, 5, rows - 8)
    for g in (Grade(tables, (4097, pm.SKEWED, 1), MATRIX, (4097, pm.WIDE, 2)), Grade(tables, (17, pm.WIDE, 1))):     # one workgroup a CU, and two
        for half in (True, False):
            _check(cvs, g, half, full, full, full, _picture(5, full, half, g), "a column of %d rows" % rows)
    few = (0, 0, 130, 8)
    g = Grade(tables, (4097, pm.SKEWED, 1), MATRIX, (4097, pm.WIDE, 2))
    _check(cvs, g, True, few, few, few, _picture(6, few, True, g), "fewer blocks than waves")


def test_empty_windows_are_a_success(cvs, tables):
    g = Grade(tables, (3, pm.WIDE, 1), MATRIX, None)
    full = (0, 0, 9, 2)
    for half in (True, False):
        pixels = np.zeros(_box(full) + (4,), np.uint16 if half else np.float32)
        for scur, tfull in ((None, full), (full, (20, 0, 29, 2)), ((3, 0, 2, 2), full)):
            got, window, before = _once(cvs, half, tfull, full, scur, pixels, g)
            assert window is None and got.tobytes() == before.tobytes()


@pytest.mark.parametrize("size", [2, 3, 5, 17, 1025, 4097])
def test_identity_curves_return_the_codes(cvs, size):
    """Straight from the device, without the model: identity curves on [0, 1] with K - 1 a power of two give back every half code
    in [0, 1] and the f32 values of them, before and after an identity matrix."""
    cv = pm.identity(size)
    flat = cv.planar()
    dev = cvs.cvs_malloc(flat.nbytes)
    assert dev
    try:
        _lib.check(cvs.cvs_memcpy_h2d(dev, flat.ctypes.data, flat.nbytes, None), "h2d")
        codes = np.arange(0x3C01, dtype=np.uint16)
        codes = np.concatenate([codes, codes[:4 * 129 * 30 - codes.size]]).reshape(30, 129, 4)
        full = (0, 0, 128, 29)
        p = _lib.primary(size, [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], size)
        for half, pixels in ((True, codes), (False, pm.widen(codes))):
            source = DeviceFrame.from_host(HostFrame(full, pixels.dtype, pixels, full))
            target = DeviceFrame.from_host(HostFrame(full, pixels.dtype, np.zeros_like(pixels)))
            try:
                assert _entry(cvs, half)(target.ref(), source.ref(), C.byref(p), dev, dev, None) == 0, _lib.last_error()
                _lib.check(cvs.cvs_stream_sync(None), "sync")
                assert target.current_window.tuple() == full and target.download().array.tobytes() == pixels.tobytes()
            finally:
                source.free(); target.free()
    finally:
        cvs.cvs_free(dev)


def test_entries_refuse_on_the_device(cvs, tables):
    """With a device present the refusals are the contract's own (not the missing device's), and nothing is written."""
    full = (0, 0, 15, 2)
    _, dev = tables(2, pm.UNIT)
    nan = float("nan")
    for half in (True, False):
        dtype, sentinel = (np.uint16, SENTINEL16) if half else (np.float32, SENTINEL32)
        before = np.broadcast_to(sentinel, _box(full) + (4,)).copy()
        source = DeviceFrame.from_host(HostFrame(full, dtype, before, full))
        target = DeviceFrame.from_host(HostFrame(full, dtype, before))
        try:
            for p, pre, post, word in ((_lib.primary(), None, None, "no stage"), (_lib.primary(2, flags=2), dev, None, "flags"), (_lib.primary(4098), dev, None, "outside 2..4097"),
                                       (_lib.primary((2, (0, 0, 0), (1, 0, 1))), dev, None, "ascending"), (_lib.primary(2), dev + 4, None, "16-byte"), (_lib.primary(2), None, None, "need"),
                                       (_lib.primary(2), dev, dev, "absent"), (_lib.primary(2, [nan] * 12), dev, None, "not finite")):
                cvs.cvs_clear_last_error()
                target.c.current_window = target.c.full_window
                assert _entry(cvs, half)(target.ref(), source.ref(), C.byref(p), pre, post, None) == -1, word
                assert word in _lib.last_error() and target.current_window.is_empty(), (word, _lib.last_error())
            _lib.check(cvs.cvs_stream_sync(None), "sync")
            assert target.download().array.tobytes() == before.tobytes()
        finally:
            source.free(); target.free()
