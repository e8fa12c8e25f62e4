"""The 3D LUT on the GPU, bit for bit against the numpy model (tests/lut3d_model.py; DESIGN.md "3D LUT"), every entry case under
both cvs_set_arithmetic settings with identical codes required.  Every operation of the contract is a correctly rounded IEEE f32
operation or an exact conversion, so there is no tolerance anywhere: one differing code fails.  What is folded before comparing
(tests/util.py canon_f16 / canon_f32) is the sign of zero and the payload of a NaN, which x86 and gfx950 choose differently.
Target pixels outside the window must keep a sentinel, inputs and the lattice must come back unwritten.  Windows are at most
129 x 3 pixels."""
import ctypes as C

import numpy as np
import pytest

import oracle
from canvas_amd import _lib
from canvas_amd.abi import HostFrame
from canvas_amd.device import DeviceFrame
from tests import lut3d_model as lm
from tests.entry_cases import all_codes
from tests.models import f2h_rz_model, over_model
from tests.test_fields_gpu import SPECIALS, Tape, _pull
from tests.test_lut3d_cpu import _tie_frames
from tests.test_unsharp_gpu import _in_flavour, _pull32
from tests.util import canon_f16, canon_f32

pytestmark = pytest.mark.gpu

FLAVOURS = [("gcc", _lib.ARITH_SEPARATE), ("fma", _lib.ARITH_CONTRACTED)]
SENTINEL16 = np.array([0x7E17, 0x1234, 0xFBCD, 0x0001], np.uint16)
SENTINEL32 = np.array([1234.5, -7.25, 3.0e-5, 0.4375], np.float32)
SIZES = [2, 3, 4, 10, 17, 33, 65]
WIDTHS = [1, 2, 63, 64, 65, 129]
SKEWED = ((-0.25, 0.0, 0.125), (1.5, 2.0, 0.875))          # a domain that is not [0, 1] and differs per channel
DOMAINS = {2: lm.UNIT, 3: SKEWED, 4: SKEWED, 10: lm.UNIT, 17: SKEWED, 33: lm.UNIT, 65: SKEWED}
RASTER = (0, -1, 128, 1)                                     # the tape's pictures: 129 x 3


def _box(full):
    return (full[3] - full[1] + 1, full[2] - full[0] + 1)


class Lattices:
    """One device copy per size, made once and checked unwritten at the end of the module."""

    def __init__(self, cvs):
        self.cvs, self.held = cvs, {}

    def __call__(self, size):
        if size not in self.held:
            lat = lm.distinct(size, size)
            flat = lm.packed(lat)
            dev = self.cvs.cvs_malloc(flat.nbytes)
            assert dev and dev % 16 == 0, _lib.last_error()
            _lib.check(self.cvs.cvs_memcpy_h2d(dev, flat.ctypes.data, flat.nbytes, None), "h2d")
            self.held[size] = (lat, dev, flat)
        return self.held[size][:2]

    def close(self):
        for lat, dev, flat in self.held.values():
            back = np.empty_like(flat)
            _lib.check(self.cvs.cvs_memcpy_d2h(back.ctypes.data, dev, flat.nbytes, None), "d2h")
            self.cvs.cvs_free(dev)
            assert back.tobytes() == flat.tobytes(), "the lattice was written"


@pytest.fixture(scope="module")
def lattices(cvs):
    held = Lattices(cvs)
    yield held
    held.close()


def _pixels32(rng, full, domain):
    """f32 RGBA over `full`: colours spread over the domain and a quarter beyond it on either side, then a scatter of what the
    contract singles out: the domain's corners, lattice planes, greys, +-Inf, NaN, huge and tiny magnitudes, both zeros."""
    h, w = _box(full)
    lo, hi = np.array(domain[0], np.float32), np.array(domain[1], np.float32)
    s = np.empty((h, w, 4), np.float32)
    s[..., :3] = lo + (hi - lo) * rng.uniform(-0.25, 1.25, (h, w, 3)).astype(np.float32)
    s[..., 3] = rng.uniform(0, 1, (h, w)).astype(np.float32)
    grey = rng.uniform(size=(h, w)) < 0.1
    s[grey, :3] = s[grey, :1]
    pool = [np.append(lo, 1.0), np.append(hi, 0.5), np.append((lo + hi) / 2, 0.25), np.array([np.inf, 0.5, 0.5, 1.0]), np.array([0.5, -np.inf, 0.5, 0.5]),
            np.array([0.5, 0.5, np.nan, 0.75]), np.array([0.25, 0.5, 0.75, np.nan]), np.array([0.25, 0.5, 0.75, np.inf]), np.array([0.0, -0.0, 0.0, -0.0]),
            np.array([3e38, -3e38, 1e-42, 1.0]), np.array([1e-30, 1.0, -1e-30, 0.0])]
    hit = rng.uniform(size=(h, w)) < 0.1
    s[hit] = np.stack(pool).astype(np.float32)[rng.integers(0, len(pool), int(hit.sum()))]
    return s


def _pixels16(rng, full, domain):
    """The same as half codes, with the special halfs of test_fields_gpu.py (signalling NaNs, subnormals, the largest finite
    half, both zeros) scattered over all four channels."""
    codes = f2h_rz_model(_pixels32(rng, full, domain))
    scatter = rng.uniform(size=codes.shape) < 0.05
    codes[scatter] = SPECIALS[rng.integers(0, len(SPECIALS), int(scatter.sum()))]
    return codes


def _entry(cvs, half):
    return cvs.cvs_lut3d_f16_dev if half else cvs.cvs_lut3d_f32_dev


def _same(got, want, half, what):
    g, w = (canon_f16(got), canon_f16(want)) if half else (canon_f32(got), canon_f32(want))
    g, w = g.reshape(got.shape), w.reshape(want.shape)
    if not np.array_equal(g, w):
        raw = (lambda a: a) if half else (lambda a: np.ascontiguousarray(a).view(np.uint32))
        bad = np.argwhere((g != w).any(axis=-1))
        y, x = bad[0]
        raise AssertionError("%s: %d pixels differ; first at buffer row %d column %d: got %s want %s" % (
            what, len(bad), y, x, [hex(int(v)) for v in raw(got)[y, x]], [hex(int(v)) for v in raw(want)[y, x]]))


def _once(cvs, half, tfull, sfull, scur, pixels, dev, size, domain):
    """One out-of-place call on fresh device frames -> (target buffer, window or None, what the target held before)."""
    dtype, sentinel = (np.uint16, SENTINEL16) if half else (np.float32, SENTINEL32)
    before = np.broadcast_to(sentinel, _box(tfull) + (4,)).copy()
    source = DeviceFrame.from_host(HostFrame(sfull, dtype, pixels, (0, 0, -1, -1) if scur is None else scur))
    target = DeviceFrame.from_host(HostFrame(tfull, dtype, before))
    try:
        rc = _entry(cvs, half)(target.ref(), source.ref(), dev, C.byref(_lib.lut3d(size, *domain)), None)
        _lib.check(cvs.cvs_stream_sync(None), "sync")
        assert rc == 0, _lib.last_error()
        got = target.download().array
        window = None if target.current_window.is_empty() else target.current_window.tuple()
        assert source.download().array.tobytes() == np.ascontiguousarray(pixels).tobytes(), "the input was written"
    finally:
        source.free(); target.free()
    return got, window, before


def _in_place(cvs, half, full, cur, pixels, dev, size, domain):
    frame = DeviceFrame.from_host(HostFrame(full, np.uint16 if half else np.float32, pixels, cur))
    try:
        assert _entry(cvs, half)(frame.ref(), frame.ref(), dev, C.byref(_lib.lut3d(size, *domain)), None) == 0, _lib.last_error()
        _lib.check(cvs.cvs_stream_sync(None), "sync")
        return frame.download().array, (None if frame.current_window.is_empty() else frame.current_window.tuple())
    finally:
        frame.free()


def _check(cvs, lattices, half, tfull, sfull, scur, pixels, size, domain, what, in_place=False):
    """The call under both arithmetic settings: the model's codes, the model's window, and the same codes from both."""
    lat, dev = lattices(size)
    results = []
    for flavour, mode in FLAVOURS:
        with _in_flavour(cvs, flavour, mode):
            if in_place:
                got, window = _in_place(cvs, half, sfull, scur, pixels, dev, size, domain)
                before, tfull = pixels, sfull
            else:
                got, window, before = _once(cvs, half, tfull, sfull, scur, pixels, dev, size, domain)
        want, win = lm.expected(before, tfull, pixels, sfull, scur, lat, domain)
        label = "%s N=%d %s %s%s" % (what, size, "f16" if half else "f32", flavour, " in place" if in_place else "")
        assert window == win, "%s: window %r, want %r" % (label, window, win)
        _same(got, want, half, label)
        results.append(got)
    assert results[0].tobytes() == results[1].tobytes(), what + ": the two arithmetic settings give different codes"
    return results[0]


def _geometries(width, rows):
    """(name, source full, source current, target full) for a window `width` wide: on an even and on an odd first column of an
    even-pitched buffer (the pair path, cut on the left, on the right, on both or on neither), as the whole of a buffer (an odd
    width: the one-pixel path), with a target that is smaller than the source window, and one with an odd base column."""
    y1 = rows - 1
    out = []
    for x0 in (0, 1, 2):
        x1 = x0 + width - 1
        full = (0, 0, (x1 + 2) // 2 * 2 - 1, y1)                          # an even pitch from column 0
        out.append(("first column %d" % x0, full, (x0, 0, x1, y1), full))
    whole = (-3, -1, width - 4, y1 - 1)
    out.append(("whole buffer", whole, whole, whole))
    if width > 4:
        full = (0, 0, width - 1, y1)
        out.append(("smaller target", full, full, (2, 0, width - 3, max(y1 - 1, 0))))
        out.append(("odd target base", full, full, (-1, 0, width, y1)))
    return out


@pytest.mark.parametrize("size", SIZES)
def test_sizes_widths_and_windows(cvs, lattices, size):
    rng = np.random.default_rng(size)
    domain = DOMAINS[size]
    for width in WIDTHS:
        for rows in (1, 3):
            for gname, sfull, scur, tfull in _geometries(width, rows):
                for half in (True, False):
                    pixels = _pixels16(rng, sfull, domain) if half else _pixels32(rng, sfull, domain)
                    what = "%dx%d %s" % (width, rows, gname)
                    _check(cvs, lattices, half, tfull, sfull, scur, pixels, size, domain, what)
                    if tfull == sfull:
                        _check(cvs, lattices, half, tfull, sfull, scur, pixels, size, domain, what, in_place=True)


def test_in_place_leaves_the_rest_of_the_buffer(cvs, lattices):
    rng = np.random.default_rng(7)
    full, cur = (-2, 0, 127, 2), (1, 1, 120, 2)
    _, dev = lattices(17)
    for half in (True, False):
        pixels = _pixels16(rng, full, SKEWED) if half else _pixels32(rng, full, SKEWED)
        got, window = _in_place(cvs, half, full, cur, pixels, dev, 17, SKEWED)
        assert window == cur
        outside = np.ones(_box(full), bool)
        lm.crop(outside, full, cur)[...] = False
        assert np.array_equal(got[outside].view(np.uint8), np.ascontiguousarray(pixels)[outside].view(np.uint8))
        assert not np.array_equal(lm.crop(got, full, cur), lm.crop(pixels, full, cur))


def test_empty_windows_are_a_success(cvs, lattices):
    _, dev = lattices(3)
    full = (0, 0, 9, 2)
    for half in (True, False):
        pixels = np.zeros(_box(full) + (4,), np.uint16 if half else np.float32)
        for scur, tfull in ((None, full), (full, (20, 0, 29, 2)), ((3, 0, 2, 2), full)):
            got, window, before = _once(cvs, half, tfull, full, scur, pixels, dev, 3, lm.UNIT)
            assert window is None and got.tobytes() == before.tobytes()


@pytest.mark.parametrize("roll", range(4))
def test_every_half_code(cvs, lattices, roll):
    """entry_cases.all_codes over 129 x 129, every half code (NaN, Inf and negatives included) in the channel positions `roll`
    moves them to, fed through in bands of three rows."""
    tall = np.roll(all_codes((0, 0, 128, 128), (0, 0, 128, 128)).array, roll, axis=-1)
    assert len(np.unique(tall[..., 0])) == 16384 and len(np.unique(tall)) == 65536
    full = (0, 0, 128, 2)
    for band in range(0, 129, 3):
        _check(cvs, lattices, True, full, full, full, np.ascontiguousarray(tall[band:band + 3]), 17, SKEWED, "all codes, rows %d.." % band)


@pytest.mark.parametrize("size", [2, 5, 10, 33])
def test_ties(cvs, lattices, size):
    frames = _tie_frames(size)
    for first in range(0, frames.shape[1], 129):
        s = np.ascontiguousarray(frames[:, first:first + 129])
        full = (0, 0, s.shape[1] - 1, 2)
        _check(cvs, lattices, False, full, full, full, s, size, lm.UNIT, "ties from %d" % first)
        codes = f2h_rz_model(s)
        codes[..., 1] = codes[..., 0]                                   # equal halfs: equal fractions
        _check(cvs, lattices, True, full, full, full, codes, size, lm.UNIT, "ties from %d" % first)


@pytest.mark.parametrize("size", [2, 3, 5, 9, 17, 33, 65])
def test_identity_lattice_returns_the_codes(cvs, size):
    """Straight from the device, without the model: an identity lattice on [0, 1] with N - 1 a power of two gives back every half
    code in [0, 1] and the f32 values of them."""
    flat = lm.packed(lm.identity(size))
    dev = cvs.cvs_malloc(flat.nbytes)
    assert dev
    try:
        _lib.check(cvs.cvs_memcpy_h2d(dev, flat.ctypes.data, flat.nbytes, None), "h2d")
        rng = np.random.default_rng(size)
        codes = rng.integers(0, 0x3C01, (3, 129, 4), dtype=np.uint16)
        codes[0, :4, :3] = [[0, 0, 0], [0x3C00] * 3, [0x3C00, 0, 0x0001], [0x3BFF, 0x0400, 0x03FF]]
        full = (0, 0, 128, 2)
        got, window, _ = _once(cvs, True, full, full, full, codes, dev, size, lm.UNIT)
        assert window == full and np.array_equal(got, codes)
        s = lm.widen(codes)
        got, window, _ = _once(cvs, False, full, full, full, s, dev, size, lm.UNIT)
        assert window == full and np.array_equal(got.view(np.uint32), s.view(np.uint32))
    finally:
        cvs.cvs_free(dev)


def test_entries_refuse_on_the_device(cvs, lattices):
    """With a device present the refusals are the contract's own (not the missing device's), and nothing is written."""
    full = (0, 0, 15, 2)
    _, dev = lattices(2)
    for half in (True, False):
        dtype, sentinel = (np.uint16, SENTINEL16) if half else (np.float32, SENTINEL32)
        before = np.broadcast_to(sentinel, _box(full) + (4,)).copy()
        source = DeviceFrame.from_host(HostFrame(full, dtype, before, full))
        target = DeviceFrame.from_host(HostFrame(full, dtype, before))
        try:
            for lattice, p, word in ((dev + 4, _lib.lut3d(2), "16-byte"), (dev, _lib.lut3d(66), "outside 2..65"), (dev, _lib.lut3d(2, (0, 0, 0), (1, 0, 1)), "ascending"),
                                     (dev, _lib.lut3d(2, flags=1), "flags"), (None, _lib.lut3d(2), "need")):
                cvs.cvs_clear_last_error()
                target.c.current_window = target.c.full_window
                assert _entry(cvs, half)(target.ref(), source.ref(), lattice, C.byref(p), None) == -1, word
                assert word in _lib.last_error() and target.current_window.is_empty(), word
            _lib.check(cvs.cvs_stream_sync(None), "sync")
            assert target.download().array.tobytes() == before.tobytes()
        finally:
            source.free(); target.free()


# ---------------------------------------------------------------- the node

@pytest.fixture(scope="module")
def process(cvs):
    from fluggo.media import process
    return process


@pytest.fixture(scope="module")
def bt():
    from fluggo.media import basetypes
    return basetypes


def _lut(process, size, domain, seed=None):
    lat = lm.distinct(size, size if seed is None else seed)
    return process.Lut3D(size, lat.reshape(-1), domain[0], domain[1]), lat


def test_node_pulls_equal_the_model_and_a_replaced_lattice_takes_effect(cvs, process):
    tape = Tape(RASTER)
    full = (-3, -2, 131, 2)
    node = None
    # another lattice, of another size and domain, between pulls: the device copy goes with the old one; then the first again
    for size, domain, seed in ((17, SKEWED, None), (5, lm.UNIT, 77), (17, SKEWED, None)):
        lut, lat = _lut(process, size, domain, seed)
        if node is None:
            node = process.VideoLut3DFilter(tape, lut)
        else:
            node.lut = lut
        assert node.lut is lut
        for index in (2, 5):
            codes = tape.picture(index)
            got16, w16 = _pull(node, index, full)                       # half-native source: the f16 entry, in place, one launch
            got32, w32 = _pull32(node, index, full)
            assert w16 == RASTER and w32 == RASTER
            _same(lm.crop(got16, full, RASTER), lm.apply_pixels(codes, lat, domain), True, "f16 pull, N=%d" % size)
            _same(lm.crop(got32, full, RASTER), lm.apply_pixels(lm.widen(codes), lat, domain), False, "f32 pull, N=%d" % size)
            tile = (10, 0, 70, 1)
            t16, tw16 = _pull(node, index, tile)
            assert tw16 == tile and np.array_equal(t16, lm.crop(got16, full, tile))
    node.set_source(None)
    assert _pull(node, 0, full)[1] is None and _pull32(node, 0, full)[1] is None


def test_node_over_a_device_source_pulled_as_f16(cvs, process, bt):
    """A source that is not half-native (a solid colour): the f16 pull is the f32 render truncated."""
    color, box, full = (0.1, 0.6, 0.15, 0.875), (5, 0, 100, 1), (0, 0, 128, 2)
    lut, lat = _lut(process, 10, lm.UNIT)
    node = process.VideoLut3DFilter(process.SolidColorVideoSource(color, bt.box2i(*box)), lut)
    s = np.broadcast_to(np.array(color, np.float32), _box(box) + (4,)).copy()
    want = lm.apply_f32(s, lat)
    got32, w32 = _pull32(node, 0, full)
    got16, w16 = _pull(node, 0, full)
    assert w32 == box and w16 == box
    _same(lm.crop(got32, full, box), want, False, "solid f32")
    _same(lm.crop(got16, full, box), f2h_rz_model(want), True, "solid f16")


@pytest.mark.parametrize("flavour,mode", FLAVOURS)
def test_graded_layer_over_a_solid_in_a_workspace(cvs, process, bt, flavour, mode):
    """The workspace pulls the node as f32 (nothing rounded before the over) and blends it over the solid at mix 1.0: the
    model's lookup, then the over -- tests/models.py over_model in the separate flavour (and the gcc oracle's over must agree
    with it), the contracting oracle build's over in the contracted one, which over_model does not state."""
    with _in_flavour(cvs, flavour, mode):
        tape = Tape(RASTER)
        full = RASTER
        lut, lat = _lut(process, 33, lm.UNIT)
        ground = (0.9, 0.1, 0.3, 0.75)
        ws = process.VideoWorkspace()
        ws.add(source=process.SolidColorVideoSource(ground, bt.box2i(*full)), x=0, length=10, z=0, offset=0)
        ws.add(source=process.VideoLut3DFilter(tape, lut), x=0, length=10, z=1, offset=0)
        lower = np.broadcast_to(np.array(ground, np.float32), _box(full) + (4,)).copy()
        codes = tape.picture(3)
        codes[..., 3] = np.random.default_rng(3).integers(0, 0x3C01, codes.shape[:2])      # (the tape's own alpha is 1 everywhere)
        tape.picture = lambda index: codes
        upper = lm.apply_f32(lm.widen(codes), lat)
        assert ((upper[..., 3] > 0) & (upper[..., 3] < 1)).any()
        acc = HostFrame(full, np.float32, lower.copy(), full)
        oracle.lib().orc_mix_over_f32(acc.ref(), HostFrame(full, np.float32, upper, full).ref(), C.c_float(1.0))
        assert acc.current_window.tuple() == full
        if flavour == "gcc":
            want, wwin = over_model(lower, full, upper, full, full, 1.0)
            assert tuple(wwin) == full
            _same(acc.array, want, False, "the oracle's over against over_model")
        else:
            want = acc.array
        got32, w32 = _pull32(ws, 3, full)
        got16, w16 = _pull(ws, 3, full)
        assert w32 == full and w16 == full
        _same(got32, want, False, "workspace f32 " + flavour)
        _same(got16, f2h_rz_model(want), True, "workspace f16 " + flavour)


def test_pull_queue_over_two_device_contexts_and_a_replaced_lattice(cvs, process, bt):
    """VideoPullQueue(devices=[0, 0]): two contexts on the one GPU, so the node makes a copy of the lattice in each on first use;
    the frames are the ones a direct pull gives.  Replacing the lattice from this thread frees both queue contexts' copies (each
    from a context this thread is not bound to) and the next pulls upload the new one; the thread's own context is unchanged."""
    import threading
    home = cvs.cvs_current_context()
    q = process.VideoPullQueue(workers=4, devices=[0, 0])
    assert len(set(q.contexts)) == 2
    window = bt.box2i(0, 0, 128, 2)
    source = process.SolidColorVideoSource(process.LerpFunc((0.1, 0.9, 0.3, 1.0), (0.8, 0.2, 0.6, 0.5), 8.0), window)
    node = None
    for size, domain, seed in ((17, SKEWED, None), (33, lm.UNIT, 5), (4, SKEWED, None)):
        lut, lat = _lut(process, size, domain, seed)
        if node is None:
            node = process.VideoLut3DFilter(source, lut)
        else:
            node.lut = lut
        assert cvs.cvs_current_context() == home
        want = {g: node.get_frame_f16(g, window) for g in range(8)}
        done, got = threading.Event(), {}

        def callback(frame_index, frame, user_data, got=got, done=done):
            got[frame_index] = frame
            if len(got) == 8:
                done.set()
        items = [q.enqueue(source=node, frame_index=g, window=window, callback=callback, user_data=None) for g in range(8)]
        assert [it.owner for it in items] == [g % 2 for g in range(8)]
        assert done.wait(60), "callbacks did not arrive"
        for g in range(8):
            colour = np.array([[tuple(source.get_frame_f32(g, window).pixel(5, 1))]], np.float32)
            model = canon_f16(f2h_rz_model(lm.apply_f32(colour, lat, domain))[0, 0])
            assert got[g].current_window == want[g].current_window
            for x, y in ((0, 0), (77, 1), (128, 2)):
                assert tuple(got[g].pixel(x, y)) == tuple(want[g].pixel(x, y)), (size, g, x, y)
                codes = np.array(tuple(got[g].pixel(x, y)), np.float32).astype(np.float16).view(np.uint16)
                assert np.array_equal(canon_f16(codes), model), (size, g, x, y)
        del items
    del node
    assert cvs.cvs_current_context() == home
