"""Unsharp mask and blur nodes on the GPU, bit for bit against the model (tests/unsharp_model.py over the CPU oracle's blur in
the arithmetic flavour under test; DESIGN.md "Unsharp mask"), every case in both flavours.  Colour channels are compared with
the sign of zero and NaN payloads folded (tests/util.py canon_f16 / canon_f32), alpha code for code, target pixels outside the
window must keep a sentinel, inputs must come back unwritten.  No tolerance anywhere: one differing code fails."""
import ctypes as C
import threading

import numpy as np
import pytest

import oracle
from canvas_amd import _lib, synth
from canvas_amd.abi import HostFrame
from canvas_amd.device import DeviceFrame
from tests import unsharp_model as um
from tests.models import f2h_rz_model, over_model
from tests.test_fields_gpu import SPECIALS, Tape, _pull
from tests.util import canon_f16, canon_f32, f32p

pytestmark = pytest.mark.gpu

FLAVOURS = [("gcc", _lib.ARITH_SEPARATE), ("fma", _lib.ARITH_CONTRACTED)]
SENTINEL16 = np.array([0x7E17, 0x1234, 0xFBCD, 0x0001], np.uint16)
SENTINEL32 = np.array([1234.5, -7.25, 3.0e-5, 0.4375], np.float32)
AMOUNTS = [0.0, 0.5, 1.5, -1.0]
THRESHOLDS = [0.0, 2.0 ** -6, float("inf")]
FAST_TAPS = {
    "gauss3": synth.gaussian_taps(3, 0.8), "gauss5": synth.gaussian_taps(5, 1.0), "gauss9": synth.gaussian_taps(9, 1.5),
    "gauss13": synth.gaussian_taps(13, 2.0), "asym7": np.array([0.05, -0.15, 0.3, 0.5, 0.2, 0.15, -0.05], np.float32),
}
GENERAL_TAPS = {
    "even4": np.array([0.1, 0.4, 0.3, 0.2], np.float32), "gauss15": synth.gaussian_taps(15, 2.5), "gauss21": synth.gaussian_taps(21, 3.5),
    "inf5": np.array([0.1, 0.2, np.inf, 0.2, 0.1], np.float32),
}
SIZES = [(720, 480), (1920, 1080), (333, 71), (17, 9), (2, 1)]


def _box(full):
    return (full[3] - full[1] + 1, full[2] - full[0] + 1)


def _pixels(rng, full, layer=0):
    """synth.layer_pixels where the size allows, random halfs otherwise, with the special-half band of test_fields_gpu.py."""
    h, w = _box(full)
    if w >= 16 and h >= 16:
        codes = synth.layer_pixels(w, h, layer, int(rng.integers(0, 4)), opaque_base=False).copy()
    else:
        codes = rng.integers(0, 0x3C01, (h, w, 4), dtype=np.uint16)
    top = h // 3
    band = codes[top:top + 3]
    band[...] = SPECIALS[rng.integers(0, len(SPECIALS), band.shape)]
    scatter = rng.uniform(size=codes.shape) < 0.02
    codes[scatter] = SPECIALS[rng.integers(0, len(SPECIALS), int(scatter.sum()))]
    return codes


def _geometries(w, h):
    """(name, source full, source current or None, target full)"""
    full = (0, 0, w - 1, h - 1)
    inset = (1, 1 if h > 2 else 0, w - 2 if w > 3 else w - 1, h - 1)             # starts on an odd column: off the pair grid
    shifted = (w // 3, -(h // 2) - 1, w // 3 + w - 1, h - (h // 2) - 2 + 1)     # the target reaches beyond the source on two sides
    return [("whole", full, full, full), ("inset", full, inset, full), ("partly outside", full, full, shifted),
            ("disjoint", full, full, (w + 5, 0, 2 * w + 4, h - 1))]


def _oracle_blur(s32, sfull, scur, win, taps):
    """B over `win` from the oracle build in force."""
    src = HostFrame(sfull, np.float32, s32, scur)
    out = HostFrame(win, np.float32)
    oracle.lib().orc_fir_blur_f32(out.ref(), src.ref(), f32p(np.ascontiguousarray(taps, np.float32)), len(taps))
    assert out.current_window.tuple() == tuple(win)
    return out.array


def _call(cvs, half, target, source, taps, amount, threshold):
    t = np.ascontiguousarray(taps, np.float32)
    entry = cvs.cvs_unsharp_mask_f16_dev if half else cvs.cvs_unsharp_mask_f32_dev
    rc = entry(target.ref(), source.ref(), f32p(t), len(t), amount, threshold, None)
    kernel = cvs.cvs_fir_last_kernel()
    _lib.check(cvs.cvs_stream_sync(None), "sync")
    return rc, kernel


def _compare(got, want, half, what):
    """colours folded, alpha code for code"""
    g, w = (canon_f16(got), canon_f16(want)) if half else (canon_f32(got), canon_f32(want))
    g, w = g.reshape(got.shape).copy(), w.reshape(want.shape).copy()
    raw = (lambda a: a) if half else (lambda a: np.ascontiguousarray(a).view(np.uint32))
    g[..., 3], w[..., 3] = raw(got)[..., 3], raw(want)[..., 3]
    if not np.array_equal(g, w):
        bad = np.argwhere((g != w).any(axis=-1))
        y, x = bad[0]
        raise AssertionError("%s: %d pixels differ; first at buffer row %d column %d: got %s want %s" % (
            what, len(bad), y, x, [hex(int(v)) for v in raw(got)[y, x]], [hex(int(v)) for v in raw(want)[y, x]]))


def _check_geometry(cvs, codes, sfull, scur, tfull, taps, want_kernel, what, combos=None, blur=_oracle_blur, keep=None):
    """Both entries x every (amount, threshold) on one geometry and tap list, in the flavour in force.  want_kernel: the
    cvs_fir_last_kernel() every call must report (None: any).  keep: a dict that receives the results by (half, amount, threshold)."""
    s32 = um.widen(codes)
    win = None if scur is None else um.intersect(scur, tfull)
    blurred = None if win is None else blur(s32, sfull, scur, win, taps)
    for half in (True, False):
        dtype, sentinel = (np.uint16, SENTINEL16) if half else (np.float32, SENTINEL32)
        before = np.broadcast_to(sentinel, _box(tfull) + (4,)).copy()
        src_host = codes if half else s32
        source = DeviceFrame.from_host(HostFrame(sfull, dtype, src_host, (0, 0, -1, -1) if scur is None else scur))
        try:
            for amount, threshold in (combos or [(a, t) for a in AMOUNTS for t in THRESHOLDS]):
                label = "%s %s amount %g threshold %g" % (what, "f16" if half else "f32", amount, threshold)
                target = DeviceFrame.from_host(HostFrame(tfull, dtype, before))
                try:
                    rc, kernel = _call(cvs, half, target, source, taps, amount, threshold)
                    assert rc == 0, "%s: %s" % (label, _lib.last_error())
                    got = target.download().array
                    window = None if target.current_window.is_empty() else target.current_window.tuple()
                finally:
                    target.free()
                assert window == win, "%s: window %r, want %r" % (label, window, win)
                if want_kernel is not None:
                    assert kernel == want_kernel, "%s: kernel %d" % (label, kernel)
                want, _ = um.expected(before, tfull, src_host, sfull, scur, lambda *a: blurred, amount, threshold)
                _compare(got, want, half, label)
                if keep is not None:
                    keep[(half, amount, threshold)] = got
            assert source.download().array.tobytes() == np.ascontiguousarray(src_host).tobytes(), what + ": the input was written"
        finally:
            source.free()


def _in_flavour(cvs, name, mode):
    class ctx:
        def __enter__(self):
            self.prev = cvs.cvs_set_arithmetic(mode)
            self.orc = oracle.flavour(name)
            self.orc.__enter__()

        def __exit__(self, *exc):
            self.orc.__exit__(None, None, None)
            cvs.cvs_set_arithmetic(self.prev if self.prev >= 0 else _lib.ARITH_SEPARATE)
            return False
    return ctx()


@pytest.mark.timeout(1500)
@pytest.mark.parametrize("width,height", SIZES)
@pytest.mark.parametrize("flavour,mode", FLAVOURS)
def test_fused_entries(cvs, flavour, mode, width, height):
    """Both entries x the five fast tap lists x the four window geometries x every (amount, threshold) pair at one size; the
    oracle's blur is made once per geometry and tap list."""
    rng = np.random.default_rng(width * 131 + height)
    with _in_flavour(cvs, flavour, mode):
        for tname, taps in FAST_TAPS.items():
            for gname, sfull, scur, tfull in _geometries(width, height):
                codes = _pixels(rng, sfull)
                _check_geometry(cvs, codes, sfull, scur, tfull, taps, _lib.FIR_KERNEL_UNSHARP,
                                "%s %dx%d %s %s" % (flavour, width, height, tname, gname))


@pytest.mark.timeout(1500)
@pytest.mark.parametrize("flavour,mode", FLAVOURS)
def test_general_path(cvs, flavour, mode):
    """Tap lists the sweep has no instance for, and the fast lists with the table kernels pinned: the model's codes, and for
    the fast lists the fused run's codes."""
    rng = np.random.default_rng(77)
    with _in_flavour(cvs, flavour, mode):
        for width, height in [(333, 71), (64, 36), (17, 9)]:
            geometries = _geometries(width, height)[:3]
            for tname, taps in GENERAL_TAPS.items():
                for gname, sfull, scur, tfull in geometries:
                    codes = _pixels(rng, sfull)
                    what = "%s %dx%d %s %s" % (flavour, width, height, tname, gname)
                    _check_geometry(cvs, codes, sfull, scur, tfull, taps, None, what)
                    assert cvs.cvs_fir_last_kernel() not in (_lib.FIR_KERNEL_UNSHARP, _lib.FIR_KERNEL_NONE), what
            for tname, taps in FAST_TAPS.items():
                for gname, sfull, scur, tfull in geometries:
                    codes = _pixels(rng, sfull)
                    what = "%s %dx%d %s %s" % (flavour, width, height, tname, gname)
                    fused, tables = {}, {}
                    _check_geometry(cvs, codes, sfull, scur, tfull, taps, _lib.FIR_KERNEL_UNSHARP, what, keep=fused)
                    cvs.cvs_fir_path_override(_lib.FIR_PATH_TABLES)
                    try:
                        _check_geometry(cvs, codes, sfull, scur, tfull, taps, None, what + " tables pinned", keep=tables)
                        assert cvs.cvs_fir_last_kernel() not in (_lib.FIR_KERNEL_UNSHARP, _lib.FIR_KERNEL_WINDOW, _lib.FIR_KERNEL_WINDOW_PAIR), what
                    finally:
                        cvs.cvs_fir_path_override(_lib.FIR_PATH_AUTO)
                    assert fused.keys() == tables.keys() and len(fused) == 2 * len(AMOUNTS) * len(THRESHOLDS)
                    for key in fused:
                        half = key[0]
                        _compare(tables[key], fused[key], half, what + " tables against fused %r" % (key,))


@pytest.mark.timeout(3000)
def test_full_size_frame(cvs):
    """3840x2160 f16, 9 taps, both flavours (the oracle blurs a 4K frame on one host thread: one case, its own time budget)."""
    full = (0, 0, 3839, 2159)
    codes = _pixels(np.random.default_rng(4), full)
    for flavour, mode in FLAVOURS:
        with _in_flavour(cvs, flavour, mode):
            s32 = um.widen(codes)
            blurred = _oracle_blur(s32, full, full, full, FAST_TAPS["gauss9"])
            source = DeviceFrame.from_host(HostFrame(full, np.uint16, codes))
            target = DeviceFrame.from_host(HostFrame(full, np.uint16, np.broadcast_to(SENTINEL16, (2160, 3840, 4)).copy()))
            try:
                rc, kernel = _call(cvs, True, target, source, FAST_TAPS["gauss9"], 1.5, 2.0 ** -6)
                assert rc == 0 and kernel == _lib.FIR_KERNEL_UNSHARP and target.current_window.tuple() == full
                _compare(target.download().array, f2h_rz_model(um.mask(s32, blurred, 1.5, 2.0 ** -6)), True, "4K " + flavour)
            finally:
                source.free(); target.free()


# ---------------------------------------------------------------- the nodes

@pytest.fixture(scope="module")
def process(cvs):
    from fluggo.media import process
    return process


@pytest.fixture(scope="module")
def bt():
    from fluggo.media import basetypes
    return basetypes


RASTER = (0, -2, 45, 28)
TAPS5 = tuple(float(t) for t in FAST_TAPS["gauss5"])


def _pull32(node, index, full):
    """The node's f32 pull through the C entry a plugin host uses."""
    from canvas_amd.abi import video_frame_source_funcs, video_source
    lib = _lib.load()
    C.pythonapi.PyCapsule_GetPointer.restype = C.c_void_p
    C.pythonapi.PyCapsule_GetPointer.argtypes = [C.py_object, C.c_char_p]
    funcs = C.cast(C.pythonapi.PyCapsule_GetPointer(node._video_frame_source_funcs, b"_video_frame_source_funcs"), C.POINTER(video_frame_source_funcs))
    source = video_source(id(node), funcs)
    frame = HostFrame(full, np.float32)
    lib.video_get_frame_f32(C.byref(source), index, frame.ref())
    w = frame.current_window
    return frame.array, (None if w.is_empty() else w.tuple())


def _node_model(s32, sfull, scur, full, taps, amount, threshold):
    """(masked f32 pixels over the window, window) of a node pulled over `full` whose source holds s32 inside scur"""
    win = um.intersect(scur, full)
    blurred = _oracle_blur(s32, sfull, scur, win, taps)
    return um.mask(um.crop(s32, sfull, win), blurred, amount, threshold), win


def _check_node_pulls(node, index, full, want32, win, what):
    got16, w16 = _pull(node, index, full)
    got32, w32 = _pull32(node, index, full)
    assert w16 == win and w32 == win, (what, w16, w32, win)
    _compare(um.crop(got32, full, win), want32, False, what + " f32 pull")
    _compare(um.crop(got16, full, win), f2h_rz_model(want32), True, what + " f16 pull")
    return got16, got32


def _tiles(full):
    x0, y0, x1, y1 = full
    mx, my = (x0 + x1) // 2, (y0 + y1) // 2 + 1
    return [(x0, y0, mx, my - 1), (mx + 1, y0, x1, my - 1), (x0, my, mx, y1), (mx + 1, my, x1, y1)]


@pytest.mark.parametrize("flavour,mode", FLAVOURS)
def test_unsharp_node_over_solid_and_host_frames(cvs, process, bt, flavour, mode):
    with _in_flavour(cvs, flavour, mode):
        full = (0, 0, 63, 47)
        # a solid colour whose window lies inside the pull window: the mask sharpens its edges
        box = (5, 4, 40, 30)
        color = (0.25, 0.5, 0.75, 0.875)
        node = process.VideoUnsharpMaskFilter(process.SolidColorVideoSource(color, bt.box2i(*box)), TAPS5, 1.5, 2.0 ** -6)
        grown = (full[0] - 2, full[1] - 2, full[2] + 2, full[3] + 2)
        s32 = np.zeros(_box(grown) + (4,), np.float32)
        um.crop(s32, grown, box)[...] = np.array(color, np.float32)
        want, win = _node_model(s32, grown, box, full, FAST_TAPS["gauss5"], 1.5, 2.0 ** -6)
        assert win == box
        _check_node_pulls(node, 0, full, want, win, "solid " + flavour)
        # a half-native host-frame source of random pixels, whole and in four tiles
        tape = Tape()
        full = (-3, -5, 50, 31)
        for taps in (FAST_TAPS["gauss5"], FAST_TAPS["gauss13"], GENERAL_TAPS["even4"]):
            node = process.VideoUnsharpMaskFilter(tape, tuple(float(t) for t in taps), amount=0.5)
            s32 = um.widen(tape.picture(2))
            want, win = _node_model(s32, RASTER, RASTER, full, taps, 0.5, 0.0)
            assert win == RASTER
            whole16, whole32 = _check_node_pulls(node, 2, full, want, win, "tape %d taps %s" % (len(taps), flavour))
            for tile in _tiles(full):
                got16, w16 = _pull(node, 2, tile)
                got32, w32 = _pull32(node, 2, tile)
                tw = um.intersect(tile, RASTER)
                assert w16 == tw and w32 == tw, (tile, w16, w32)
                assert np.array_equal(um.crop(got16, tile, tw), um.crop(whole16, full, tw)), ("f16 tile", tile)
                assert np.array_equal(um.crop(got32, tile, tw).view(np.uint32), um.crop(whole32, full, tw).view(np.uint32)), ("f32 tile", tile)


def test_amount_follows_a_frame_function(cvs, process):
    tape = Tape()
    node = process.VideoUnsharpMaskFilter(tape, TAPS5, amount=process.LerpFunc((0.0,), (2.0,), 2.0), threshold=0.0)
    for flavour, mode in FLAVOURS:
        with _in_flavour(cvs, flavour, mode):
            for index in range(3):
                want, win = _node_model(um.widen(tape.picture(index)), RASTER, RASTER, RASTER, FAST_TAPS["gauss5"], float(index), 0.0)
                _check_node_pulls(node, index, RASTER, want, win, "lerp frame %d %s" % (index, flavour))
    assert np.array_equal(_pull(node, 0, RASTER)[0][..., 3], tape.picture(0)[..., 3])       # amount 0


def test_blur_node_equals_the_blur_entry(cvs, process):
    tape = Tape()
    full = (-3, -5, 50, 31)
    for taps in (FAST_TAPS["gauss9"], GENERAL_TAPS["even4"]):
        node = process.VideoBlurFilter(tape, tuple(float(t) for t in taps))
        for flavour, mode in FLAVOURS:
            with _in_flavour(cvs, flavour, mode):
                got, window = _pull(node, 1, full)
                source = DeviceFrame.from_host(HostFrame(RASTER, np.uint16, tape.picture(1)))
                target = DeviceFrame(full, np.uint16)
                try:
                    t = np.ascontiguousarray(taps, np.float32)
                    assert cvs.cvs_fir_blur_f16_dev(target.ref(), source.ref(), f32p(t), len(t), None) == 0
                    _lib.check(cvs.cvs_stream_sync(None), "sync")
                    assert window == target.current_window.tuple() == RASTER
                    assert np.array_equal(um.crop(got, full, RASTER), um.crop(target.download().array, full, RASTER)), (len(taps), flavour)
                finally:
                    source.free(); target.free()


@pytest.mark.parametrize("flavour,mode", FLAVOURS)
def test_node_under_a_workspace_overlay(cvs, process, bt, flavour, mode):
    """The node as a workspace's lowest item under one overlay: the workspace pulls it as f32 (nothing rounded before the
    over), blends the overlay over it at mix 1.0; the model's mask, then the over: tests/models.py over_model in the separate
    flavour (and the gcc oracle's over must agree with it), the contracting oracle build's over in the contracted one, which
    over_model does not state."""
    with _in_flavour(cvs, flavour, mode):
        tape = Tape()
        full = RASTER
        node = process.VideoUnsharpMaskFilter(tape, TAPS5, 1.5, 2.0 ** -6)
        top_color, top_box = (0.9, 0.1, 0.3, 0.4), (8, 5, 40, 20)
        ws = process.VideoWorkspace()
        ws.add(source=node, x=0, length=10, z=0, offset=0)
        ws.add(source=process.SolidColorVideoSource(top_color, bt.box2i(*top_box)), x=0, length=10, z=1, offset=0)
        lower, win = _node_model(um.widen(tape.picture(3)), RASTER, RASTER, full, FAST_TAPS["gauss5"], 1.5, 2.0 ** -6)
        assert win == full
        upper = np.zeros(_box(full) + (4,), np.float32)
        um.crop(upper, full, top_box)[...] = np.array(top_color, np.float32)
        # the over in the flavour under test is the oracle build's of that flavour; tests/models.py over_model states the
        # separately rounded one, so it is the expectation in the gcc flavour and must agree with the oracle there
        acc = HostFrame(full, np.float32, lower.copy(), full)
        oracle.lib().orc_mix_over_f32(acc.ref(), HostFrame(full, np.float32, upper, top_box).ref(), C.c_float(1.0))
        assert acc.current_window.tuple() == full
        if flavour == "gcc":
            want, wwin = over_model(lower, full, upper, top_box, full, 1.0)
            assert tuple(wwin) == full
            _compare(acc.array, want, False, "the oracle's over against over_model")
        else:
            want = acc.array
        got32, w32 = _pull32(ws, 3, full)
        got16, w16 = _pull(ws, 3, full)
        assert w32 == full and w16 == full
        _compare(got32, want, False, "workspace f32 " + flavour)
        _compare(got16, f2h_rz_model(want), True, "workspace f16 " + flavour)


def test_set_source_under_concurrent_pulls(cvs, process, bt):
    """Pull-queue workers read the node while the main thread keeps swapping its source between two solids: no crash, and
    every frame that comes back is one of the two sources' answers (49 pixels spread over the frame, corners and edges
    included, all from the same answer: the frame object is read pixel by pixel from a callback)."""
    window = bt.box2i(0, 0, 45, 28)
    full = (0, 0, 45, 28)
    solids = [process.SolidColorVideoSource(c, bt.box2i(-8, -8, 90, 60)) for c in ((0.25, 0.5, 0.75, 1.0), (0.75, 0.125, 0.5, 0.5))]
    for node in (process.VideoUnsharpMaskFilter(solids[0], TAPS5, 1.5), process.VideoBlurFilter(solids[0], TAPS5)):
        answers = []
        for s in solids:
            node.set_source(s)
            answers.append(_pull(node, 0, full)[0].copy())
        assert not np.array_equal(answers[0], answers[1])
        q = process.VideoPullQueue(workers=3)
        total, got, all_done, lock = 300, [], threading.Event(), threading.Lock()

        def callback(frame_index, frame, user_data):
            w = frame.current_window
            ok = w == window
            if ok:
                # the corners, the edges' middles and a lattice inside: all from ONE of the two answers
                spots = [(x, y) for y in (0, 1, 9, 14, 19, 27, 28) for x in (0, 1, 11, 22, 33, 44, 45)]
                px = [tuple(frame.pixel(x, y)) for x, y in spots]
                ok = any(px == [tuple(float(v) for v in a[y, x].view(np.float16)) for x, y in spots] for a in answers)
            with lock:
                got.append(ok)
                if len(got) == total:
                    all_done.set()

        def feeder():
            for i in range(total):
                q.enqueue(node, i % 7 - 3, window, callback, None)

        t = threading.Thread(target=feeder, daemon=True)
        t.start()
        writes = 0
        while not all_done.is_set() and writes < 100000:
            node.set_source(solids[writes % 2])
            writes += 1
        assert all_done.wait(60), "%s: %d of %d pulls came back after %d writes" % (type(node).__name__, len(got), total, writes)
        t.join(30)
        assert all(got), type(node).__name__
        # every pixel, once the swapping has stopped
        node.set_source(solids[1])
        assert np.array_equal(_pull(node, 0, full)[0], answers[1])


def test_long_run_gives_device_memory_back(cvs, process, bt):
    def free_bytes():
        f, t = C.c_size_t(), C.c_size_t()
        _lib.check(cvs.cvs_stream_sync(None))
        cvs.cvs_pool_trim()
        _lib.check(cvs.cvs_mem_info(C.byref(f), C.byref(t)))
        return f.value

    source = process.SolidColorVideoSource(process.LerpFunc((0.0, 1.0, 0.25, 1.0), (1.0, 0.0, 0.75, 1.0), 64.0), bt.box2i(-3, -3, 70, 50))
    graph = process.VideoUnsharpMaskFilter(process.VideoBlurFilter(process.VideoUnsharpMaskFilter(source, TAPS5, 1.5, 0.01),
                                                                   tuple(float(t) for t in GENERAL_TAPS["even4"])),
                                           tuple(float(t) for t in GENERAL_TAPS["gauss15"]), process.LerpFunc((0.0,), (2.0,), 50.0))
    window = bt.box2i(0, 0, 63, 35)

    def pulls(count):
        for i in range(count):
            assert not graph.get_frame_f16(i % 97 - 20, window).current_window.empty()
            if i % 4 == 0:
                assert not graph.get_frame_f32(i % 97 - 20, window).current_window.empty()

    pulls(50)
    start = free_bytes()
    pulls(2000)
    assert free_bytes() == start
