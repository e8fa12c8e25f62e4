"""process.VideoMedianFilter on the GPU against the numpy model (tests/median_model.py), composed with the models of the nodes
around it by tests/graph_model.py's route rule (pull): over a tape written in Python, pulled as f16 and as f32, into host frames
and through the device slot; in tiles; with a frame function as the threshold; under a VideoTransformFilter, inside a
VideoWorkspace over a solid, and between the chroma key and the matte refine.  The median's own bytes are compared raw."""
import ctypes as C

import numpy as np
import pytest

from canvas_amd import _lib
from canvas_amd.abi import video_frame_source_funcs, video_source
from tests import entry_cases as ec
from tests import graph_model as gm
from tests import median_model as mm
from tests.test_fields_gpu import Tape as RealTape
from tests.test_fields_gpu import _pull
from tests.test_unsharp_gpu import _pull32
from tests.util import canon_f16, canon_f32

pytestmark = pytest.mark.gpu

FLAVOURS = [("separate", _lib.ARITH_SEPARATE), ("contracted", _lib.ARITH_CONTRACTED)]
RASTER = (0, -2, 45, 28)
FULL = (-3, -5, 50, 31)
WINDOWS = [FULL, RASTER, (10, 3, 30, 20), (20, 10, 45, 28), (7, -1, 7, 9)]


@pytest.fixture(scope="module")
def process(cvs):
    from fluggo.media import process
    return process


@pytest.fixture(scope="module")
def bt():
    from fluggo.media import basetypes
    return basetypes


class Median(gm.Node):
    """VideoMedianFilter: pulls its source over the window asked for grown by the radius, then the entry of the pull's format"""
    filter = True

    def __init__(self, source, radius=1, threshold=0.0, channels="rgba"):
        self.sources, self.radius, self.threshold, self.channels = (source,), radius, threshold, channels

    def render(self, index, full, fmt):
        grown = gm._grow(full, self.radius)
        src, scur = gm.pull(self.sources[0], index, grown, fmt)
        bits = src if fmt == gm.F16 else np.ascontiguousarray(src).view(np.uint32)
        threshold = self.threshold(index) if callable(self.threshold) else self.threshold
        out, win = mm.expected(np.zeros(gm._box(full) + (4,), bits.dtype), full, bits, grown, scur, self.radius, threshold, self.channels)
        return (out if fmt == gm.F16 else out.view(np.float32)), win


def speck_tape(seed=0, specials=True):
    """(model tape, real tape): frame i is the speck picture over RASTER"""
    h, w = gm._box(RASTER)
    model = gm.Tape(RASTER, pictures=lambda index: mm.speck_picture(np.random.default_rng([seed, index + 1000]), w, h, np.uint16, specials))

    class SpeckTape(RealTape):
        def picture(self, index):
            return model.picture(index)
    return model, SpeckTape(RASTER)


def _pull_dev(cvs, node, index, full, half):
    """the node's device slot: (pixels over `full` as the format's numpy type, window or None)"""
    C.pythonapi.PyCapsule_GetPointer.restype = C.c_void_p
    C.pythonapi.PyCapsule_GetPointer.argtypes = [C.py_object, C.c_char_p]
    funcs = C.cast(C.pythonapi.PyCapsule_GetPointer(node._video_frame_source_funcs, b"_video_frame_source_funcs"), C.POINTER(video_frame_source_funcs))
    source = video_source(id(node), funcs)
    got = np.zeros(gm._box(full) + (4,), np.uint16 if half else np.float32)
    box = _lib.box2i.of(*full)
    d = _lib.rgba_frame_dev(cvs.cvs_malloc(got.nbytes), ec.FORMAT_F16 if half else ec.FORMAT_F32, box, box, None)
    try:
        _lib.check(cvs.cvs_memcpy_h2d(d.data, got.ctypes.data, got.nbytes, None))
        cvs.video_get_frame_dev(C.byref(source), index, C.byref(d))
        _lib.check(cvs.cvs_stream_sync(None))
        _lib.check(cvs.cvs_memcpy_d2h(got.ctypes.data, d.data, got.nbytes, None))
        return got, (None if d.current_window.is_empty() else d.current_window.tuple())
    finally:
        cvs.cvs_free(d.data)


def _same(got, gwin, want, wwin, full, what, fold=False):
    """windows equal; inside the window raw bytes equal -- or, where arithmetic of other nodes follows the median (fold), the
    codes with the sign of zero and the payload of a NaN folded, as tests/test_node_graphs_gpu.py compares them"""
    assert gwin == wwin, "%s: window %r, the model's %r" % (what, gwin, wwin)
    if wwin is not None:
        a, b = np.ascontiguousarray(mm.crop(got, full, wwin)), np.ascontiguousarray(mm.crop(want, full, wwin))
        if fold:
            canon = canon_f16 if a.dtype == np.uint16 else canon_f32
            a, b = canon(a), canon(b)
        assert a.tobytes() == b.tobytes(), what


@pytest.mark.parametrize("flavour,mode", FLAVOURS)
def test_the_node_against_the_model_in_both_formats_and_both_slots(cvs, process, flavour, mode):
    model_tape, tape = speck_tape()
    before = cvs.cvs_set_arithmetic(mode)
    try:
        for n, (radius, threshold, channels) in enumerate([(1, 0.0, "rgba"), (2, mm.THRESHOLD, "rgba"), (1, mm.THRESHOLD, "a"), (2, 0.0, "ga"), (2, mm.THRESHOLD, "rgb")]):
            node = process.VideoMedianFilter(tape, radius, threshold, channels)
            model = Median(model_tape, radius, threshold, channels)
            assert (node.radius, node.threshold, node.channels) == (radius, threshold, "".join(c for c in "rgba" if c in channels))
            for full in WINDOWS:
                what = "radius %d threshold %g channels %s window %r" % (radius, threshold, channels, full)
                want16, win16 = gm.pull(model, n, full, gm.F16)
                want32, win32 = gm.pull(model, n, full, gm.F32)
                assert win16 == win32 == mm.intersect(full, RASTER)
                _same(*_pull(node, n, full), want16, win16, full, what + ", f16 host frame")
                _same(*_pull32(node, n, full), want32, win32, full, what + ", f32 host frame")
                _same(*_pull_dev(cvs, node, n, full, True), want16, win16, full, what + ", f16 device slot")
                _same(*_pull_dev(cvs, node, n, full, False), want32, win32, full, what + ", f32 device slot")
            # the f16 pull over a half-native source is the f16 entry: the tape's own codes, selected
            got, win = _pull(node, n, RASTER)
            for c in range(4):
                assert np.isin(got[..., c], model_tape.picture(n)[..., c]).all()
    finally:
        cvs.cvs_set_arithmetic(before if before >= 0 else _lib.ARITH_SEPARATE)


def test_a_pull_in_tiles_equals_the_whole_pull(cvs, process):
    _, tape = speck_tape(3)
    x, y = 21, 10
    tiles = [(FULL[0], FULL[1], x - 1, y - 1), (x, FULL[1], FULL[2], y - 1), (FULL[0], y, x - 1, FULL[3]), (x, y, FULL[2], FULL[3]),
             (FULL[0], FULL[1], FULL[2], 10), (FULL[0], 11, FULL[2], FULL[3]), (5, 5, 5, 5)]
    for radius in (1, 2):
        node = process.VideoMedianFilter(tape, radius, mm.THRESHOLD)
        for pull in (_pull, _pull32):
            whole, window = pull(node, 2, FULL)
            assert window == RASTER
            for tile in tiles:
                part, twin = pull(node, 2, tile)
                assert twin == mm.intersect(tile, RASTER), tile
                assert np.array_equal(mm.crop(part, tile, twin).view(np.uint8), mm.crop(whole, FULL, twin).view(np.uint8)), (radius, tile)


def test_threshold_as_a_frame_function_and_the_attributes(cvs, process):
    model_tape, tape = speck_tape(5)
    node = process.VideoMedianFilter(tape, 2, threshold=process.LinearFrameFunc(0.03125, 0.0), channels="rgb")
    assert isinstance(node.threshold, process.LinearFrameFunc)
    model = Median(model_tape, 2, lambda i: 0.03125 * i, "rgb")
    different = 0
    for i in range(4):
        want, win = gm.pull(model, i, FULL, gm.F16)
        _same(*_pull(node, i, FULL), want, win, FULL, "frame %d" % i)
        other, _ = gm.pull(Median(model_tape, 2, 0.0, "rgb"), i, FULL, gm.F16)
        different += not np.array_equal(other, want)
    assert different == 3                                                 # frame 0 has threshold 0: every pixel takes the median
    # setters: a legal value is taken and shows in the next pull; a refused one raises and keeps the old
    node.threshold, node.radius, node.channels = 0.0, 1, "a"
    want, win = gm.pull(Median(model_tape, 1, 0.0, "a"), 1, FULL, gm.F16)
    _same(*_pull(node, 1, FULL), want, win, FULL, "after the setters")
    for attr, bad in (("radius", 3), ("channels", "xyz"), ("threshold", None)):
        with pytest.raises((TypeError, ValueError)):
            setattr(node, attr, bad)
    assert (node.radius, node.threshold, node.channels) == (1, 0.0, "a")
    # a threshold the entry refuses gives an empty window and no exception
    node.threshold = -1.0
    cvs.cvs_clear_last_error()
    assert _pull(node, 1, FULL)[1] is None and "threshold" in _lib.last_error()
    assert _pull32(node, 1, FULL)[1] is None
    node.threshold = 0.0
    node.set_source(None)
    assert _pull(node, 1, FULL)[1] is None and _pull32(node, 1, FULL)[1] is None
    node.source = process.EmptyVideoSource()
    assert _pull(node, 1, FULL)[1] is None


@pytest.mark.parametrize("flavour,mode", FLAVOURS)
def test_under_a_transform_and_inside_a_workspace(cvs, process, bt, flavour, mode):
    """the composed models: the transform's and the workspace's of tests/graph_model.py around the median's"""
    model_tape, tape = speck_tape(7, specials=False)
    rect = (2, 0, 40, 25)
    before = cvs.cvs_set_arithmetic(mode)
    try:
        import oracle
        with oracle.flavour("fma" if flavour == "contracted" else "gcc"):
            for radius, threshold in ((1, mm.THRESHOLD), (2, 0.0)):
                median, real_median = Median(model_tape, radius, threshold), process.VideoMedianFilter(tape, radius, threshold)
                for kw in (dict(position=(3.0, -2.0), filter="nearest"), dict(rotation=90.0, anchor=(20.0, 12.0), position=(20.0, 12.0), filter="bilinear"),
                           dict(scale=(1.25, 0.75), rotation=11.0, position=(1.5, 0.25), filter="bilinear")):
                    model = gm.Transform(median, rect, **kw)
                    node = process.VideoTransformFilter(real_median, bt.box2i(*rect), kw.get("anchor", (0.0, 0.0)), kw.get("scale", (1.0, 1.0)), kw.get("rotation", 0.0),
                                                        kw.get("position", (0.0, 0.0)), kw["filter"])
                    for full in (FULL, (10, 3, 30, 20)):
                        want, win = gm.pull(model, 1, full, gm.F32)
                        _same(*_pull32(node, 1, full), want, win, full, "transform %r over radius %d, f32" % (kw, radius), True)
                        want, win = gm.pull(model, 1, full, gm.F16)
                        _same(*_pull(node, 1, full), want, win, full, "transform %r over radius %d, f16" % (kw, radius), True)
                # (the solid over the tape's raster: the over of windows that differ can read outside one, tests/graph_model.py Undefined)
                solid = gm.Solid((0.125, 0.25, 0.5, 1.0), RASTER)
                model = gm.Workspace([dict(source=solid), dict(source=median)])
                ws = process.VideoWorkspace()
                ws.add(source=process.SolidColorVideoSource((0.125, 0.25, 0.5, 1.0), bt.box2i(*RASTER)), x=0, length=10, z=0, offset=0)
                ws.add(source=real_median, x=0, length=10, z=1, offset=0)
                for full in (FULL, (10, 3, 30, 20)):
                    want, win = gm.pull(model, 1, full, gm.F32)
                    _same(*_pull32(ws, 1, full), want, win, full, "workspace over radius %d, f32" % radius, True)
                    want, win = gm.pull(model, 1, full, gm.F16)
                    _same(*_pull(ws, 1, full), want, win, full, "workspace over radius %d, f16" % radius, True)
    finally:
        cvs.cvs_set_arithmetic(before if before >= 0 else _lib.ARITH_SEPARATE)


@pytest.mark.parametrize("flavour,mode", FLAVOURS)
def test_between_the_keyer_and_the_matte_refine(cvs, process, flavour, mode):
    """VideoMatteFilter(VideoMedianFilter(VideoChromaKeyFilter(tape), channels="a")): the three models in sequence, each pulling
    the window the next one asks for"""
    model_tape = gm.Tape(RASTER, seed=9)

    class KeyTape(RealTape):
        def picture(self, index):
            return model_tape.picture(index)
    tape = KeyTape(RASTER)
    before = cvs.cvs_set_arithmetic(mode)
    try:
        key = gm.Key(model_tape, gm.TAPE_KEY, 0.08, 0.25)
        model = gm.Matte(Median(key, 2, 0.0, "a"), 1, "taps5", 0.05, 0.95)
        real_key = process.VideoChromaKeyFilter(tape, tuple(gm.TAPE_KEY[:3]) + (1.0,), 0.08, 0.25, 0.0, 0.0, False)
        node = process.VideoMatteFilter(process.VideoMedianFilter(real_key, 2, 0.0, "a"), 1, gm.FEATHERS["taps5"], 0.05, 0.95, False)
        for full in (FULL, (10, 3, 30, 20)):
            want, win = gm.pull(model, 2, full, gm.F32)
            _same(*_pull32(node, 2, full), want, win, full, "key, median, matte: f32 %r" % (full,), True)
            want, win = gm.pull(model, 2, full, gm.F16)
            _same(*_pull(node, 2, full), want, win, full, "key, median, matte: f16 %r" % (full,), True)
    finally:
        cvs.cvs_set_arithmetic(before if before >= 0 else _lib.ARITH_SEPARATE)
