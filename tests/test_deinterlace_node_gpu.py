"""AdaptiveDeinterlaceFilter and AdaptiveBobDeinterlaceFilter on the GPU over a Python-written source of a short clip, bit for bit
against the model (tests/deinterlace_model.py): the first and the last frame of the clip have one neighbour absent, a pull in
four tiles equals the whole pull, threshold given as a frame function, the bob node's frame arithmetic at negative indices,
absent sources, set_source while pull-queue workers pull (the pull queue and not Python threads pulling through the GIL: DESIGN.md
§4.7 has the reason), and a long run that must leave the scratch pool where it started."""
import ctypes as C
import threading

import numpy as np
import pytest

from canvas_amd import _lib
from tests import deinterlace_model as dm
from tests import fields_model as fm
from tests.test_fields_gpu import RASTER, Tape, _box, _pull
from tests.util import canon_f16

pytestmark = pytest.mark.gpu

FLAVOURS = [("separate", _lib.ARITH_SEPARATE), ("contracted", _lib.ARITH_CONTRACTED)]
THRESHOLD, SOFTNESS = 0.05, 0.1
FULL = (-3, -5, 50, 31)


@pytest.fixture(scope="module")
def process(cvs):
    from fluggo.media import process
    return process


@pytest.fixture(scope="module")
def bt():
    from fluggo.media import basetypes
    return basetypes


class Clip(Tape):
    """Frames lo .. hi - 1 over RASTER, nothing outside them: a still third, a third that trembles by less than the ramp's
    width from frame to frame and a third of noise, so that every class of the weight is met in every frame."""

    def __init__(self, lo, hi, seed=7):
        Tape.__init__(self)
        self.lo, self.hi = lo, hi
        h, w = _box(RASTER)
        rng = np.random.default_rng(seed)
        base = rng.uniform(0.0, 1.0, (h, w, 4)).astype(np.float32)
        a, b = w // 3, w - w // 3
        self.frames = {}
        for i in range(lo, hi):
            f = base.copy()
            f[:, a:b] += rng.uniform(-0.06, 0.06, (h, b - a, 4)).astype(np.float32)
            f[:, b:] = rng.uniform(0.0, 1.0, (h, w - b, 4))
            self.frames[i] = f.astype(np.float16).view(np.uint16)

    def picture(self, index):
        return self.frames[index]

    def _fill(self, obj, index, fp):
        if index not in self.frames:
            f = fp.contents
            f.current_window.min.x, f.current_window.min.y, f.current_window.max.x, f.current_window.max.y = 0, 0, -1, -1
            return
        Tape._fill(self, obj, index, fp)


def _grown(full):
    return (full[0] - 1, full[1] - 1, full[2] + 1, full[3] + 1)


def _model(clip, source_frame, field, full, threshold, softness, orc):
    """what a pull of `full` gives: (codes over full, window), from the source frames as the node pulls them"""
    def frame(i):
        if i not in clip.frames:
            return None
        return (clip.frames[i], RASTER, fm.intersect(_grown(full), RASTER))
    before = np.zeros(_box(full) + (4,), np.uint16)
    cur = frame(source_frame)
    if cur is None or cur[2] is None:
        return before, None, None
    after, window, _exact, k = dm.expected(before, full, cur, frame(source_frame - 1), frame(source_frame + 1), field, threshold, softness, orc.float_to_half)
    return after, window, k


def _same(got, gwin, want, wwin, full, what):
    assert gwin == wwin, "%s: window %r, the model's %r" % (what, gwin, wwin)
    if wwin is not None:
        assert np.array_equal(canon_f16(fm.crop(got, full, wwin)), canon_f16(fm.crop(want, full, wwin))), what


@pytest.mark.parametrize("flavour,mode", FLAVOURS)
def test_both_nodes_against_the_model(cvs, orc, process, flavour, mode):
    clip = Clip(0, 5)
    before = cvs.cvs_set_arithmetic(mode)
    try:
        seen = np.zeros(3)
        for field in (0, 1):
            node = process.AdaptiveDeinterlaceFilter(clip, field, THRESHOLD, SOFTNESS)
            assert (node.field, node.threshold, node.softness) == (field, THRESHOLD, SOFTNESS)
            for i in range(-2, 7):
                want, wwin, k = _model(clip, i, field, FULL, THRESHOLD, SOFTNESS, orc)
                got, gwin = _pull(node, i, FULL)
                _same(got, gwin, want, wwin, FULL, "deinterlace field %d frame %d" % (field, i))
                assert (wwin is None) == (i < 0 or i > 4)
                if k is not None:
                    seen += np.array(dm.classes(k)) > 0
            bob = process.AdaptiveBobDeinterlaceFilter(clip, field, THRESHOLD, SOFTNESS)
            assert bob.first_field == field
            for j in range(-3, 13):
                want, wwin, _ = _model(clip, j >> 1, field ^ (j & 1), FULL, THRESHOLD, SOFTNESS, orc)
                got, gwin = _pull(bob, j, FULL)
                _same(got, gwin, want, wwin, FULL, "bob first field %d frame %d" % (field, j))
        assert (seen >= 10).all(), seen                                   # every class in every frame of the clip
    finally:
        cvs.cvs_set_arithmetic(before if before >= 0 else _lib.ARITH_SEPARATE)


def test_the_bob_node_at_negative_indices(cvs, orc, process):
    """frame arithmetic floors: output frame j shows source frame j >> 1 with field first_field ^ (j & 1)"""
    clip = Clip(-4, 3, seed=11)
    for first in (0, 1):
        bob = process.AdaptiveBobDeinterlaceFilter(clip, first_field=first, threshold=THRESHOLD, softness=SOFTNESS)
        for j in range(-9, 7):
            want, wwin, _ = _model(clip, j >> 1, first ^ (j & 1), FULL, THRESHOLD, SOFTNESS, orc)
            got, gwin = _pull(bob, j, FULL)
            _same(got, gwin, want, wwin, FULL, "bob first field %d frame %d" % (first, j))
            assert (wwin is None) == (j < -8 or j > 5), j


def test_a_pull_in_four_tiles_equals_the_whole_pull(cvs, orc, process):
    clip = Clip(0, 3, seed=13)
    x, y = 21, 10                                                        # an odd first column and an even first row of the lower right tile
    tiles = [(FULL[0], FULL[1], x - 1, y - 1), (x, FULL[1], FULL[2], y - 1), (FULL[0], y, x - 1, FULL[3]), (x, y, FULL[2], FULL[3])]
    for node in (process.AdaptiveDeinterlaceFilter(clip, 1, THRESHOLD, SOFTNESS), process.AdaptiveBobDeinterlaceFilter(clip, 0, THRESHOLD, SOFTNESS)):
        for i in (0, 1, 2) if node.__class__.__name__ == "AdaptiveDeinterlaceFilter" else (0, 1, 4, 5):
            whole, window = _pull(node, i, FULL)
            assert window == RASTER
            for tile in tiles + [(FULL[0], FULL[1], FULL[2], 10), (FULL[0], 11, FULL[2], FULL[3])]:
                part, twin = _pull(node, i, tile)
                assert twin == fm.intersect(tile, RASTER), (i, tile)
                assert np.array_equal(fm.crop(part, tile, twin), fm.crop(whole, FULL, twin)), (type(node).__name__, i, tile)


def test_threshold_and_softness_as_frame_functions(cvs, orc, process):
    clip = Clip(0, 5, seed=17)
    node = process.AdaptiveDeinterlaceFilter(clip, 0, threshold=process.LinearFrameFunc(0.03125, 0.015625), softness=SOFTNESS)
    assert isinstance(node.threshold, process.LinearFrameFunc)
    different = 0
    for i in range(5):
        threshold = 0.03125 * i + 0.015625
        want, wwin, _ = _model(clip, i, 0, FULL, threshold, SOFTNESS, orc)
        got, gwin = _pull(node, i, FULL)
        _same(got, gwin, want, wwin, FULL, "frame %d" % i)
        other, _, _ = _model(clip, i, 0, FULL, 0.015625, SOFTNESS, orc)
        different += not np.array_equal(canon_f16(other), canon_f16(want))
    assert different >= 3
    # the bob node evaluates them at the OUTPUT frame
    bob = process.AdaptiveBobDeinterlaceFilter(clip, 0, THRESHOLD, softness=process.LinearFrameFunc(0.0625, 0.0))
    for j in (0, 1, 4, 7):
        want, wwin, _ = _model(clip, j >> 1, j & 1, FULL, THRESHOLD, 0.0625 * j, orc)
        got, gwin = _pull(bob, j, FULL)
        _same(got, gwin, want, wwin, FULL, "bob frame %d" % j)
    # attributes: a refused value leaves the old one; a legal one is taken
    node.threshold = 0.25
    assert node.threshold == 0.25
    with pytest.raises(TypeError):
        node.softness = None
    assert node.softness == SOFTNESS
    with pytest.raises(ValueError):
        process.AdaptiveDeinterlaceFilter(clip, 2)
    with pytest.raises(ValueError):
        process.AdaptiveBobDeinterlaceFilter(clip, first_field=-1)
    # a parameter the entry refuses gives an empty window and no exception
    node.softness = -1.0
    cvs.cvs_clear_last_error()
    assert _pull(node, 1, FULL)[1] is None and "softness" in _lib.last_error()


def _nodes(process, source):
    return [process.AdaptiveDeinterlaceFilter(source), process.AdaptiveDeinterlaceFilter(source, 1, 0.0, 0.0),
            process.AdaptiveBobDeinterlaceFilter(source), process.AdaptiveBobDeinterlaceFilter(source, 1)]


def test_empty_and_absent_sources_give_empty_windows(process, bt):
    window = bt.box2i(-4, -4, 19, 11)
    for source in (None, process.EmptyVideoSource()):
        for node in _nodes(process, source):
            for i in (-2, 0, 1, 2 ** 31 - 1, -2 ** 31):
                assert node.get_frame_f16(i, window).current_window.empty(), (type(node).__name__, i)
                assert node.get_frame_f32(i, window).current_window.empty(), (type(node).__name__, i)
    far = bt.box2i(500, 500, 520, 510)                                   # a request the source has nothing in
    for node in _nodes(process, Tape()):
        assert node.get_frame_f16(1, far).current_window.empty(), type(node).__name__
    # a neighbour whose index would leave int is absent, the frame itself is made
    for node in _nodes(process, process.SolidColorVideoSource((0.25, 0.5, 0.75, 1.0), bt.box2i(0, -2, 45, 28))):
        for i in (2 ** 31 - 1, -2 ** 31):
            assert node.get_frame_f16(i, window).current_window == bt.box2i(0, -2, 19, 11), (type(node).__name__, i)


def test_set_source_under_concurrent_pulls(process, bt):
    """Pull-queue workers read each node (reader side of its lock, no GIL) while the main thread keeps replacing its source
    (writer side): every pull ends, with the whole window or -- source absent at that moment -- an empty one."""
    window = bt.box2i(0, -2, 45, 28)
    solid = process.SolidColorVideoSource((0.25, 0.5, 0.75, 1.0), bt.box2i(-8, -8, 90, 60))
    for node in _nodes(process, solid):
        q = process.VideoPullQueue(workers=3)
        total, got, all_done = 200, [], threading.Event()

        def callback(frame_index, frame, user_data):
            w = frame.current_window
            got.append(w.empty() or w == window)
            if len(got) == total:
                all_done.set()

        def feeder():
            for i in range(total):
                q.enqueue(node, i % 7 - 3, window, callback, None)

        t = threading.Thread(target=feeder, daemon=True)
        t.start()
        writes = 0
        while not all_done.is_set() and writes < 100000:
            node.set_source(None if writes % 2 == 0 else solid)
            writes += 1
        assert all_done.wait(60), "%s: %d of %d pulls came back after %d writes" % (type(node).__name__, len(got), total, writes)
        t.join(30)
        assert all(got), type(node).__name__
        node.set_source(solid)
        assert node.get_frame_f16(1, window).current_window == window


def test_long_run_gives_device_memory_back(cvs, process, bt):
    def free_bytes():
        f, t = C.c_size_t(), C.c_size_t()
        _lib.check(cvs.cvs_stream_sync(None))
        cvs.cvs_pool_trim()
        _lib.check(cvs.cvs_mem_info(C.byref(f), C.byref(t)))
        return f.value

    source = process.SolidColorVideoSource(process.LerpFunc((0.0, 1.0, 0.25, 1.0), (1.0, 0.0, 0.75, 1.0), 64.0), bt.box2i(-3, -3, 70, 50))
    graph = process.AdaptiveBobDeinterlaceFilter(process.AdaptiveDeinterlaceFilter(source, 1), 0, 0.01, 0.0)
    window = bt.box2i(0, 0, 63, 35)

    def pulls(count):
        for i in range(count):
            assert not graph.get_frame_f16(i % 97 - 20, window).current_window.empty()

    pulls(30)
    start = free_bytes()
    pulls(300)
    assert free_bytes() == start
