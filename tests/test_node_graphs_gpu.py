"""Graphs of spatial nodes on the GPU, bit for bit against the composed model (tests/graph_model.py over the per-node models and
the CPU oracle in the arithmetic flavour under test).  What no single-node test reaches: window requests that feed window
requests, sources that answer with less than they were asked for, pooled intermediates that hold the previous node's pixels
outside their window, the half / float route through a deep graph, and several streams at once.  Pixels are compared after
tests/util.py canon_f16 / canon_f32 (the sign of zero and the payload of a NaN folded), through tests/test_key_gpu.py _same; a
pull promises nothing outside its current window, so both sides are set to zero there.  No tolerance anywhere."""
import ctypes as C
import gc
import threading
import time

import numpy as np
import pytest

from canvas_amd import _lib
from tests import graph_model as gm
from tests import unsharp_model as um
from tests.test_fields_gpu import _pull
from tests.test_key_gpu import _same
from tests.test_unsharp_gpu import _in_flavour, _pull32, _tiles

pytestmark = pytest.mark.gpu

FLAVOURS = [("gcc", _lib.ARITH_SEPARATE), ("fma", _lib.ARITH_CONTRACTED)]
MODES = dict(FLAVOURS)
FULL = (-3, -5, 50, 31)


@pytest.fixture(scope="module")
def process(cvs):
    from fluggo.media import process
    return process


@pytest.fixture(scope="module")
def bt():
    from fluggo.media import basetypes
    return basetypes


def _free_bytes(cvs):
    """tests/test_unsharp_gpu.py test_long_run_gives_device_memory_back's measure"""
    f, t = C.c_size_t(), C.c_size_t()
    _lib.check(cvs.cvs_stream_sync(None))
    cvs.cvs_pool_trim()
    _lib.check(cvs.cvs_mem_info(C.byref(f), C.byref(t)))
    return f.value


class Built:
    """The seed's graphs and the fixed chains as model and as real nodes, the tapes behind them, and the model's answers (made
    once per graph, frame, window, format and flavour, shared by the tests)."""

    def __init__(self, process, bt):
        self.tapes = []
        self.random = [(graph, raster, gm.build(process, bt, graph, self.tapes)) for graph, raster in gm.graphs()]
        self.fixed = {name: (graph, gm.build(process, bt, graph, self.tapes)) for name, graph in gm.fixed_chains().items()}
        self._answers = {}

    def model(self, graph, index, full, half, flavour):
        """Inside _in_flavour(flavour): the oracle build in force is that flavour's."""
        key = (id(graph), index, full, half, flavour)
        if key not in self._answers:
            self._answers[key] = gm.pull(graph, index, full, gm.F16 if half else gm.F32)
        return self._answers[key]


@pytest.fixture(scope="module")
def built(cvs, process, bt):
    return Built(process, bt)


def _canvas(pixels, full, win):
    out = np.zeros_like(pixels)
    if win is not None:
        um.crop(out, full, win)[...] = um.crop(pixels, full, win)
    return out


def _pulled(node, index, full, half):
    pixels, win = (_pull if half else _pull32)(node, index, full)
    return _canvas(pixels, full, win), win


def _check_whole_and_tiles(built, graph, node, index, full, flavour, what):
    """Both pulls over `full` equal the model's, window and pixels; the pull over each tile is the crop of the whole pull."""
    for half in (True, False):
        label = "%s frame %d %s %s window %r" % (what, index, "f16" if half else "f32", flavour, full)
        want, wwin = built.model(graph, index, full, half, flavour)
        got, win = _pulled(node, index, full, half)
        assert win == wwin, "%s: window %r, the model's %r" % (label, win, wwin)
        _same(got, want, half, label)
        for tile in _tiles(full):
            tgot, twin = _pulled(node, index, tile, half)
            assert twin == (None if win is None else um.intersect(win, tile)), "%s tile %r: window %r of %r" % (label, tile, twin, win)
            assert tgot.tobytes() == np.ascontiguousarray(um.crop(got, full, tile)).tobytes(), "%s: tile %r is not the crop of the whole pull" % (label, tile)


def _describe(node):
    return gm.kind(node) + ("(" + ", ".join(_describe(s) for s in node.sources) + ")" if node.sources else "")


@pytest.mark.parametrize("raster", ["raster", "wide"])
@pytest.mark.parametrize("flavour", list(MODES))
def test_random_graphs_against_the_model(cvs, built, flavour, raster):
    """The 48 graphs of the seed (36 on the 46 x 31 raster pulled over a window that reaches beyond it on every side, 12 on the
    300 x 41 one pulled whole and over a window starting on an odd column), frames 0 and 3, f16 and f32 pulls."""
    started, count = time.perf_counter(), 0
    with _in_flavour(cvs, flavour, MODES[flavour]):
        for n, (graph, on, node) in enumerate(built.random):
            if (on == gm.RASTER) != (raster == "raster"):
                continue
            for full in gm.windows(on):
                for index in gm.FRAMES:
                    _check_whole_and_tiles(built, graph, node, index, full, flavour, "graph %d %s" % (n, _describe(graph)))
                    count += 1
    assert count == {"raster": 36 * 2, "wide": 12 * 2 * 2}[raster]
    print("%d graph pulls in %.2f s" % (count, time.perf_counter() - started))


@pytest.mark.parametrize("name", list(gm.fixed_chains()))
def test_fixed_chains(cvs, built, name):
    """The chains that must be there whatever the seed, each in both flavours and both formats, whole and in tiles."""
    graph, node = built.fixed[name]
    for flavour, mode in FLAVOURS:
        with _in_flavour(cvs, flavour, mode):
            for index in (2, 5):
                _check_whole_and_tiles(built, graph, node, index, FULL, flavour, name)


def test_a_scaler_on_both_axes_pulled_whole(cvs, process, bt):
    """The generator's scalers enlarge along one axis, because the reference's two-pass scaler clips its intermediate frame to the
    target's window (video_scale.c:256-262) and so does not tile; pulled whole, a scaler on both axes in mid-chain is the
    model's like any other node."""
    graph = gm.Unsharp(gm.Scaler(gm.Blur(gm.Tape(gm.RASTER, 21), "gauss5"), (24.5, 12.0), (22.0, 13.5), (1.25, 1.5), gm._grow(gm.RASTER, -2)), "gauss9", 0.75)
    node = gm.build(process, bt, graph)
    for flavour, mode in FLAVOURS:
        with _in_flavour(cvs, flavour, mode):
            for half in (True, False):
                want, wwin = gm.pull(graph, 1, FULL, gm.F16 if half else gm.F32)
                got, win = _pulled(node, 1, FULL, half)
                assert win == wwin and win is not None
                _same(got, want, half, "scaler on both axes %s %s" % ("f16" if half else "f32", flavour))


def test_a_blurred_turned_layer_keeps_its_halo_in_a_tile(cvs, built):
    """The transform node used to report the entry's own window, which depends on how much of the source the pull asked for:
    pulled in this tile the turned layer's window began three rows lower than in the whole pull, and the blur above it, which
    writes nothing outside its source's window, lost the rows of its halo there.  The node now reports where source_rect lands
    in the window asked for."""
    graph, node = built.fixed["blur(transform(tape)), 13 taps over a turned layer"]
    tile = _tiles(FULL)[1]
    assert tile == (24, -5, 50, 13)
    for half in (True, False):
        whole, win = _pulled(node, 2, FULL, half)
        got, twin = _pulled(node, 2, tile, half)
        assert win == FULL and twin == tile
        assert got.tobytes() == np.ascontiguousarray(um.crop(whole, FULL, tile)).tobytes()
        assert (um.crop(whole, FULL, (24, -4, 28, -3))[..., 3] != 0).any()          # the halo the tile lost


def test_stale_pool_blocks_and_pulls_back_to_back(cvs, built, process, bt):
    """A throw-away pull of another graph of the same sizes first, so that its blocks are what the pool hands the checked pull
    (they hold that graph's plausible pixels outside the windows, where the entry tests put NaN); then the checked pull eight
    times in a row with nothing between the calls.  All eight equal the model."""
    graph, node = built.fixed["transform(blur(matte(key(tape))))"]
    other = gm.Transform(gm.Blur(gm.Matte(gm.Key(gm.Tape(gm.RASTER, 99), gm.TAPE_KEY, 0.0625, 0.5, 0.0, 0.0), -1, "taps5"), "gauss9"),
                         gm.RASTER, (20.0, 15.0), (0.875, 1.5), 20.0, (25.0, 11.0))
    decoy = gm.build(process, bt, other)
    for flavour, mode in FLAVOURS:
        with _in_flavour(cvs, flavour, mode):
            for half in (True, False):
                want, wwin = built.model(graph, 2, FULL, half, flavour)
                assert _pulled(decoy, 4, FULL, half)[1] is not None
                answers = [_pulled(node, 2, FULL, half) for _ in range(8)]
                for k, (got, win) in enumerate(answers):
                    assert win == wwin
                    _same(got, want, half, "pull %d of 8 after the decoy, %s %s" % (k, "f16" if half else "f32", flavour))


def _queue_jobs(built):
    return [(node, index, gm.windows(raster)[0]) for graph, raster, node in built.random for index in gm.FRAMES]


def _through_a_queue(queue, bt, jobs, in_flight=16):
    """jobs: [(node, frame, window)] -> the delivered frames, in order; at most `in_flight` enqueued at a time."""
    delivered = [None] * len(jobs)
    for first in range(0, len(jobs), in_flight):
        batch = range(first, min(first + in_flight, len(jobs)))
        done, lock, left = threading.Event(), threading.Lock(), [len(batch)]

        def callback(frame_index, frame, job):
            with lock:
                delivered[job] = frame
                left[0] -= 1
                if left[0] == 0:
                    done.set()

        items = [queue.enqueue(source=jobs[j][0], frame_index=jobs[j][1], window=bt.box2i(*jobs[j][2]), callback=callback, user_data=j) for j in batch]
        assert done.wait(60), "%d of %d frames did not arrive" % (left[0], len(batch))
        del items
    return delivered


@pytest.mark.parametrize("devices", [None, [0, 0]])
def test_graphs_through_a_pull_queue(cvs, built, process, bt, devices):
    """The 48 graphs, frames 0 and 3, through four workers on four streams (and on two device contexts of device 0), sixteen
    frames in flight: every delivered frame equals the direct pull of that graph and frame, every byte inside the window."""
    started = time.perf_counter()
    jobs = _queue_jobs(built)
    direct = [_pull(node, index, full) for node, index, full in jobs]
    queue = process.VideoPullQueue(workers=4) if devices is None else process.VideoPullQueue(workers=4, devices=devices)
    delivered = _through_a_queue(queue, bt, jobs)
    for j, ((node, index, full), (want, wwin), frame) in enumerate(zip(jobs, direct, delivered)):
        got, win = _pull(frame, 0, full)
        assert win == wwin, "graph %d frame %d: window %r, the direct pull's %r" % (j // 2, index, win, wwin)
        assert _canvas(got, full, win).tobytes() == _canvas(want, full, wwin).tobytes(), "graph %d frame %d differs from the direct pull" % (j // 2, index)
    del delivered, queue
    gc.collect()
    print("%d frames in %.2f s" % (len(jobs), time.perf_counter() - started))


def _workload(built, process, bt):
    """Every pull the file makes of the seed's graphs and the fixed chains, whole and in tiles, in both formats, and the graphs
    through both kinds of pull queue."""
    for graph, raster, node in built.random:
        for full in gm.windows(raster):
            for window in [full] + _tiles(full):
                for index in gm.FRAMES:
                    _pull(node, index, window)
                    _pull32(node, index, window)
    for graph, node in built.fixed.values():
        for window in [FULL] + _tiles(FULL):
            _pull(node, 2, window)
            _pull32(node, 2, window)
    for kw in (dict(workers=4), dict(workers=4, devices=[0, 0])):
        _through_a_queue(process.VideoPullQueue(**kw), bt, _queue_jobs(built))
    gc.collect()


def test_inputs_come_back_unwritten_and_device_memory_returns(cvs, built, process, bt):
    """Last in the file.  Every picture a tape handed out is still the one its seed gives.  Free device memory, by the measure
    of test_long_run_gives_device_memory_back: after one pass over the file's whole workload (the tap tables every context
    keeps exist then, and a queue's device contexts have been made) a second pass leaves it where it was.  Before the queue's
    contexts were handed on to the next queue, every VideoPullQueue(devices=...) opened two more and left their tables and
    parked scratch behind."""
    pictures = 0
    for model, tape in built.tapes:
        for index, codes in model._pictures.items():
            assert codes.tobytes() == model.fresh_picture(index).tobytes(), (model.seed, index)
            pictures += 1
    _workload(built, process, bt)
    assert pictures >= 2 * len(built.random)
    level, contexts = _free_bytes(cvs), cvs.cvs_context_count()
    _workload(built, process, bt)
    assert cvs.cvs_context_count() == contexts
    assert _free_bytes(cvs) == level
