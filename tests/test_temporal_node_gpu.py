"""VideoTemporalDenoiseFilter on the GPU over a Python-written source of a short seeded clip, bit for bit against the model
(tests/temporal_model.py): both radii, the first and the last frames of the clip against the neighbours they have, threshold and
softness given as frame functions, channels="a" on a keyed matte (colour code for code), a pull in tiles against the whole pull,
the attribute setters, absent sources, and a long run that must leave the scratch pool where it started."""
import ctypes as C

import numpy as np
import pytest

from canvas_amd import _lib
from tests import fields_model as fm
from tests import temporal_model as tm
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
    """Frames lo .. hi - 1 over RASTER, nothing outside them: a still third with noise well under the threshold, a third that
    trembles by about the ramp's width from frame to frame and a third of unrelated noise, so that every class of the weights is
    met in every frame."""

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
            f[:, :a] += rng.uniform(-0.01, 0.01, (h, a, 4)).astype(np.float32)
            f[:, a:b] += rng.uniform(-0.05, 0.05, (h, b - a, 4)).astype(np.float32)
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


def _model(clip, i, radius, full, threshold, softness, channels, orc):
    """what a pull of `full` gives: (codes over full, window, weights), from the source frames as the node pulls them"""
    def frame(k):
        if k not in clip.frames:
            return None
        return (clip.frames[k], RASTER, fm.intersect(_grown(full), RASTER))
    before = np.zeros(_box(full) + (4,), np.uint16)
    cur = frame(i)
    if cur is None or cur[2] is None:
        return before, None, None
    far = (lambda k: frame(k)) if radius == 2 else (lambda k: None)
    after, window, _exact, w = tm.expected(before, full, cur, [frame(i - 1), frame(i + 1), far(i - 2), far(i + 2)], threshold, softness, channels, orc.float_to_half)
    return after, window, w


def _same(got, gwin, want, wwin, full, what):
    assert gwin == wwin, "%s: window %r, the model's %r" % (what, gwin, wwin)
    if wwin is not None:
        assert np.array_equal(canon_f16(fm.crop(got, full, wwin)), canon_f16(fm.crop(want, full, wwin))), what


@pytest.mark.parametrize("flavour,mode", FLAVOURS)
def test_the_node_against_the_model(cvs, orc, process, flavour, mode):
    clip = Clip(0, 6)
    before = cvs.cvs_set_arithmetic(mode)
    try:
        for radius in (1, 2):
            node = process.VideoTemporalDenoiseFilter(clip, radius, THRESHOLD, SOFTNESS)
            assert (node.radius, node.threshold, node.softness, node.channels) == (radius, THRESHOLD, SOFTNESS, "rgba")
            seen = np.zeros(3)
            for i in range(-3, 9):
                want, wwin, w = _model(clip, i, radius, FULL, THRESHOLD, SOFTNESS, tm.ALL, orc)
                got, gwin = _pull(node, i, FULL)
                _same(got, gwin, want, wwin, FULL, "radius %d frame %d" % (radius, i))
                assert (wwin is None) == (i < 0 or i > 5)
                if w is not None:
                    # the clip's first and last frames have weights on one side only
                    assert bool(w[0].any()) == (i >= 1) and bool(w[1].any()) == (i <= 4), i
                    assert bool(w[2].any()) == (radius == 2 and i >= 2) and bool(w[3].any()) == (radius == 2 and i <= 3), i
                    if 1 <= i <= 4:
                        seen += np.array(tm.classes(w[0])) > 0.05
            assert (seen == 4).all(), seen                                # every class in every inner frame of the clip
    finally:
        cvs.cvs_set_arithmetic(before if before >= 0 else _lib.ARITH_SEPARATE)


def test_a_pull_in_tiles_equals_the_whole_pull(cvs, process):
    clip = Clip(0, 5, seed=13)
    x, y = 21, 10                                                        # an odd first column and an even first row of the lower right tile
    tiles = [(FULL[0], FULL[1], x - 1, y - 1), (x, FULL[1], FULL[2], y - 1), (FULL[0], y, x - 1, FULL[3]), (x, y, FULL[2], FULL[3]),
             (FULL[0], FULL[1], FULL[2], 10), (FULL[0], 11, FULL[2], FULL[3])]
    for radius in (1, 2):
        node = process.VideoTemporalDenoiseFilter(clip, radius, THRESHOLD, SOFTNESS)
        for i in (0, 2, 4):
            whole, window = _pull(node, i, FULL)
            assert window == RASTER
            for tile in tiles:
                part, twin = _pull(node, i, tile)
                assert twin == fm.intersect(tile, RASTER), (i, tile)
                assert np.array_equal(fm.crop(part, tile, twin), fm.crop(whole, FULL, twin)), (radius, i, tile)


def test_alpha_alone_on_a_keyed_matte_leaves_colour_code_for_code(cvs, orc, process):
    """the temporal matte smoother: VideoChromaKeyFilter's matte shimmers from frame to frame, channels="a" averages it"""
    clip = Clip(0, 5, seed=19)
    keyed = process.VideoChromaKeyFilter(clip, (0.1, 0.8, 0.2), 0.3, 0.4)
    node = process.VideoTemporalDenoiseFilter(keyed, 2, 0.2, 0.2, channels="a")
    assert node.channels == "a"
    changed = 0
    for i in range(5):
        source, swin = _pull(keyed, i, FULL)
        got, gwin = _pull(node, i, FULL)
        assert gwin == swin == RASTER
        a, b = fm.crop(got, FULL, gwin), fm.crop(source, FULL, gwin)
        assert np.array_equal(a[..., :3], b[..., :3]), i
        changed += int((a[..., 3] != b[..., 3]).sum())
        # and the matte is the model's, from the keyed frames as the node pulls them
        frames = {k: _pull(keyed, k, _grown(FULL)) for k in range(i - 2, i + 3) if 0 <= k <= 4}
        frame = lambda k: (frames[k][0], _grown(FULL), frames[k][1]) if k in frames else None
        want, wwin, _exact, _w = tm.expected(np.zeros(_box(FULL) + (4,), np.uint16), FULL, frame(i), [frame(i - 1), frame(i + 1), frame(i - 2), frame(i + 2)],
                                             0.2, 0.2, tm.A, orc.float_to_half)
        _same(got, gwin, want, wwin, FULL, "matte frame %d" % i)
    assert changed > 500


def test_parameters_as_frame_functions_and_the_setters(cvs, orc, process):
    clip = Clip(0, 5, seed=17)
    node = process.VideoTemporalDenoiseFilter(clip, 1, threshold=process.LinearFrameFunc(0.03125, 0.015625), softness=SOFTNESS)
    assert isinstance(node.threshold, process.LinearFrameFunc)
    different = 0
    for i in range(5):
        threshold = 0.03125 * i + 0.015625
        want, wwin, _ = _model(clip, i, 1, FULL, threshold, SOFTNESS, tm.ALL, orc)
        got, gwin = _pull(node, i, FULL)
        _same(got, gwin, want, wwin, FULL, "frame %d" % i)
        other, _, _ = _model(clip, i, 1, FULL, 0.015625, SOFTNESS, tm.ALL, orc)
        different += not np.array_equal(canon_f16(other), canon_f16(want))
    assert different >= 3
    node = process.VideoTemporalDenoiseFilter(clip, 2, THRESHOLD, softness=process.LinearFrameFunc(0.0625, 0.0), channels="gb")
    for i in (0, 1, 3):
        want, wwin, _ = _model(clip, i, 2, FULL, THRESHOLD, 0.0625 * i, tm.G | tm.B, orc)
        got, gwin = _pull(node, i, FULL)
        _same(got, gwin, want, wwin, FULL, "softness function, frame %d" % i)
    # attributes: a refused value leaves the old one; a legal one is taken and changes the pull
    node.threshold, node.softness, node.radius, node.channels = 0.25, 0.125, 1, "ra"
    assert (node.threshold, node.softness, node.radius, node.channels) == (0.25, 0.125, 1, "ra")
    want, wwin, _ = _model(clip, 2, 1, FULL, 0.25, 0.125, tm.R | tm.A, orc)
    got, gwin = _pull(node, 2, FULL)
    _same(got, gwin, want, wwin, FULL, "after the setters")
    with pytest.raises(TypeError):
        node.softness = None
    with pytest.raises(ValueError):
        node.radius = 3
    with pytest.raises(TypeError):
        node.radius = 1.0
    with pytest.raises(ValueError):
        node.channels = "rr"
    with pytest.raises(ValueError):
        node.channels = ""
    assert (node.softness, node.radius, node.channels) == (0.125, 1, "ra")
    for bad in (0, 3, -1):
        with pytest.raises(ValueError):
            process.VideoTemporalDenoiseFilter(clip, bad)
    with pytest.raises(ValueError):
        process.VideoTemporalDenoiseFilter(clip, channels="x")
    # a parameter the entry refuses gives an empty window and no exception
    node.softness = -1.0
    cvs.cvs_clear_last_error()
    assert _pull(node, 1, FULL)[1] is None and "softness" in _lib.last_error()


def test_empty_and_absent_sources_give_empty_windows(process, bt):
    window = bt.box2i(-4, -4, 19, 11)
    nodes = lambda source: [process.VideoTemporalDenoiseFilter(source), process.VideoTemporalDenoiseFilter(source, 2, 0.0, 0.0, "a")]
    for source in (None, process.EmptyVideoSource()):
        for node in nodes(source):
            for i in (-2, 0, 1, 2 ** 31 - 1, -2 ** 31):
                assert node.get_frame_f16(i, window).current_window.empty(), i
                assert node.get_frame_f32(i, window).current_window.empty(), i
    far = bt.box2i(500, 500, 520, 510)                                   # a request the source has nothing in
    for node in nodes(Tape()):
        assert node.get_frame_f16(1, far).current_window.empty()
    # a neighbour whose index would leave int is absent, the frame itself is made
    for node in nodes(process.SolidColorVideoSource((0.25, 0.5, 0.75, 1.0), bt.box2i(0, -2, 45, 28))):
        for i in (2 ** 31 - 1, 2 ** 31 - 2, -2 ** 31, -2 ** 31 + 1):
            assert node.get_frame_f16(i, window).current_window == bt.box2i(0, -2, 19, 11), i


def test_long_run_gives_device_memory_back(cvs, process, bt):
    def free_bytes():
        f, t = C.c_size_t(), C.c_size_t()
        _lib.check(cvs.cvs_stream_sync(None))
        cvs.cvs_pool_trim()
        _lib.check(cvs.cvs_mem_info(C.byref(f), C.byref(t)))
        return f.value

    source = process.SolidColorVideoSource(process.LerpFunc((0.0, 1.0, 0.25, 1.0), (1.0, 0.0, 0.75, 1.0), 64.0), bt.box2i(-3, -3, 70, 50))
    graph = process.VideoTemporalDenoiseFilter(process.VideoTemporalDenoiseFilter(source, 2), 1, 0.01, 0.0)
    window = bt.box2i(0, 0, 63, 35)

    def pulls(count):
        for i in range(count):
            assert not graph.get_frame_f16(i % 97 - 20, window).current_window.empty()

    pulls(20)
    start = free_bytes()
    pulls(120)
    assert free_bytes() == start
