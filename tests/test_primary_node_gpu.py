"""process.VideoColorCorrectFilter on the GPU against the numpy model (tests/primary_model.py), composed with the models of the
nodes around it by tests/graph_model.py's route rule (pull): over a tape written in Python, pulled as f16 and as f32, into host
frames and through the device slot; in tiles; with attributes changed between pulls; inside a VideoWorkspace over a solid; as the
shaper in front of VideoLut3DFilter (tests/lut3d_model.py); after the chroma key; and with no stage set, where it hands its
source's frame on.  Codes are compared with the sign of zero and the payload of a NaN folded, as tests/test_primary_gpu.py does."""
import numpy as np
import pytest

from canvas_amd import _lib
from fluggo.media import grade
from tests import graph_model as gm
from tests import lut3d_model as lm
from tests import primary_model as pm
from tests.test_fields_gpu import Tape as RealTape
from tests.test_fields_gpu import _pull
from tests.test_median_node_gpu import _pull_dev
from tests.test_unsharp_gpu import _pull32
from tests.util import canon_f16, canon_f32

pytestmark = pytest.mark.gpu

FLAVOURS = [("separate", _lib.ARITH_SEPARATE), ("contracted", _lib.ARITH_CONTRACTED)]
RASTER = (0, -2, 45, 28)
FULL = (-3, -5, 50, 31)
WINDOWS = [FULL, RASTER, (10, 3, 30, 20), (7, -1, 7, 9)]
MATRIX = [0.75, 0.5, -0.25, 0.0625, 0.0, -1.0, 2.0, 0.0, 0.3, 0.3, 0.3, -0.2]
SHAPER_DOMAIN = ((-0.125, -0.125, -0.125), (1.5, 1.5, 1.5))     # the shaper's, wider than [0, 1] on both sides


@pytest.fixture(scope="module")
def process(cvs):
    from fluggo.media import process
    return process


@pytest.fixture(scope="module")
def bt():
    from fluggo.media import basetypes
    return basetypes


class ColorCorrect(gm.Node):
    """VideoColorCorrectFilter: pulls its source over the window asked for, into the frame itself, and grades it in place; with no
    stage the source's frame as it came"""
    filter = True

    def __init__(self, source, pre=None, matrix=None, post=None):
        self.sources, self.pre, self.matrix, self.post = (source,), pre, matrix, post

    def render(self, index, full, fmt):
        src, scur = gm.pull(self.sources[0], index, full, fmt)
        if self.pre is None and self.matrix is None and self.post is None:
            return src, scur
        return pm.expected(np.zeros_like(src), full, src, full, scur, self.pre, self.matrix, self.post)


class Lut3D(gm.Node):
    """VideoLut3DFilter, the same way, through tests/lut3d_model.py"""
    filter = True

    def __init__(self, source, lat, domain):
        self.sources, self.lat, self.domain = (source,), lat, domain

    def render(self, index, full, fmt):
        src, scur = gm.pull(self.sources[0], index, full, fmt)
        return lm.expected(np.zeros_like(src), full, src, full, scur, self.lat, self.domain)


def picture_tape(size, domain, seed=0):
    """(model tape, real tape): frame i is the test picture for curves of `size` nodes on `domain` over RASTER"""
    h, w = gm._box(RASTER)
    model = gm.Tape(RASTER, pictures=lambda index: pm.picture(np.random.default_rng([seed, index + 1000]), w, h, True, size, domain))

    class PictureTape(RealTape):
        def picture(self, index):
            return model.picture(index)
    return model, PictureTape(RASTER)


def _real(process, cv):
    return None if cv is None else process.ColorCurves(cv.size, cv.table, cv.domain[0], cv.domain[1])


def _same(got, gwin, want, wwin, full, what):
    assert gwin == wwin, "%s: window %r, the model's %r" % (what, gwin, wwin)
    if wwin is not None:
        a, b = np.ascontiguousarray(pm.crop(got, full, wwin)), np.ascontiguousarray(pm.crop(want, full, wwin))
        canon = canon_f16 if a.dtype == np.uint16 else canon_f32
        assert canon(a).tobytes() == canon(b).tobytes(), what


def _check(cvs, node, model, index, what, windows=WINDOWS, slots=True):
    for full in windows:
        want16, win16 = gm.pull(model, index, full, gm.F16)
        want32, win32 = gm.pull(model, index, full, gm.F32)
        _same(*_pull(node, index, full), want16, win16, full, "%s, window %r, f16 host frame" % (what, full))
        _same(*_pull32(node, index, full), want32, win32, full, "%s, window %r, f32 host frame" % (what, full))
        if slots:
            _same(*_pull_dev(cvs, node, index, full, True), want16, win16, full, "%s, window %r, f16 device slot" % (what, full))
            _same(*_pull_dev(cvs, node, index, full, False), want32, win32, full, "%s, window %r, f32 device slot" % (what, full))


@pytest.mark.parametrize("flavour,mode", FLAVOURS)
def test_the_node_against_the_model_in_both_formats_and_both_slots(cvs, process, flavour, mode):
    model_tape, tape = picture_tape(1025, pm.SKEWED)
    pre, post = pm.distinct(1025, pm.SKEWED, 1), pm.distinct(17, pm.WIDE, 2)
    before = cvs.cvs_set_arithmetic(mode)
    try:
        for n, (a, m, b) in enumerate([(pre, MATRIX, post), (pre, None, None), (None, MATRIX, None), (None, None, pre), (pre, None, post)]):
            node = process.VideoColorCorrectFilter(tape, _real(process, a), m, _real(process, b))
            _check(cvs, node, ColorCorrect(model_tape, a, m, b), n, "stages %d" % n)
        # a source that is not half-native: the f16 pull is the f32 render truncated
        solid = gm.Solid((0.1, 0.6, 0.15, 0.875), (5, 0, 40, 20))
        node = process.VideoColorCorrectFilter(process.SolidColorVideoSource((0.1, 0.6, 0.15, 0.875), _box2i(solid.window)), _real(process, pre), MATRIX, _real(process, post))
        _check(cvs, node, ColorCorrect(solid, pre, MATRIX, post), 0, "over a solid")
    finally:
        cvs.cvs_set_arithmetic(before if before >= 0 else _lib.ARITH_SEPARATE)


def _box2i(window):
    from fluggo.media import basetypes
    return basetypes.box2i(*window)


def test_a_pull_in_tiles_equals_the_whole_pull(cvs, process):
    _, tape = picture_tape(17, pm.WIDE, 3)
    node = process.VideoColorCorrectFilter(tape, _real(process, pm.distinct(17, pm.WIDE, 1)), MATRIX, _real(process, pm.distinct(3, pm.SKEWED, 2)))
    x, y = 21, 10
    tiles = [(FULL[0], FULL[1], x - 1, y - 1), (x, FULL[1], FULL[2], y - 1), (FULL[0], y, x - 1, FULL[3]), (x, y, FULL[2], FULL[3]), (5, 5, 5, 5)]
    for pull in (_pull, _pull32):
        whole, window = pull(node, 2, FULL)
        assert window == RASTER
        for tile in tiles:
            part, twin = pull(node, 2, tile)
            assert twin == pm.intersect(tile, RASTER), tile
            assert np.ascontiguousarray(pm.crop(part, tile, twin)).tobytes() == np.ascontiguousarray(pm.crop(whole, FULL, twin)).tobytes(), tile


def test_attributes_changed_between_pulls_and_the_node_without_a_stage(cvs, process):
    model_tape, tape = picture_tape(5, pm.UNIT, 5)
    a, b, c = pm.distinct(5, pm.UNIT, 1), pm.distinct(4097, pm.SKEWED, 2), pm.distinct(2, pm.WIDE, 3)
    ra, rb, rc = (_real(process, cv) for cv in (a, b, c))
    node = process.VideoColorCorrectFilter(tape)
    steps = [(None, None, None), (a, None, None), (a, MATRIX, None), (a, MATRIX, b), (b, MATRIX, a), (None, None, c), (c, grade.saturation_matrix(0.5), None), (None, None, None)]
    real = {id(a): ra, id(b): rb, id(c): rc, id(None): None}
    for n, (pre, matrix, post) in enumerate(steps):
        node.pre, node.matrix, node.post = real[id(pre)], matrix, real[id(post)]
        assert node.pre is real[id(pre)] and node.post is real[id(post)] and (node.matrix is None) == (matrix is None)
        _check(cvs, node, ColorCorrect(model_tape, pre, matrix, post), n % 3, "step %d" % n, windows=[FULL, (10, 3, 30, 20)], slots=(n in (0, 3)))
        for attr, bad in (("pre", 3), ("matrix", [1.0] * 5), ("matrix", [float("nan")] * 12), ("post", "x")):
            with pytest.raises((TypeError, ValueError)):
                setattr(node, attr, bad)
        _check(cvs, node, ColorCorrect(model_tape, pre, matrix, post), n % 3, "step %d after the refusals" % n, windows=[(10, 3, 30, 20)], slots=False)
    # with no stage the node is its source: the tape's own codes, NaNs and all, byte for byte
    got, win = _pull(node, 1, FULL)
    assert win == RASTER and pm.crop(got, FULL, RASTER).tobytes() == model_tape.picture(1).tobytes()
    node.set_source(None)
    assert _pull(node, 1, FULL)[1] is None and _pull32(node, 1, FULL)[1] is None
    node.pre = ra
    assert _pull(node, 1, FULL)[1] is None and _pull32(node, 1, FULL)[1] is None
    node.source = process.EmptyVideoSource()
    assert _pull(node, 1, FULL)[1] is None


@pytest.mark.parametrize("flavour,mode", FLAVOURS)
def test_inside_a_workspace(cvs, process, bt, flavour, mode):
    """the composed models: the workspace's of tests/graph_model.py around the node's.  Curves with values in 0 .. 1 and a picture
    without special codes, as the over's other tests have it."""
    h, w = gm._box(RASTER)
    model_tape = gm.Tape(RASTER, seed=7)

    class T(RealTape):
        def picture(self, index):
            return model_tape.picture(index)
    tape = T(RASTER)
    table, matrix = grade.cdl((1.1, 1.0, 0.9), (0.01, 0.0, -0.01), (1.0, 0.9, 1.2), 0.8, size=1025)
    pre = pm.Curves(table)
    before = cvs.cvs_set_arithmetic(mode)
    try:
        import oracle
        with oracle.flavour("fma" if flavour == "contracted" else "gcc"):
            real = process.VideoColorCorrectFilter(tape, process.ColorCurves(1025, table), matrix)
            graded = ColorCorrect(model_tape, pre, matrix)
            solid = gm.Solid((0.125, 0.25, 0.5, 1.0), RASTER)
            model = gm.Workspace([dict(source=solid), dict(source=graded)])
            ws = process.VideoWorkspace()
            ws.add(source=process.SolidColorVideoSource((0.125, 0.25, 0.5, 1.0), bt.box2i(*RASTER)), x=0, length=10, z=0, offset=0)
            ws.add(source=real, x=0, length=10, z=1, offset=0)
            _check(cvs, ws, model, 1, "workspace " + flavour, windows=[FULL, (10, 3, 30, 20)], slots=False)
    finally:
        cvs.cvs_set_arithmetic(before if before >= 0 else _lib.ARITH_SEPARATE)


def test_as_the_shaper_in_front_of_the_3d_lut(cvs, process):
    """VideoLut3DFilter(VideoColorCorrectFilter(tape, pre=shaper)): a linear -> Rec.709 shaper of 4097 nodes on a domain wider than
    [0, 1], then a 17-node cube on [0, 1]: the two models composed, each pulling the window the next asks for."""
    domain = SHAPER_DOMAIN
    model_tape, tape = picture_tape(4097, domain, 11)
    shaper = pm.Curves(grade.transfer_curves("linear_to_rec709", 4097, (domain[0][0], domain[1][0])), domain)
    lat = lm.distinct(17, 17)
    node = process.VideoLut3DFilter(process.VideoColorCorrectFilter(tape, pre=_real(process, shaper)), process.Lut3D(17, lat.reshape(-1)))
    model = Lut3D(ColorCorrect(model_tape, shaper), lat, lm.UNIT)
    _check(cvs, node, model, 2, "shaper and cube", windows=[FULL, (10, 3, 30, 20)])


@pytest.mark.parametrize("flavour,mode", FLAVOURS)
def test_after_the_keyer(cvs, process, flavour, mode):
    """VideoColorCorrectFilter(VideoChromaKeyFilter(tape)): the two models in sequence; the key's alpha passes code for code"""
    model_tape = gm.Tape(RASTER, seed=9)

    class KeyTape(RealTape):
        def picture(self, index):
            return model_tape.picture(index)
    tape = KeyTape(RASTER)
    pre, post = pm.distinct(17, pm.UNIT, 1), pm.distinct(1024, pm.WIDE, 2)
    before = cvs.cvs_set_arithmetic(mode)
    try:
        key = gm.Key(model_tape, gm.TAPE_KEY, 0.08, 0.25)
        model = ColorCorrect(key, pre, MATRIX, post)
        real_key = process.VideoChromaKeyFilter(tape, tuple(gm.TAPE_KEY[:3]) + (1.0,), 0.08, 0.25, 0.0, 0.0, False)
        node = process.VideoColorCorrectFilter(real_key, _real(process, pre), MATRIX, _real(process, post))
        _check(cvs, node, model, 2, "key, grade: " + flavour, windows=[FULL, (10, 3, 30, 20)])
        keyed, _ = gm.pull(key, 2, FULL, gm.F16)
        got, _ = _pull(node, 2, FULL)
        assert np.array_equal(pm.crop(got, FULL, RASTER)[..., 3], pm.crop(keyed, FULL, RASTER)[..., 3])
    finally:
        cvs.cvs_set_arithmetic(before if before >= 0 else _lib.ARITH_SEPARATE)
