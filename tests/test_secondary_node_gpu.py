"""process.VideoQualifierFilter, process.VideoMatteMixFilter and grade.secondary on the GPU against the numpy models composed by
tests/graph_model.py's route rule (pull): tests/secondary_model.py for the two nodes, tests/primary_model.py for the grade and
tests/matte_model.py for the choke and feather between them.  Pulled as f16 and as f32, into host frames and through the device
slot, at a 33 x 9 request window over sources whose windows differ; with frame functions for a hue centre and a luma bound at
two frame indices; with attributes set after construction; and with an empty pull from each source.  Codes are compared with
the sign of zero and the payload of a NaN folded, as tests/test_secondary_gpu.py does."""
import numpy as np
import pytest

from canvas_amd import _lib
from fluggo.media import grade
from tests import graph_model as gm
from tests import secondary_cases as sc
from tests import secondary_model as sm
from tests.test_fields_gpu import Tape as RealTape
from tests.test_fields_gpu import _pull
from tests.test_median_node_gpu import _pull_dev
from tests.test_primary_node_gpu import ColorCorrect, _same
from tests.test_unsharp_gpu import _pull32

pytestmark = pytest.mark.gpu

FLAVOURS = [("separate", _lib.ARITH_SEPARATE), ("contracted", _lib.ARITH_CONTRACTED)]
REQUEST = (5, 3, 37, 11)                        # 33 x 9
RASTER_A, RASTER_B, RASTER_M = (0, -2, 45, 28), (10, 0, 45, 28), (-4, 5, 30, 20)       # their intersection cuts the request on three sides
WINDOWS = [REQUEST, (-6, -4, 50, 30)]
MATRIX = grade.saturation_matrix(0.25)
INF = float("inf")


@pytest.fixture(scope="module")
def process(cvs):
    from fluggo.media import process
    return process


class Qualifier(gm.Node):
    """VideoQualifierFilter: pulls its source (and its key source) over the window asked for, in the format asked for"""
    any_format = True

    def __init__(self, source, hue=None, saturation=None, luma=None, key_source=None, invert=False, show_matte=False):
        self.sources = (source,) if key_source is None else (source, key_source)
        self.hue, self.saturation, self.luma, self.invert, self.show_matte = hue, saturation, luma, invert, show_matte

    def q(self, index):
        at = lambda axis: None if axis is None else tuple(gm.scalar(member, index) for member in axis)
        return sm.Qualifier(at(self.hue), at(self.saturation), at(self.luma), self.invert, self.show_matte)

    def render(self, index, full, fmt):
        src, scur = gm.pull(self.sources[0], index, full, fmt)
        if len(self.sources) == 1:
            return sm.expected_qualify(np.zeros_like(src), full, src, full, scur, self.q(index))
        key, kcur = gm.pull(self.sources[1], index, full, fmt)
        return sm.expected_qualify(np.zeros_like(src), full, src, full, scur, self.q(index), key, full, kcur)


class MatteMix(gm.Node):
    """VideoMatteMixFilter: the three sources over the window asked for, in the format asked for"""
    any_format = True

    def __init__(self, a, b, matte, channel="a", invert=False):
        self.sources, self.channel, self.invert = (a, b, matte), channel, invert

    def render(self, index, full, fmt):
        pulled = [gm.pull(s, index, full, fmt) for s in self.sources]
        args = [v for pixels, cur in pulled for v in (pixels, full, cur)]
        return sm.expected_mix(np.zeros_like(pulled[0][0]), full, *args, luma=self.channel == "luma", invert=self.invert)


def tape(raster, seed, specials=True):
    """(model tape, real tape): frame i is the secondaries' test picture over `raster`; specials=False: tests/graph_model.py's
    picture, colours and alphas in 0 .. 1 and nothing else, as the matte filter's own tests have it (its minimum and maximum
    leave a NaN's fate open)"""
    model = gm.Tape(raster, pictures=lambda index: sc.picture(np.random.default_rng([seed, index + 1000]), True, raster).array) if specials else gm.Tape(raster, seed)

    class PictureTape(RealTape):
        def picture(self, index):
            return model.picture(index)
    return model, PictureTape(raster)


def _real_axis(process, axis):
    return None if axis is None else tuple(gm._real(process, None, member) for member in axis)


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
def test_the_qualifier_against_the_model(cvs, process, flavour, mode):
    ma, ta = tape(RASTER_A, 1)
    mb, tb = tape(RASTER_B, 2)
    before = cvs.cvs_set_arithmetic(mode)
    try:
        for n, q in enumerate(sc.QUALIFIERS):
            keyed = n % 2 == 1
            node = process.VideoQualifierFilter(ta, hue=q.hue, saturation=q.saturation, luma=q.luma, key_source=tb if keyed else None, invert=q.invert, show_matte=q.show_matte)
            model = Qualifier(ma, q.hue, q.saturation, q.luma, mb if keyed else None, q.invert, q.show_matte)
            _check(cvs, node, model, n % 3, "qualifier %d %r" % (n, q), slots=n < 4)
            want, win = gm.pull(model, n % 3, REQUEST, gm.F16)
            assert win == (sm.intersect(REQUEST, RASTER_B) if keyed else REQUEST)
    finally:
        cvs.cvs_set_arithmetic(before if before >= 0 else _lib.ARITH_SEPARATE)


@pytest.mark.parametrize("flavour,mode", FLAVOURS)
def test_the_matte_mix_against_the_model(cvs, process, flavour, mode):
    ma, ta = tape(RASTER_A, 3)
    mb, tb = tape(RASTER_B, 4)
    mm, tm = tape(RASTER_M, 5)
    before = cvs.cvs_set_arithmetic(mode)
    try:
        for channel in ("a", "luma"):
            for invert in (False, True):
                node = process.VideoMatteMixFilter(ta, tb, tm, channel=channel, invert=invert)
                model = MatteMix(ma, mb, mm, channel, invert)
                _check(cvs, node, model, 1, "matte mix %s %r" % (channel, invert), slots=not invert)
                assert gm.pull(model, 1, REQUEST, gm.F16)[1] == (10, 5, 30, 11)
        # a source that renders in either format, and one buffer's worth of source three times
        solid = gm.Solid((0.1, 0.6, 0.15, 0.875), (8, 0, 40, 20))
        from fluggo.media import basetypes
        real_solid = process.SolidColorVideoSource((0.1, 0.6, 0.15, 0.875), basetypes.box2i(8, 0, 40, 20))
        _check(cvs, process.VideoMatteMixFilter(ta, real_solid, tm), MatteMix(ma, solid, mm), 2, "a solid as b")
        _check(cvs, process.VideoMatteMixFilter(ta, ta, ta), MatteMix(ma, ma, ma), 2, "one source three times", slots=False)
    finally:
        cvs.cvs_set_arithmetic(before if before >= 0 else _lib.ARITH_SEPARATE)


@pytest.mark.parametrize("flavour,mode", FLAVOURS)
def test_grade_secondary_is_the_composed_models(cvs, process, flavour, mode):
    """grade.secondary(source, graded, ...) with and without the VideoMatteFilter between the qualifier and the mix"""
    ma, ta = tape(RASTER_A, 6, specials=False)
    hue, luma = (30.0, 120.0, 30.0), (0.2, INF, 0.1, 0.0)
    before = cvs.cvs_set_arithmetic(mode)
    try:
        graded = process.VideoColorCorrectFilter(ta, None, MATRIX)
        model_graded = ColorCorrect(ma, None, MATRIX)
        plain = grade.secondary(ta, graded, hue=hue, luma=luma)
        assert type(plain.matte).__name__ == "VideoQualifierFilter"
        _check(cvs, plain, MatteMix(ma, model_graded, Qualifier(ma, hue, None, luma)), 0, "secondary, no refine")
        refined = grade.secondary(ta, graded, hue=hue, luma=luma, invert=True, choke=1, feather=gm.FEATHERS["taps3"])
        assert type(refined.matte).__name__ == "VideoMatteFilter" and refined.matte.source.invert is True
        model = MatteMix(ma, model_graded, gm.Matte(Qualifier(ma, hue, None, luma, invert=True), 1, "taps3"))
        _check(cvs, refined, model, 1, "secondary, choke and feather", slots=False)
        only_feather = grade.secondary(ta, graded, saturation=(0.3, 1.0, 0.1, 0.0), feather=gm.FEATHERS["taps5"])
        assert type(only_feather.matte).__name__ == "VideoMatteFilter"
        _check(cvs, only_feather, MatteMix(ma, model_graded, gm.Matte(Qualifier(ma, None, (0.3, 1.0, 0.1, 0.0)), 0, "taps5")), 2, "secondary, feather", windows=[REQUEST], slots=False)
    finally:
        cvs.cvs_set_arithmetic(before if before >= 0 else _lib.ARITH_SEPARATE)


def test_frame_functions_and_attributes_set_after_construction(cvs, process):
    ma, ta = tape(RASTER_A, 7)
    mb, tb = tape(RASTER_B, 8)
    centre, bound = gm.Lerp((0.0,), (360.0,), 4.0), gm.Lerp((0.1,), (0.5,), 4.0)
    hue, luma = (centre, 90.0, 20.0), (bound, INF, 0.125, 0.0)
    node = process.VideoQualifierFilter(ta, hue=_real_axis(process, hue), luma=_real_axis(process, luma))
    model = Qualifier(ma, hue, None, luma)
    for index in (1, 3):
        assert model.q(index).hue[0] == 90.0 * index and model.q(index).luma[0] == pytest.approx(0.1 + 0.1 * index)
        _check(cvs, node, model, index, "frame functions at %d" % index, slots=index == 1)
    # attributes, one at a time
    steps = [("saturation", (0.25, 0.75, 0.1, 0.1)), ("hue", None), ("invert", True), ("key_source", "b"), ("show_matte", True), ("luma", None), ("hue", (350.0, 40.0, 10.0)),
             ("key_source", None), ("invert", False)]
    for n, (attr, val) in enumerate(steps):
        if attr == "key_source":
            node.key_source = tb if val else None
            model.sources = (ma, mb) if val else (ma,)
            assert node.key_source is (tb if val else None)
        else:
            setattr(node, attr, val)
            setattr(model, attr, val)
            assert getattr(node, attr) == val
        for bad_attr, bad in (("hue", (1.0, 2.0)), ("hue", (0.0, -1.0, 0.0)), ("luma", (0.5, 0.25, 0.0, 0.0)), ("saturation", "x"), ("invert", 1)):
            with pytest.raises((TypeError, ValueError)):
                setattr(node, bad_attr, bad)
        _check(cvs, node, model, n % 3, "after setting %s" % attr, windows=[REQUEST], slots=n in (3, 4))
    mix = process.VideoMatteMixFilter(ta, tb, ta)
    mm = MatteMix(ma, mb, ma)
    for attr, val in (("channel", "luma"), ("invert", True), ("matte", "b"), ("src_a", "b"), ("src_b", "a"), ("channel", "a")):
        if attr in ("matte", "src_a", "src_b"):
            setattr(mix, attr, tb if val == "b" else ta)
            at = {"src_a": 0, "src_b": 1, "matte": 2}[attr]
            mm.sources = tuple((mb if val == "b" else ma) if k == at else s for k, s in enumerate(mm.sources))
        else:
            setattr(mix, attr, val)
            setattr(mm, attr, val)
            assert getattr(mix, attr) == val
        with pytest.raises((TypeError, ValueError)):
            mix.channel = "r"
        _check(cvs, mix, mm, 1, "mix after setting %s" % attr, windows=[REQUEST], slots=False)


def test_a_frame_function_that_leaves_the_contract_gives_an_empty_frame_and_says_why(cvs, process):
    _, ta = tape(RASTER_A, 9)
    node = process.VideoQualifierFilter(ta, hue=(0.0, process.LerpFunc((10.0,), (-30.0,), 4), 0.0))
    assert _pull(node, 0, REQUEST)[1] == REQUEST
    assert _pull(node, 2, REQUEST)[1] is None and "cvs_qualify_f16_dev" in process.last_error() and "hue range" in process.last_error()
    assert _pull32(node, 2, REQUEST)[1] is None and "cvs_qualify_f32_dev" in process.last_error()


def test_an_empty_pull_from_each_source(cvs, process):
    _, ta = tape(RASTER_A, 10)
    empty = process.EmptyVideoSource()
    elsewhere = (100, 100, 120, 110)                 # and a request none of the tapes reaches
    for source, key in ((empty, None), (ta, empty), (empty, ta), (None, None), (ta, None)):
        node = process.VideoQualifierFilter(source, hue=(0.0, 60.0, 0.0), key_source=key)
        window = elsewhere if source is ta and key is None else REQUEST
        for pull in (_pull, _pull32):
            assert pull(node, 0, window)[1] is None, (source, key)
    for k in range(3):
        sources = [ta, ta, ta]
        sources[k] = empty
        node = process.VideoMatteMixFilter(*sources)
        for pull in (_pull, _pull32):
            assert pull(node, 0, REQUEST)[1] is None, k
        sources[k] = None
        node = process.VideoMatteMixFilter(*sources)
        assert _pull(node, 0, REQUEST)[1] is None, k
    assert _pull(process.VideoMatteMixFilter(ta, ta, ta), 0, elsewhere)[1] is None
    out = grade.secondary(empty, ta, hue=(0.0, 60.0, 0.0), choke=1)
    assert _pull(out, 0, REQUEST)[1] is None and _pull32(out, 0, REQUEST)[1] is None
