"""What tests/test_far_windows_gpu.py takes for granted, established without a GPU: the expectations it applies far from the
origin hold there (DESIGN.md "Coordinates").

The catalogue's own cases (tests/entry_cases.py) are run on the CPU oracle -- the reference's pixel code in `int`, through a
stand-in library that hands cvs_X_dev(..., stream) to orc_X(...) on frames in host memory -- at the origin and through
entry_cases.Shifted at every offset the GPU module uses for that case: an equivariant case must give the origin's bytes and
windows, a modelled one must run and stay inside its buffers.  The Python models the other GPU modules tie the remaining
entries to (fields, key, matte, unsharp, transform) are evaluated the same way on a small frame each."""
import numpy as np
import pytest

from tests import entry_cases as ec
from tests import fields_model as fm
from tests import key_model as km
from tests import matte_model as mm
from tests import transform_model as tm
from tests import unsharp_model as um
from tests.models import f2h_rz_model
from tests.reference_library import NotInTheOracle, OnHost, OracleAsLibrary      # (shared with tests/test_extents_*.py)
from tests.util import same_window

# Offsets taken out for one group, by name, because the reference's own `int` code is undefined there: (group prefix, offset
# name) -> why.  None today.
ORACLE_UNDEFINED = {}


def _oracle_cases():
    lib = OracleAsLibrary()
    for gid, _pin, build in ec.GROUPS:
        if ec.FAR_CLASSES[gid.split("[")[0]][0] not in ("equivariant", "modelled"):
            continue
        for what, case in build(lib):
            yield gid, what, case


def test_the_oracle_at_every_far_offset():
    """Copies, gain, mixers, weave, blur, the bilinear scaler, the Lanczos resampler and blur + Lanczos, in f32 and composed for
    halfs and batches, as the reference's code computes them: at the offsets the GPU module runs each case at."""
    ran, reached, modelled, written_at_origin, written_far = 0, set(), set(), set(), set()
    for gid, what, case in _oracle_cases():
        cls, rule = ec.far_class(gid, what)
        near = OnHost(OracleAsLibrary())
        probe = ec.Shifted(near, (0, 0))
        try:
            assert case(probe) == 0
        except NotInTheOracle:
            continue
        want, want_windows = near.collect(), probe.windows_back()
        boxes = [(o.out, h.full_window.tuple()) for o, h in zip(near.objects, probe.hosts)]
        offsets = ec.far_offsets_for(gid, what, boxes)
        if gid.startswith("weave_fields"):
            offsets = offsets + ec.odd_dy_offsets(rule, boxes)           # modelled there: the oracle must run, not agree
        offsets = [o for o in offsets if (gid.split("[")[0], o[0]) not in ORACLE_UNDEFINED]
        assert len(offsets) >= 4, "%s / %s: far offsets %r" % (gid, what, offsets)
        if cls == "modelled":
            modelled.add(what)
            if isinstance(want[-1], np.ndarray) and not np.array_equal(want[-1], probe.hosts[-1].array):
                written_at_origin.add(what)
        for name, d, s in offsets:
            label = "%s / %s, %s: target moved by %r, source by %r" % (gid, what, name, d, s)
            inner = OnHost(OracleAsLibrary())
            far = ec.Shifted(inner, d, s)
            assert case(far) == 0
            got = inner.collect()
            for o, h, g in zip(inner.objects, far.hosts, got):
                w = o.frame.current_window
                assert w.is_empty() or (h.full_window.min.x <= w.min.x and w.max.x <= h.full_window.max.x and
                                        h.full_window.min.y <= w.min.y and w.max.y <= h.full_window.max.y), "%s: %s reports %r" % (label, o.name, w.tuple())
                if not o.out:
                    assert g.tobytes() == h.array.tobytes(), "%s: %s was written" % (label, o.name)
            if cls == "modelled" and not np.array_equal(got[-1], far.hosts[-1].array):
                written_far.add((what, name))                       # the far source was found: the target is not as it was
            if cls != "equivariant" or "dy odd" in name:
                continue
            for o, w, ww in zip(inner.objects, far.windows_back(), want_windows):
                assert same_window(w, ww), "%s: %s reports %r (translated back), at the origin %r" % (label, o.name, w.tuple(), ww.tuple())
            for o, g, w in zip(inner.objects, got, want):
                assert not o.out or g.tobytes() == w.tobytes(), "%s: %s differs from the origin's" % (label, o.name)
        ran += 1
        reached.add(gid.split("[")[0])
    # every modelled resampler case in every form, and each of them finds its source at every far offset it is run at
    assert len(modelled) >= 30, sorted(modelled)
    assert written_at_origin == modelled
    assert {w for w, _n in written_far} == modelled and len(written_far) >= 4 * len(modelled), sorted(modelled - {w for w, _n in written_far})
    assert ran > 100 and {"copies_and_conversions", "attenuate_in_place", "weave_fields", "mixers_f32", "blur_and_unsharp", "lanczos_resample",
                          "scale_bilinear"} <= reached, (ran, reached)


# ------------------------------------------------------------------ the Python models

FULL, CUR, TARGET = (-3, -2, 20, 11), (-1, 0, 17, 9), (2, -2, 25, 8)
RULES = {"any": ec._ANY, "even": ec._EVEN}


def _offsets(rule):
    return ec.far_offsets(rule, [(False, FULL), (True, TARGET)])


def _pixels(half, seed=7):
    rng = np.random.default_rng(seed)
    s = rng.uniform(-0.25, 1.25, (FULL[3] - FULL[1] + 1, FULL[2] - FULL[0] + 1, 4)).astype(np.float32)
    return f2h_rz_model(s) if half else s


def _before(half):
    h, w = TARGET[3] - TARGET[1] + 1, TARGET[2] - TARGET[0] + 1
    return np.broadcast_to(ec.SENT16 if half else ec.SENT32, (h, w, 4)).copy()


def _same_far(model, rule, half):
    """model(before, target_full, source, source_full, source_cur) -> (buffer, window): the same bytes, the window moved"""
    src = _pixels(half)
    want, win = model(_before(half), TARGET, src, FULL, CUR)
    offsets = _offsets(rule)
    assert len(offsets) >= 5
    for name, d, _s in offsets:
        got, w = model(_before(half), ec.move_box(TARGET, d), src, ec.move_box(FULL, d), ec.move_box(CUR, d))
        assert w == ec.move_box(win, d), (name, w, win)
        assert got.tobytes() == want.tobytes(), name


@pytest.mark.parametrize("half", [True, False], ids=["f16", "f32"])
def test_key_matte_and_unsharp_models_are_equivariant(half):
    _same_far(lambda b, tf, s, sf, sc: km.expected(b, tf, s, sf, sc, km.GREEN, 0.08, 0.25, 0.8, 0.4), ec._ANY, half)
    _same_far(lambda b, tf, s, sf, sc: mm.expected(b, tf, s, sf, sc, choke=2, feather=ec.ROUGH25[:5] / ec.ROUGH25[:5].sum(), black=0.1, white=0.9), ec._ANY, half)

    def box_blur(s32, sfull, scur, win):                     # any blur that is a function of the window's pixels alone
        c = um.crop(s32, sfull, win)
        return ((c + np.roll(c, 1, axis=1)) * np.float32(0.5)).astype(np.float32)
    _same_far(lambda b, tf, s, sf, sc: um.expected(b, tf, s, sf, sc, box_blur, 0.7, 0.01), ec._ANY, half)


def test_field_models_are_equivariant_under_an_even_dy_and_run_under_an_odd_one():
    from oracle import float_to_half
    src = _pixels(True)
    ops = {"field0": lambda cur, y0: fm.field_to_frame(cur, y0, 0, float_to_half), "field1": lambda cur, y0: fm.field_to_frame(cur, y0, 1, float_to_half),
           "soften": lambda cur, y0: fm.soften(cur, float_to_half)}
    other = _pixels(True, 8)
    for name, d, _s in _offsets(ec._EVEN) + [("odd dy", (-2 ** 16 - 2, 2 ** 15 + 1), None)]:
        for op, fn in ops.items():
            want, win = fm.expected_one_input(_before(True), TARGET, (src, FULL, CUR), fn)
            got, w = fm.expected_one_input(_before(True), ec.move_box(TARGET, d), (src, ec.move_box(FULL, d), ec.move_box(CUR, d)), fn)
            assert w == ec.move_box(win, d), (name, op)
            assert (got.tobytes() == want.tobytes()) == (d[1] % 2 == 0 or op == "soften"), (name, op)
        want, win = fm.expected_interlace(_before(True), TARGET, (src, FULL, CUR), (other, FULL, FULL))
        got, w = fm.expected_interlace(_before(True), ec.move_box(TARGET, d), (src, ec.move_box(FULL, d), ec.move_box(CUR, d)),
                                       (other, ec.move_box(FULL, d), ec.move_box(FULL, d)))
        assert w == ec.move_box(win, d), name
        assert (got.tobytes() == want.tobytes()) == (d[1] % 2 == 0), name


@pytest.mark.parametrize("half", [True, False], ids=["f16", "f32"])
def test_transform_model_runs_at_the_far_arguments(half):
    """Not equivariant (positions are formed in float): the model must run, report a window inside the target and write
    nothing but finite-or-source values there; at an offset of zero the hook returns the matrix unchanged."""
    rule = ec.FAR_CLASSES["transform"][1]
    src = _pixels(half)
    for mname, m in ec._transforms(TARGET[2] - TARGET[0] + 1, TARGET[3] - TARGET[1] + 1, CUR):
        assert ec.Shifted(OnHost(None), (0, 0)).matrix(m) == tuple(m)
        offsets = _offsets(rule)
        assert len(offsets) >= 4
        for name, d, s in offsets:
            far = ec.Shifted(OnHost(None), d, s).matrix(m)
            for filt in (tm.NEAREST, tm.BILINEAR):
                got, w = tm.expected(_before(half), ec.move_box(TARGET, d), src, ec.move_box(FULL, d), ec.move_box(CUR, d), far, filt)
                T = ec.move_box(TARGET, d)
                assert w is None or (T[0] <= w[0] <= w[2] <= T[2] and T[1] <= w[1] <= w[3] <= T[3]), (mname, name, w)
                assert got.shape == _before(half).shape
                if mname == "half-pixel shift" and filt == tm.NEAREST:
                    assert w is not None, (mname, name)             # an exact map: the source is still found where it was moved to
