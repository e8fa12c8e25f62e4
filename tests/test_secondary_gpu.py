"""The secondaries on the GPU, bit for bit against the numpy model (tests/secondary_model.py; DESIGN.md "Secondaries"): every case
of tests/secondary_cases.py under both cvs_set_arithmetic settings.  Every operation of the contract is a correctly rounded IEEE
f32 operation or an exact conversion, so there is no tolerance anywhere: one differing code fails.  What is folded before
comparing is what tests/test_primary_gpu.py folds (tests/util.py canon_f16 / canon_f32): the sign of zero and the payload of a NaN.
Target pixels outside the window keep the sentinel, inputs come back unwritten.  Then the refusals, in place against out of place
on every permitted pair, and one buffer handed in as two and as three inputs."""
import ctypes as C

import numpy as np
import pytest

from canvas_amd import _lib
from canvas_amd.abi import HostFrame
from canvas_amd.device import DeviceFrame
from tests import secondary_cases as sc
from tests import secondary_model as sm
from tests.entry_cases import SENT16, SENT32, Twin, _box
from tests.util import canon_f16, canon_f32

pytestmark = pytest.mark.gpu

GROUP_IDS = [g[0] for g in sc.GROUPS]
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module", params=["separate", "contracted"])
def flavour(request, cvs):
    before = cvs.cvs_set_arithmetic(_lib.ARITH_CONTRACTED if request.param == "contracted" else _lib.ARITH_SEPARATE)
    yield request.param
    cvs.cvs_set_arithmetic(before if before >= 0 else _lib.ARITH_SEPARATE)


def _canon(a):
    return (canon_f16(a) if a.dtype == np.uint16 else canon_f32(a)).reshape(a.shape)


def _same(got, want, what):
    g, w = _canon(got), _canon(want)
    if not np.array_equal(g, w):
        raw = (lambda a: a) if got.dtype == np.uint16 else (lambda a: np.ascontiguousarray(a).view(np.uint32))
        bad = np.argwhere((g != w).any(axis=-1))
        y, x = bad[0]
        raise AssertionError("%s: %d pixels differ; first at buffer row %d column %d: got %s want %s" % (
            what, len(bad), y, x, [hex(int(v)) for v in raw(got)[y, x]], [hex(int(v)) for v in raw(want)[y, x]]))


class Kept(Twin):
    """Twin that keeps what every frame was uploaded with"""

    def _make_frame(self, o, host):
        Twin._make_frame(self, o, host)
        o.held = host.array.tobytes()


def _run(cvs, what, case):
    """The case on frames with allocations of their own -> (the written frame's pixels, its window or None); every input must
    come back as it was uploaded"""
    twin = Kept(cvs)
    try:
        rc = case(twin)
        assert rc == 0, "%s: returned %r (%s)" % (what, rc, _lib.last_error())
        got = twin.collect()
        outs = [k for k, o in enumerate(twin.objects) if o.out]
        assert len(outs) == 1, what
        for o, g in zip(twin.objects, got):
            if not o.out:
                assert g.tobytes() == o.held, "%s: %s was written" % (what, o.name)
        o = twin.objects[outs[0]]
        full = o.frame.full_window.tuple()
        pixels = got[outs[0]].view(np.uint16 if o.cls == "f16" else np.float32).reshape(_box(full) + (4,))
        window = None if o.frame.current_window.is_empty() else o.frame.current_window.tuple()
        return pixels, window
    finally:
        twin.free()


@pytest.mark.parametrize("gid,build", sc.GROUPS, ids=GROUP_IDS)
def test_every_case_against_the_model(cvs, flavour, gid, build):
    for what, case in build(cvs):
        got, window = _run(cvs, what, case)
        want, win = sc.expected(what)
        assert window == win, "%s: window %r, the model's %r" % (what, window, win)
        _same(got, want, what + ", " + flavour)


@pytest.mark.parametrize("gid,build", sc.GROUPS, ids=GROUP_IDS)
def test_in_place_equals_out_of_place_on_every_permitted_pair(cvs, flavour, gid, build):
    """Each in-place case against the out-of-place case of the same operands, over the pixels both wrote"""
    cases = dict(build(cvs))
    pairs = 0
    for what, d in sc.CASES.items():
        if what not in cases or d.get("place", "out") == "out":
            continue
        sibling = what.replace(" %s " % d["place"], " out ", 1)
        assert sibling in cases, what
        got, window = _run(cvs, what, cases[what])
        other, owin = _run(cvs, sibling, cases[sibling])
        full = {"source": d.get("sfull"), "key": d.get("kfull")}.get(d["place"]) or d["fulls"][{"a": 0, "b": 1, "matte": 2}[d["place"]]]
        both = sm.intersect(window, owin) if window and owin else None
        if both is not None:
            a, b = sm.crop(got, full, both), sm.crop(other, d["tfull"], both)
            assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), what + ": in place differs from out of place"
        pairs += 1
    assert pairs >= 20, pairs
    seen = {sc.CASES[w]["place"] for w in cases if "place" in sc.CASES[w]}
    assert seen == ({"out", "source", "key"} if gid.startswith("qualify") else {"out", "a", "b", "matte"}), seen


def _frames(half, full, cur, seeds):
    return [DeviceFrame.from_host(sc.picture(np.random.default_rng(s), half, full, cur)) for s in seeds]


@pytest.mark.parametrize("half", [True, False], ids=["f16", "f32"])
def test_one_buffer_as_two_and_as_three_inputs(cvs, flavour, half):
    """SHARED: inputs that are one buffer -- one struct handed in twice, and two structs over one buffer with windows of their own"""
    full, cur = (0, 0, 130, 8), (1, 0, 129, 8)
    dtype = np.uint16 if half else np.float32
    x, y = _frames(half, full, cur, (41, 42))
    hx, hy = x.download().array, y.download().array
    target = DeviceFrame.from_host(HostFrame(full, dtype, np.broadcast_to(SENT16 if half else SENT32, _box(full) + (4,)).copy()))
    again = DeviceFrame(full, dtype, (3, 1, 100, 7), ptr=x.ptr)                  # x's buffer under a window of its own
    before = target.download().array
    mix = cvs.cvs_matte_mix_f16_dev if half else cvs.cvs_matte_mix_f32_dev
    qual = cvs.cvs_qualify_f16_dev if half else cvs.cvs_qualify_f32_dev
    try:
        for luma, invert in sc.MIXES:
            p = _lib.matte_mix(luma, invert)
            for a, b, m in ((x, x, x), (x, x, y), (x, y, x), (y, x, x), (x, again, y), (again, x, again)):
                host = {id(x): (hx, cur), id(y): (hy, cur), id(again): (hx, again.current_window.tuple())}
                target.upload(before)
                assert mix(target.ref(), a.ref(), b.ref(), m.ref(), C.byref(p), None) == 0, _lib.last_error()
                _lib.check(cvs.cvs_stream_sync(None), "sync")
                args = [v for f in (a, b, m) for v in (host[id(f)][0], full, host[id(f)][1])]
                want, win = sm.expected_mix(before, full, *args, luma=luma, invert=invert)
                assert target.current_window.tuple() == win
                _same(target.download().array, want, "mix of shared buffers, luma %r invert %r" % (luma, invert))
        for q in sc.QUALIFIERS[::3]:
            p = sc.params(q)
            for key, kcur in ((x, cur), (again, again.current_window.tuple())):
                target.upload(before)
                assert qual(target.ref(), x.ref(), key.ref(), C.byref(p), None) == 0, _lib.last_error()
                _lib.check(cvs.cvs_stream_sync(None), "sync")
                want, win = sm.expected_qualify(before, full, hx, full, cur, q, hx, full, kcur)
                assert target.current_window.tuple() == win
                _same(target.download().array, want, "source as its own key, %r" % q)
        assert x.download().array.tobytes() == hx.tobytes() and y.download().array.tobytes() == hy.tobytes(), "an input was written"
    finally:
        x.free(); y.free(); target.free()


def test_entries_refuse_on_the_device(cvs):
    """With a device present the refusals are the contract's own: -1, the window emptied, nothing written, and cvs_last_error
    names the entry."""
    full = (0, 0, 15, 2)
    lim = _lib.MAX_COORD
    for half in (True, False):
        dtype, sentinel = (np.uint16, SENT16) if half else (np.float32, SENT32)
        frame_t = _lib.rgba_frame_f16 if half else _lib.rgba_frame_f32
        before = np.broadcast_to(sentinel, _box(full) + (4,)).copy()
        source = DeviceFrame.from_host(HostFrame(full, dtype, before, full))
        target = DeviceFrame.from_host(HostFrame(full, dtype, before))
        qname, mname = ("cvs_qualify_f16_dev", "cvs_matte_mix_f16_dev") if half else ("cvs_qualify_f32_dev", "cvs_matte_mix_f32_dev")
        qual, mix = getattr(cvs, qname), getattr(cvs, mname)
        outside = frame_t(source.ptr, _lib.box2i.of(*full), _lib.box2i.of(0, 0, 16, 2))
        far = frame_t(source.ptr, _lib.box2i.of(lim - 14, 0, lim + 1, 2), _lib.box2i.of(lim - 14, 0, lim + 1, 2))
        try:
            calls = []
            for p, word in REFUSED_QUALIFIERS:
                calls.append((qname, lambda p=p: qual(target.ref(), source.ref(), None, C.byref(p), None), word))
            good = _lib.qualifier(hue=(0, 60, 0))
            calls += [(qname, lambda: qual(target.ref(), None, None, C.byref(good), None), "need"),
                      (qname, lambda: qual(target.ref(), source.ref(), source.ref(), None, None), "need"),
                      (qname, lambda: qual(target.ref(), C.byref(outside), None, C.byref(good), None), "outside its buffer"),
                      (qname, lambda: qual(target.ref(), source.ref(), C.byref(outside), C.byref(good), None), "outside its buffer"),
                      (qname, lambda: qual(target.ref(), source.ref(), C.byref(far), C.byref(good), None), "beyond"),
                      (mname, lambda: mix(target.ref(), source.ref(), source.ref(), source.ref(), None, None), "need"),
                      (mname, lambda: mix(target.ref(), source.ref(), None, source.ref(), C.byref(_lib.matte_mix()), None), "need"),
                      (mname, lambda: mix(target.ref(), source.ref(), source.ref(), None, C.byref(_lib.matte_mix()), None), "need"),
                      (mname, lambda: mix(target.ref(), source.ref(), source.ref(), source.ref(), C.byref(_lib.matte_mix(flags=4)), None), "unknown flags"),
                      (mname, lambda: mix(target.ref(), source.ref(), source.ref(), C.byref(outside), C.byref(_lib.matte_mix()), None), "outside its buffer"),
                      (mname, lambda: mix(target.ref(), source.ref(), C.byref(far), source.ref(), C.byref(_lib.matte_mix()), None), "beyond")]
            for name, call, word in calls:
                cvs.cvs_clear_last_error()
                target.c.current_window = target.c.full_window
                assert call() == -1, (name, word)
                assert name in _lib.last_error() and word in _lib.last_error() and target.current_window.is_empty(), (name, word, _lib.last_error())
            _lib.check(cvs.cvs_stream_sync(None), "sync")
            assert target.download().array.tobytes() == before.tobytes() and source.download().array.tobytes() == before.tobytes()
        finally:
            source.free(); target.free()


# every refusal of a cvs_qualifier that the header lists, as (struct, a word of the message)
REFUSED_QUALIFIERS = (
    [(_lib.qualifier(flags=flags), "unknown flags") for flags in (32, 0x100, 0x80000001)]
    + [(_lib.qualifier(hue=hue), "hue range") for hue in ((NAN, 10, 0), (INF, 10, 0), (0, NAN, 0), (0, INF, 0), (0, -1, 0), (0, 10, NAN), (0, 10, INF), (0, 10, -0.5))]
    + [(_lib.qualifier(**{axis: rng}), axis + " range") for axis in ("saturation", "luma")
       for rng in ((NAN, 1, 0, 0), (-INF, 1, 0, 0), (INF, INF, 0, 0), (0, NAN, 0, 0), (0.5, 0.25, 0, 0), (0, -INF, 0, 0), (0, 1, NAN, 0), (0, 1, INF, 0), (0, 1, -1, 0),
                   (0, 1, 0, NAN), (0, 1, 0, INF), (0, 1, 0, -1))])
