"""Every device entry on operands that share a buffer (include/canvas_hip.h "Operands that share a buffer"; DESIGN.md the same).

The calls are the catalogue of tests/alias_cases.py, whose policy table tests/test_alias_cases_cpu.py holds to the headers.
Each case is run with one struct handed in for both operands of its pair, and with two structs over one buffer.

"in place" and "shared" cases: the return code is 0 and no message is left; every reported window is the reference's; every
output -- the whole buffer -- equals tests/reference_library.py on DISTINCT host operands (code for code, or canonical codes
where the object's cmp says so; inside the reported window alone for reference_library.WINDOW_ONLY, the scaler between half
frames, whose reference defines no more), and, as a second witness, the whole buffer of the same entry's run on distinct
device frames; every operand that is only read holds the bytes that were uploaded.

"refused" cases: the return code is nonzero; cvs_last_error() names the entry with one of the two wordings; every written
frame's window is empty; after cvs_stream_sync every byte of every operand is what was uploaded; cvs_fir_last_kernel() is
what it was.  And a refusal leaves no trace: the pool's free bytes after a trim are what they were, 130 refused blur calls
with tap lists of their own (more than the 128 tap tables a context caches) leave room for a legal call's tables, and a
refusal while a stream is capturing ends nothing: the graph replays the legal call recorded after it.

Both arithmetic flavours, set here as tests/test_placement_gpu.py does."""
import ctypes as C

import numpy as np
import pytest

import oracle
from canvas_amd import _lib
from canvas_amd.device import DeviceFrame
from tests import alias_cases as ac
from tests import entry_cases as ec
from tests import reference_library as rl
from tests.test_graph_replay_gpu import AXIS_CACHE, Kept, _free_bytes, record
from tests.test_placement_gpu import _canon
from tests.util import f32p, same_window

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["separate", "contracted"])
def flavour(request, cvs):
    before = cvs.cvs_set_arithmetic(_lib.ARITH_CONTRACTED if request.param == "contracted" else _lib.ARITH_SEPARATE)
    yield request.param
    cvs.cvs_set_arithmetic(before if before >= 0 else _lib.ARITH_SEPARATE)
    cvs.cvs_fir_path_override(_lib.FIR_PATH_AUTO)


@pytest.fixture(scope="module")
def stream(cvs):
    s = cvs.cvs_stream_create()
    assert s, _lib.last_error()
    yield s
    _lib.check(cvs.cvs_stream_sync(s))
    cvs.cvs_stream_destroy(s)


def _oracle_flavour(flavour):
    return oracle.flavour("fma" if flavour == "contracted" else "gcc")


def _spec(objects):
    return [(o.cls, o.name, o.out, o.cmp, o.nbytes) for o in objects if not o.name.startswith(ac.DISTINCT)]


def _held(o):
    """the bytes of an object of the reference side"""
    return np.ascontiguousarray(o.frame.array if o.frame is not None else o.array).reshape(-1).view(np.uint8)


def _differs(label, o, got, want, against, window=None):
    """`window`: compare inside it alone (reference_library.WINDOW_ONLY: the scaler between half frames defines no more)"""
    a, b = _canon(got, o.cmp), _canon(want, o.cmp)
    if window is not None and not window.is_empty():
        full = o.frame.full_window
        ys, xs = slice(window.min.y - full.min.y, window.max.y - full.min.y + 1), slice(window.min.x - full.min.x, window.max.x - full.min.x + 1)
        a, b = (v.reshape(full.height, full.width, -1)[ys, xs].reshape(-1) for v in (a, b))
    if not np.array_equal(a, b):
        bad = np.flatnonzero(a != b)
        raise AssertionError("%s: %s differs from %s in %d of %d elements, first at element %d: 0x%x against 0x%x" % (
            label, o.name, against, bad.size, a.size, bad[0], a[bad[0]], b[bad[0]]))


def _in_place_or_shared(cvs, flavour, case, ref_case):
    with _oracle_flavour(flavour):
        host = rl.OnHostWithBuffers(None)
        assert ref_case(host, "distinct") == 0
    ref = [o for o in host.objects if not o.name.startswith(ac.DISTINCT)]
    twin = Kept(cvs)
    try:
        assert case(twin, "distinct") == 0, "%s on distinct frames: %s" % (case.what, _lib.last_error())
        distinct = [g for o, g in zip(twin.objects, twin.collect()) if not o.name.startswith(ac.DISTINCT)]
    finally:
        twin.free()
    for form in ac.FORMS:
        label = "%s, %s" % (case.what, form)
        fac = Kept(cvs)
        try:
            cvs.cvs_clear_last_error()
            rc = case(fac, form)
            got = fac.collect()
            assert _spec(fac.objects) == _spec(host.objects), label + ": the case is not the reference's case"
            assert rc == 0, "%s: returned %r (%s)" % (label, rc, _lib.last_error())
            assert _lib.last_error() == "", "%s: returned 0 and left the message %r" % (label, _lib.last_error())
            for o, r in zip(fac.objects, ref):
                if o.frame is not None:
                    w, ww = o.frame.current_window, r.frame.current_window
                    assert same_window(w, ww), "%s: %s reports window %r, the reference %r" % (label, o.name, w.tuple(), ww.tuple())
            for o, g, r, d in zip(fac.objects, got, ref, distinct):
                if o.out:
                    _differs(label, o, g, _held(r), "the reference on distinct operands",
                             r.frame.current_window if case.entry in rl.WINDOW_ONLY else None)
                    _differs(label, o, g, d, "the entry's own run on distinct frames")
                else:
                    assert np.array_equal(g, o.initial), "%s: %s, which is only read, was written" % (label, o.name)
        finally:
            fac.free()


def _refused(cvs, case):
    for form in ac.FORMS:
        label = "%s, %s" % (case.what, form)
        fac = Kept(cvs)
        try:
            kernel = cvs.cvs_fir_last_kernel()
            cvs.cvs_clear_last_error()
            rc = case(fac, form)
            message = _lib.last_error()
            assert rc != 0, "%s: returned 0 on operands that share a buffer" % label
            assert case.entry in message and any(w in message for w in ac.WORDINGS), "%s: the message is %r" % (label, message)
            written = [o for o in fac.objects if o.out]
            assert written
            for o in written:
                assert o.frame.current_window.is_empty(), "%s: %s keeps the window %r" % (label, o.name, o.frame.current_window.tuple())
            for o, g in zip(fac.objects, fac.collect()):                              # (collect() waits for the stream first)
                assert np.array_equal(g, o.initial), "%s: %s was written: something was launched" % (label, o.name)
            assert cvs.cvs_fir_last_kernel() == kernel, "%s: cvs_fir_last_kernel() went from %d to %d" % (label, kernel, cvs.cvs_fir_last_kernel())
        finally:
            fac.free()


@pytest.mark.parametrize("gid", [g[0] for g in ac.GROUPS])
def test_operands_that_share_a_buffer(cvs, flavour, gid):
    build = dict(ac.GROUPS)[gid]
    try:
        for case, ref_case in zip(build(cvs), build(ac.Reference())):
            cvs.cvs_fir_path_override(ac.pin_of(case))
            if case.policy == ac.REFUSED:
                _refused(cvs, case)
            else:
                _in_place_or_shared(cvs, flavour, case, ref_case)
    finally:
        cvs.cvs_fir_path_override(_lib.FIR_PATH_AUTO)


# ------------------------------------------------------------------ a refusal leaves no trace

def _tap_lists(count, ntaps):
    """`count` different lists of `ntaps` taps"""
    base = ec._taps(ntaps)
    return [(base * np.float32(1.0 + 0.001 * k)).astype(np.float32) for k in range(count)]


def test_refusals_take_nothing_from_the_pool_and_pin_no_tap_table(cvs, flavour):
    """4 taps: the table kernels, whose legal call takes two cached tap tables; 15 taps of the unsharp mask and 13 of
    blur + Lanczos: legal calls that take a pooled f32 frame.  130 refused calls of each, every blur with a tap list of its
    own, take nothing: the pool's free bytes after a trim are what they were, and a legal blur then finds a slot for its
    tables and gives the reference's pixels."""
    full = (0, 0, 130, 40)
    host = ec.px16(np.random.default_rng(5100), full, (3, 2, 127, 37))
    shared = DeviceFrame.from_host(host)
    out = DeviceFrame.from_host(ec.blank(True, full))
    lists = _tap_lists(AXIS_CACHE + 2, 4)
    t15, t13 = ec._taps(15), ec._taps(13)
    try:
        _lib.check(cvs.cvs_stream_sync(None))
        cvs.cvs_pool_trim()
        before = _free_bytes(cvs)
        for taps in lists:
            assert cvs.cvs_fir_blur_f16_dev(shared.ref(), shared.ref(), f32p(taps), 4, None) != 0
            shared.c.current_window = host.c.current_window
            assert cvs.cvs_unsharp_mask_f16_dev(shared.ref(), shared.ref(), f32p(t15), 15, C.c_float(0.7), C.c_float(0.01), None) != 0
            shared.c.current_window = host.c.current_window
            assert cvs.cvs_blur_lanczos_f16_dev(shared.ref(), shared.ref(), f32p(t13), 13, C.c_float(0.4), C.c_float(0.35), 3, None) != 0
            shared.c.current_window = host.c.current_window
        _lib.check(cvs.cvs_stream_sync(None))
        cvs.cvs_pool_trim()
        after = _free_bytes(cvs)
        assert after == before, "%d bytes did not come back after %d refused calls" % (before - after, 3 * len(lists))
        assert np.array_equal(shared.download().array, host.array)
        # the legal call of the same entry, on distinct frames, at a tap list of its own
        taps = (ec._taps(4) * np.float32(0.9)).astype(np.float32)
        cvs.cvs_clear_last_error()
        rc = cvs.cvs_fir_blur_f16_dev(out.ref(), shared.ref(), f32p(taps), 4, None)
        assert rc == 0, _lib.last_error()
        _lib.check(cvs.cvs_stream_sync(None))
        with _oracle_flavour(flavour):
            want, src = ec.blank(True, full), host.copy()
            ac.Reference().cvs_fir_blur_f16_dev(want.ref(), src.ref(), f32p(taps), 4, None)
        assert same_window(out.current_window, want.current_window)
        assert np.array_equal(_canon(out.download().array.reshape(-1).view(np.uint8), "f16"), _canon(want.array.reshape(-1).view(np.uint8), "f16"))
    finally:
        shared.free()
        out.free()
        cvs.cvs_pool_trim()


def test_a_refusal_while_a_stream_is_capturing(cvs, flavour, stream):
    """The refused call returns nonzero and records nothing; the capture ends normally, and the graph -- with a legal call of
    the same entry recorded after the refused one -- replays to the reference's pixels."""
    full = (0, 0, 130, 40)
    host = ec.px16(np.random.default_rng(5200), full, (3, 2, 127, 37))
    blank = ec.blank(True, full)
    shared, out = DeviceFrame.from_host(host), DeviceFrame.from_host(blank)
    taps = ec._taps(9)
    graph = None

    def legal():
        return cvs.cvs_fir_blur_f16_dev(out.ref(), shared.ref(), f32p(taps), 9, stream)

    def both():
        refused = cvs.cvs_fir_blur_f16_dev(shared.ref(), shared.ref(), f32p(taps), 9, stream)
        message = _lib.last_error()
        window_empty = shared.current_window.is_empty()
        shared.c.current_window = host.c.current_window
        return refused, message, window_empty, legal()
    try:
        _lib.check(legal(), "the warm run")
        _lib.check(cvs.cvs_stream_sync(stream))
        out.upload(blank.array)
        (refused, message, window_empty, rc), graph = record(cvs, stream, both)
        assert graph, "cvs_graph_end gave no graph: %s" % _lib.last_error()
        assert refused != 0 and "cvs_fir_blur_f16_dev" in message and ac.WORDINGS[0] in message and window_empty, (refused, message, window_empty)
        assert rc == 0
        _lib.check(cvs.cvs_stream_sync(stream))
        assert np.array_equal(out.download().array, blank.array), "recording ran the legal call"
        _lib.check(cvs.cvs_graph_launch(graph, stream), "cvs_graph_launch")
        _lib.check(cvs.cvs_stream_sync(stream))
        with _oracle_flavour(flavour):
            want, src = ec.blank(True, full), host.copy()
            ac.Reference().cvs_fir_blur_f16_dev(want.ref(), src.ref(), f32p(taps), 9, None)
        assert same_window(out.current_window, want.current_window)
        assert np.array_equal(_canon(out.download().array.reshape(-1).view(np.uint8), "f16"), _canon(want.array.reshape(-1).view(np.uint8), "f16"))
        assert np.array_equal(shared.download().array, host.array), "the shared frame was written"
    finally:
        cvs.cvs_stream_sync(stream)
        if graph:
            cvs.cvs_graph_destroy(graph)
        shared.free()
        out.free()
