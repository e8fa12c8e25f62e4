"""The device entry of include/canvas_temporal.h through the harnesses that run the catalogue of device-entry calls, with no
harness code of its own: the cases of tests/temporal_cases.py on frames packed into a guarded arena at every placement
(tests/test_placement_gpu.py run_case; the placements put each operand in turn at 8 modulo 16, which sends the kernel down its
one-pixel form), recorded into a graph and replayed on the recorded and on other contents (tests/test_graph_replay_gpu.py
run_case), far from the origin up to the corners of the coordinate bound (tests/test_far_windows_gpu.py run_equivariant: byte for
byte the origin's result at ANY offset, since no row parity is involved here), and with every frame operand bent one past the
bound and onto INT_MIN / INT_MAX (refused, nothing written).  Then the shared-buffer policy: the output as any present input is
refused and leaves no trace.  Both arithmetic flavours."""
import ctypes as C

import numpy as np
import pytest

from canvas_amd import _lib
from canvas_amd.abi import HostFrame
from canvas_amd.device import DeviceFrame
from tests import entry_cases as ec
from tests import temporal_cases as sc
from tests import temporal_model as tm
from tests.test_entry_cases_cpu import HostOnly, Recorder
from tests.test_far_windows_gpu import Bent, _refused, run_equivariant
from tests.test_graph_replay_gpu import _free_bytes, record
from tests.test_graph_replay_gpu import run_case as run_recorded
from tests.test_graph_replay_gpu import stream  # noqa: F401  (the module's stream fixture)
from tests.test_placement_gpu import run_case as run_packed
from tests.util import canon_f16

pytestmark = pytest.mark.gpu

GROUP_IDS = [g[0] for g in sc.GROUPS]


@pytest.fixture(scope="module", params=["separate", "contracted"])
def flavour(request, cvs):
    before = cvs.cvs_set_arithmetic(_lib.ARITH_CONTRACTED if request.param == "contracted" else _lib.ARITH_SEPARATE)
    yield request.param
    cvs.cvs_set_arithmetic(before if before >= 0 else _lib.ARITH_SEPARATE)


@pytest.mark.parametrize("gid,build", sc.GROUPS, ids=GROUP_IDS)
def test_packed_into_a_guarded_arena(cvs, flavour, gid, build):
    for what, case in build(cvs):
        run_packed(cvs, what, case)


@pytest.mark.parametrize("gid,build", sc.GROUPS, ids=GROUP_IDS)
def test_recorded_and_replayed(cvs, flavour, stream, gid, build):  # noqa: F811
    for what, case in build(cvs):
        run_recorded(cvs, stream, what, case)


@pytest.mark.parametrize("gid,build", sc.GROUPS, ids=GROUP_IDS)
def test_far_from_the_origin(cvs, flavour, gid, build):
    for what, case in build(cvs):
        run_equivariant(cvs, what, case, sc.FAR_RULE)


def _first_case_of_each_entry(build):
    """(index, which operands are frames, which the call reads) of the first case that calls each entry, found on a stand-in"""
    rec, seen, picked = Recorder(), set(), []
    for k, (_what, case) in enumerate(build(rec)):
        before = len(rec.calls)
        fac = HostOnly(rec, 1)
        case(fac)
        names = {n for n, _ in rec.calls[before:]} - seen
        if names:
            seen |= names
            picked.append((k, [o.frame is not None for o in fac.objects], [o.reads for o in fac.objects]))
    return picked


@pytest.mark.parametrize("gid,build", sc.GROUPS, ids=GROUP_IDS)
def test_one_past_the_bound_is_refused(cvs, flavour, gid, build):
    lim = ec.MAX_COORD
    cases = build(cvs)
    picked = _first_case_of_each_entry(build)
    assert len(picked) == len(sc.ENTRIES) and len(picked[0][1]) == 6          # the first case hands in all six frames
    for extreme in (False, True):
        for k, is_frame, reads in picked:
            what, case = cases[k]
            for index in [i for i, f in enumerate(is_frame) if f]:
                bends = [("full", "max", lim + 1), ("full", "min", -lim - 1)]
                if reads[index]:
                    bends += [("current", "max", lim + 1), ("current", "min", -lim - 1)]
                if extreme:
                    bends = [("full", "max", ec.INT_MAX), ("full", "min", ec.INT_MIN)] + ([("current", "max", ec.INT_MAX), ("current", "min", ec.INT_MIN)] if reads[index] else [])
                for which, side, value in bends:
                    _refused(cvs, "%s, operand %d, %s_window's %s on %d" % (what, index, which, side, value), case,
                             lambda twin: Bent(twin, index, which, side, value),
                             ("beyond", "no int holds") if which == "full" else ("beyond", "outside"))


# ---------------------------------------------------------------- the shared-buffer policy

def test_the_output_as_a_present_input_is_refused_and_leaves_no_trace(cvs, orc, flavour, stream):  # noqa: F811
    """The output's own struct as each operand in turn, and another struct over the output's buffer: nonzero, the entry named,
    the output's window empty, the buffer unchanged, nothing taken from the pool; refused while a stream is capturing, the
    capture goes on and the graph replays the legal call recorded after the refusals."""
    name = "cvs_temporal_denoise_f16_dev"
    entry = getattr(cvs, name)
    full = (0, 0, 130, 20)
    codes = tm.sequence(np.random.default_rng(5400), full, sc.THRESHOLD, sc.SOFTNESS)
    hosts = [HostFrame(full, np.uint16, c, full) for c in codes]
    blank = ec.blank(True, full)
    frames, out = [DeviceFrame.from_host(h) for h in hosts], DeviceFrame.from_host(blank)
    shared = DeviceFrame.from_host(hosts[1])                              # the buffer that is handed in as the output and as one input
    p = _lib.temporal_denoise(sc.THRESHOLD, sc.SOFTNESS)
    graph = None

    def refused_calls():
        results = []
        for k in range(5):
            for second in (False, True):
                other = C.byref(_lib.rgba_frame_f16(shared.ptr, _lib.box2i.of(*full), _lib.box2i.of(*full))) if second else shared.ref()
                refs = [f.ref() for f in frames]
                refs[k] = other
                cvs.cvs_clear_last_error()
                rc = entry(shared.ref(), refs[0], refs[1], refs[2], refs[3], refs[4], C.byref(p), stream)
                results.append((rc, _lib.last_error(), shared.current_window.is_empty()))
                shared.c.current_window = hosts[1].c.current_window
        return results

    def both():
        return refused_calls(), entry(out.ref(), *[f.ref() for f in frames], C.byref(p), stream)
    try:
        _lib.check(cvs.cvs_stream_sync(None))
        cvs.cvs_pool_trim()
        before = _free_bytes(cvs)
        for rc, message, window_empty in refused_calls():
            assert rc != 0 and name in message and "cannot be one of the inputs" in message and window_empty, (rc, message, window_empty)
        _lib.check(cvs.cvs_stream_sync(stream))
        cvs.cvs_pool_trim()
        assert _free_bytes(cvs) == before
        assert np.array_equal(shared.download().array, hosts[1].array), "a refused call wrote"
        (refusals, rc), graph = record(cvs, stream, both)
        assert graph, "cvs_graph_end gave no graph: %s" % _lib.last_error()
        assert rc == 0 and all(r != 0 and name in m and e for r, m, e in refusals), (rc, refusals)
        _lib.check(cvs.cvs_stream_sync(stream))
        assert np.array_equal(out.download().array, blank.array), "recording ran the legal call"
        _lib.check(cvs.cvs_graph_launch(graph, stream), "cvs_graph_launch")
        _lib.check(cvs.cvs_stream_sync(stream))
        given = [(c, full, full) for c in codes]
        want, window, _exact, _w = tm.expected(blank.array, full, given[2], [given[1], given[3], given[0], given[4]], sc.THRESHOLD, sc.SOFTNESS, tm.ALL, orc.float_to_half)
        assert out.current_window.tuple() == window == full
        assert np.array_equal(canon_f16(out.download().array), canon_f16(want))
        for f, h in zip(frames, hosts):
            assert np.array_equal(f.download().array, h.array)
    finally:
        if graph:
            cvs.cvs_graph_destroy(graph)
        for f in frames + [out, shared]:
            f.free()
        cvs.cvs_pool_trim()
