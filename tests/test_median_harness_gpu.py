"""The device entries of include/canvas_median.h through the harnesses that run the catalogue of device-entry calls, with no
harness code of their own: the cases of tests/median_cases.py on frames packed into a guarded arena at every placement
(tests/test_placement_gpu.py run_case), recorded into a graph and replayed on the recorded and on other contents
(tests/test_graph_replay_gpu.py run_case), far from the origin up to the corners of the coordinate bound
(tests/test_far_windows_gpu.py run_equivariant: byte for byte the origin's result at ANY offset, since nothing in a median
depends on coordinates), and with every frame operand bent one past the bound and onto INT_MIN / INT_MAX (refused, nothing
written).  Then the two things the catalogues of tests/extent_cases.py and tests/alias_cases.py hold the other entries to, which
the reference side of those harnesses has no median for: windows wider and taller than a picture, against the numpy model, and
the shared-buffer policy -- the target as the source is refused and leaves no trace.  Both arithmetic flavours."""
import ctypes as C

import numpy as np
import pytest

from canvas_amd import _lib
from canvas_amd.device import DeviceFrame
from tests import entry_cases as ec
from tests import median_cases as sc
from tests import median_model as mm
from tests.test_entry_cases_cpu import HostOnly, Recorder
from tests.test_far_windows_gpu import Bent, _refused, run_equivariant
from tests.test_graph_replay_gpu import _free_bytes, record
from tests.test_graph_replay_gpu import run_case as run_recorded
from tests.test_graph_replay_gpu import stream  # noqa: F401  (the module's stream fixture)
from tests.test_median_gpu import run
from tests.test_placement_gpu import run_case as run_packed

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
    assert len(picked) == len(sc.ENTRIES)
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


# ---------------------------------------------------------------- extents

def test_a_window_of_131073_columns(cvs):
    """a row of more than 2^16 columns: 1058 workgroups along x"""
    cw = (0, 0, 131072, 2)
    bits = mm.speck_picture(np.random.default_rng(31), 131073, 3)
    (rc, got, window), before = run(cvs, (0, 0, 131073, 2), (np.concatenate([bits, bits[:, :1]], axis=1), (0, 0, 131073, 2), cw), _lib.median(2, mm.THRESHOLD))
    assert rc == 0 and window == cw, _lib.last_error()
    want = before.copy()
    want[:, :131073] = mm.filter_pixels(bits, 2, mm.THRESHOLD)
    assert np.array_equal(got, want)


def test_a_window_of_4194305_rows(cvs):
    """the first row count past the row stream's grid fold (65 535 workgroups of 64 rows): the launcher makes the segments longer.
    Three columns of a tile of 4099 rows repeated, so that the model is the tile's (tests/median_model.py filter_tiled)."""
    height, period = 4194305, 4099
    tile = mm.speck_picture(np.random.default_rng(32), 3, period)
    bits = np.tile(tile, (-(-height // period), 1, 1))[:height]
    full = (0, 0, 2, height - 1)
    (rc, got, window), _ = run(cvs, full, (bits, full, full), _lib.median(1, mm.THRESHOLD, _lib.MEDIAN_A))
    assert rc == 0 and window == full, _lib.last_error()
    want = mm.filter_tiled(tile, height, 1, mm.THRESHOLD, "a")
    if not np.array_equal(got, want):
        rows = np.flatnonzero((got != want).any(axis=(1, 2)))
        raise AssertionError("%d rows differ, from row %d to row %d" % (rows.size, rows[0], rows[-1]))


# ---------------------------------------------------------------- the shared-buffer policy

@pytest.mark.parametrize("half", [True, False], ids=["f16", "f32"])
def test_the_target_as_the_source_is_refused_and_leaves_no_trace(cvs, flavour, stream, half):  # noqa: F811
    """One struct as both operands, and two structs over one buffer: nonzero, the entry named, the target's window empty, the
    buffer unchanged, nothing taken from the pool; refused while a stream is capturing, the capture goes on and the graph
    replays the legal call recorded after the refusal.  (Two targets over disjoint windows of one buffer are no case here: the
    entry has one input.)"""
    name = "cvs_median_f16_dev" if half else "cvs_median_f32_dev"
    entry = getattr(cvs, name)
    struct = _lib.rgba_frame_f16 if half else _lib.rgba_frame_f32
    full, cur = (0, 0, 130, 40), (3, 2, 127, 37)
    host = sc.source(np.random.default_rng(5300), half, full, cur)
    blank = ec.blank(half, full)
    shared, out = DeviceFrame.from_host(host), DeviceFrame.from_host(blank)
    p = _lib.median(2, mm.THRESHOLD)
    graph = None

    def refused_calls():
        results = []
        for second in (False, True):
            source = C.byref(struct(shared.ptr, _lib.box2i.of(*full), _lib.box2i.of(*cur))) if second else shared.ref()
            cvs.cvs_clear_last_error()
            rc = entry(shared.ref(), source, C.byref(p), stream)
            results.append((rc, _lib.last_error(), shared.current_window.is_empty()))
            shared.c.current_window = host.c.current_window
        return results

    def both():
        return refused_calls(), entry(out.ref(), shared.ref(), C.byref(p), stream)
    try:
        _lib.check(cvs.cvs_stream_sync(None))
        cvs.cvs_pool_trim()
        before = _free_bytes(cvs)
        for rc, message, window_empty in refused_calls():
            assert rc != 0 and name in message and "cannot be the source" in message and window_empty, (rc, message, window_empty)
        _lib.check(cvs.cvs_stream_sync(stream))
        cvs.cvs_pool_trim()
        assert _free_bytes(cvs) == before
        assert np.array_equal(shared.download().array.view(np.uint8), host.array.view(np.uint8)), "a refused call wrote"
        (refusals, rc), graph = record(cvs, stream, both)
        assert graph, "cvs_graph_end gave no graph: %s" % _lib.last_error()
        assert rc == 0 and all(r != 0 and name in m and e for r, m, e in refusals), (rc, refusals)
        _lib.check(cvs.cvs_stream_sync(stream))
        assert np.array_equal(out.download().array.view(np.uint8), blank.array.view(np.uint8)), "recording ran the legal call"
        _lib.check(cvs.cvs_graph_launch(graph, stream), "cvs_graph_launch")
        _lib.check(cvs.cvs_stream_sync(stream))
        dtype = np.uint16 if half else np.uint32
        want, window = mm.expected(blank.array.view(dtype), full, host.array.view(dtype), full, cur, 2, mm.THRESHOLD)
        assert out.current_window.tuple() == window == cur
        assert np.array_equal(out.download().array.view(dtype), want)
        assert np.array_equal(shared.download().array.view(np.uint8), host.array.view(np.uint8))
    finally:
        if graph:
            cvs.cvs_graph_destroy(graph)
        shared.free()
        out.free()
        cvs.cvs_pool_trim()
