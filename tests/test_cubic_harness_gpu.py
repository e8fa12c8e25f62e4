"""The four warp entries with the Catmull-Rom filter through the harnesses that run the catalogue of device-entry calls, with no
harness code of their own: the cases of tests/cubic_cases.py on frames packed into a guarded arena at every placement
(tests/test_placement_gpu.py run_case), recorded into a graph and replayed on the recorded and on other contents
(tests/test_graph_replay_gpu.py run_case), far from the origin up to the corners of the coordinate bound -- the corner pin byte
for byte the origin's result (tests/test_far_windows_gpu.py run_equivariant: positions are formed from the map's two origins,
which move with the frames), the affine warp against tests/cubic_model.py at the same far arguments, inside the transform's own
bound -- and with every frame operand bent one past the bound and onto INT_MIN / INT_MAX (refused, nothing written).  Then what
the catalogues of tests/extent_cases.py and tests/alias_cases.py hold the two older filters to: windows taller and wider than a
picture, at that catalogue's extents, against the model, and the shared-buffer policy.  Both arithmetic flavours."""
import ctypes as C

import numpy as np
import pytest

from canvas_amd import _lib
from canvas_amd.abi import HostFrame
from canvas_amd.device import DeviceFrame
from tests import cubic_cases as sc
from tests import cubic_model as cm
from tests import entry_cases as ec
from tests import extent_cases as xc
from tests import perspective_model as pm
from tests import transform_model as tm
from tests.test_entry_cases_cpu import HostOnly, Recorder
from tests.test_far_windows_gpu import Bent, _far_runs, _origin, _refused, run_equivariant
from tests.test_graph_replay_gpu import _free_bytes, record
from tests.test_graph_replay_gpu import run_case as run_recorded
from tests.test_graph_replay_gpu import stream  # noqa: F401  (the module's stream fixture)
from tests.test_key_gpu import SENTINEL16, _same
from tests.test_placement_gpu import run_case as run_packed

pytestmark = pytest.mark.gpu

GROUP_IDS = [g[0] for g in sc.GROUPS]
CUBIC = _lib.TRANSFORM_CATMULL_ROM


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


def run_modelled(cvs, what, case, rule):
    """tests/test_far_windows_gpu.py run_transform with the Catmull-Rom model: the affine warp at the same far arguments"""
    _rc, _got, _windows, spec, boxes = _origin(cvs, case)
    offsets = ec.far_offsets(rule, boxes)
    assert len(offsets) >= 4, offsets
    for label, fac, rc, got in _far_runs(cvs, what, case, spec, offsets):
        source, target = fac.hosts
        half = source.dtype == np.uint16
        want, win = cm.transform_expected(target.array, target.full_window.tuple(), source.array, source.full_window.tuple(), source.current_window.tuple(),
                                          fac.matrices[0])
        assert rc == 0, "%s: %s" % (label, _lib.last_error())
        w = fac.objects[1].frame.current_window
        assert (None if w.is_empty() else w.tuple()) == win, "%s: window %r, the model's %r" % (label, w.tuple(), win)
        _same(got[1].view(source.dtype).reshape(want.shape), want, half, label)


@pytest.mark.parametrize("gid,build", sc.GROUPS, ids=GROUP_IDS)
def test_far_from_the_origin(cvs, flavour, gid, build):
    warp = sc.warp_of(gid)
    for what, case in build(cvs):
        (run_equivariant if warp == "perspective" else run_modelled)(cvs, what, case, sc.FAR_RULE[warp])


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
    assert len(picked) == 1
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

def _call(cvs, entry, params, tfull, source, sfull):
    """One call on f16 device frames, the target filled with a sentinel -> (return code, target buffer, window or None)"""
    before = np.broadcast_to(SENTINEL16, (tfull[3] - tfull[1] + 1, tfull[2] - tfull[0] + 1, 4)).copy()
    src = DeviceFrame.from_host(HostFrame(sfull, np.uint16, source, sfull))
    out = DeviceFrame.from_host(HostFrame(tfull, np.uint16, before))
    try:
        rc = entry(out.ref(), src.ref(), C.byref(params), None)
        _lib.check(cvs.cvs_stream_sync(None), "sync")
        got = out.download().array
        window = None if out.current_window.is_empty() else out.current_window.tuple()
    finally:
        src.free(); out.free()
        cvs.cvs_pool_trim()
    return rc, got, window


def test_a_window_of_131073_columns(cvs, flavour):
    """a row of more than 2^16 columns: 4097 tiles along x.  The affine warp under a half-pixel shift, the corner pin under the
    extent catalogue's own true perspective."""
    width, height = xc.WIDE[-1]
    assert (width, height) == (131073, 2)
    full = (0, 0, width - 1, height - 1)
    source = ec.px(np.random.default_rng(2901), True, full).array
    m = (1.0, 0.0, 0.5, 0.0, 1.0, 0.5)
    rc, got, window = _call(cvs, cvs.cvs_transform_f16_dev, _lib.transform(m, CUBIC), full, source, full)
    assert rc == 0 and window == full, _lib.last_error()
    _same(got, cm.transform_plane(source, full, m, full), True, "transform, 131073 columns")
    for near in (False, True):
        h, to, so, sfull = xc.pin_map(width, height, near)
        p = (tuple(float(np.float32(c)) for c in h), to, so)
        source = ec.px(np.random.default_rng(4300), True, sfull).array
        rc, got, window = _call(cvs, cvs.cvs_perspective_f16_dev, _lib.perspective(h, to, so, CUBIC), full, source, sfull)
        want_window = cm.perspective_target_window(p, sfull, full)
        assert rc == 0 and window == want_window == full, (_lib.last_error(), window, want_window)
        want = np.broadcast_to(SENTINEL16, got.shape).copy()
        cm.crop(want, full, window)[...] = cm.perspective_plane(source, sfull, p, window)
        _same(got, want, True, "perspective, 131073 columns, %s map" % ("near" if near else "far"))


def test_a_window_of_4194305_rows(cvs, flavour):
    """Eight bands of 65 535 rows of tiles and part of a ninth, two columns wide.  The affine warp shifts a source of 4099 rows
    repeated by half a pixel: the top and the bottom of the window are the model's, and every row between them equals the row
    4099 rows above it, as the model's does (a row depends on four source rows and on nothing else: (float)y + 0.5f is exact).
    The corner pin's window is the whole target, since S reaches the vanishing line 20 rows above the last row."""
    width, (_, height) = 2, xc.STREAM_ROWS[0]
    assert height == 4194305 and height > 8 * 65535 * 8
    period = 4099
    full = (0, 0, width - 1, height - 1)
    tile = ec.px(np.random.default_rng(2902), True, (0, 0, width - 1, period - 1)).array
    source = np.tile(tile, (-(-height // period), 1, 1))[:height]
    m = (1.0, 0.0, 0.5, 0.0, 1.0, 0.5)
    rc, got, window = _call(cvs, cvs.cvs_transform_f16_dev, _lib.transform(m, CUBIC), full, source, full)
    assert rc == 0 and window == full, _lib.last_error()
    top, bottom = (0, 0, width - 1, 2 * period - 1), (0, height - 2 * period, width - 1, height - 1)
    _same(cm.crop(got, full, top), cm.transform_plane(source, full, m, top), True, "transform, the first rows of 4194305")
    _same(cm.crop(got, full, bottom), cm.transform_plane(source, full, m, bottom), True, "transform, the last rows of 4194305")
    if not np.array_equal(got[period:height - 2 * period], got[2 * period:height - period]):
        rows = period + np.flatnonzero((got[period:height - 2 * period] != got[2 * period:height - period]).any(axis=(1, 2)))
        raise AssertionError("%d rows differ from the row %d rows below, from row %d to row %d" % (rows.size, period, rows[0], rows[-1]))
    del got, source

    # Under the extent catalogue's two maps every row samples the source, and the model walks some 400 000 pixels a second: it is
    # asked for the first and the last rows (the vanishing line is 20 rows above the last), the rows either side of every band's
    # first, and forty runs of a thousand rows anywhere.  Far from the line the `near` map keeps sampling the same four source rows
    # and the `far` map another place on every row (tests/extent_cases.py pin_map) ...
    band = xc.TRANSFORM_ROWS[0][1]
    assert band == 65535 * 8 and height // band == 8
    runs = [(0, 1999), (height - 4000, height - 1)] + [(k * band - 40, k * band + 40) for k in range(1, 9)]
    runs += [(int(y), int(y) + 999) for y in np.random.default_rng(2903).integers(0, height - 1000, 40)]
    for near in (True, False):
        h, to, so, sfull = xc.pin_map(width, height, near)
        p = (tuple(float(np.float32(c)) for c in h), to, so)
        source = ec.px(np.random.default_rng(4300), True, sfull).array
        params = _lib.perspective(h, to, so, CUBIC)
        rc, got, window = _call(cvs, cvs.cvs_perspective_f16_dev, params, full, source, sfull)
        assert rc == 0 and window == full == cm.perspective_target_window(p, sfull, full), (_lib.last_error(), window)
        drawn = 0
        for y0, y1 in runs:
            want = cm.perspective_plane(source, sfull, p, (0, y0, width - 1, y1))
            drawn += int(want.any(axis=(1, 2)).sum())
            _same(got[y0:y1 + 1], want, True, "perspective, %s map, rows %d to %d of 4194305" % ("near" if near else "far", y0, y1))
        assert drawn > (3000 if near else 30000) and not got[-20:].any(), drawn
        if near:
            assert got[-4000:-20].any()
            continue
        # ... and every row is held to the same entry on a target of one band's rows, which a single launch writes: a band is
        # the same kernel on a window that starts further down
        for y0 in range(0, height, band):
            part = (0, y0, width - 1, min(y0 + band, height) - 1)
            rc, piece, window = _call(cvs, cvs.cvs_perspective_f16_dev, params, part, source, sfull)
            assert rc == 0 and window == part, (_lib.last_error(), part, window)
            assert np.array_equal(piece, got[part[1]:part[3] + 1]), "perspective, 4194305 rows: rows %d to %d differ from those of a target of one band" % (part[1], part[3])


# ---------------------------------------------------------------- the shared-buffer policy

@pytest.mark.parametrize("warp", ["transform", "perspective"])
@pytest.mark.parametrize("half", [True, False], ids=["f16", "f32"])
def test_the_target_as_the_source_is_refused_and_leaves_no_trace(cvs, flavour, stream, half, warp):  # noqa: F811
    """One struct as both operands, and two structs over one buffer: nonzero, the entry named, the target's window empty, the
    buffer unchanged, nothing taken from the pool; refused while a stream is capturing, the capture goes on and the graph
    replays the legal call recorded after the refusal."""
    name = "cvs_%s_%s_dev" % (warp, "f16" if half else "f32")
    entry = getattr(cvs, name)
    struct = _lib.rgba_frame_f16 if half else _lib.rgba_frame_f32
    full, cur = (0, 0, 70, 40), (3, 2, 67, 37)
    host = ec.px(np.random.default_rng(5400), half, full, cur)
    blank = ec.blank(half, full)
    shared, out = DeviceFrame.from_host(host), DeviceFrame.from_host(blank)
    m = tm.from_parts(anchor=(35, 20), position=(35.25, 20), rotation=30.0)
    quad = pm.from_quad(pm.outer(cur), [(10.5, 2.0), (60.0, 4.5), (66.5, 38.0), (2.0, 33.5)])
    p = _lib.transform(m, CUBIC) if warp == "transform" else _lib.perspective(*quad, filter=CUBIC)
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
            assert rc != 0 and name in message and "not in place" in message and window_empty, (rc, message, window_empty)
        _lib.check(cvs.cvs_stream_sync(stream))
        cvs.cvs_pool_trim()
        assert _free_bytes(cvs) == before
        assert np.array_equal(shared.download().array.view(np.uint8), host.array.view(np.uint8)), "a refused call wrote"
        (refusals, rc), graph = record(cvs, stream, both)
        assert graph, "cvs_graph_end gave no graph: %s" % _lib.last_error()
        assert rc == 0 and all(r != 0 and name in msg and e for r, msg, e in refusals), (rc, refusals)
        _lib.check(cvs.cvs_stream_sync(stream))
        assert np.array_equal(out.download().array.view(np.uint8), blank.array.view(np.uint8)), "recording ran the legal call"
        _lib.check(cvs.cvs_graph_launch(graph, stream), "cvs_graph_launch")
        _lib.check(cvs.cvs_stream_sync(stream))
        if warp == "transform":
            want, window = cm.transform_expected(blank.array, full, host.array, full, cur, m)
        else:
            want, window = cm.perspective_expected(blank.array, full, host.array, full, cur, quad)
        assert out.current_window.tuple() == window
        _same(out.download().array, want, half, name)
        assert np.array_equal(shared.download().array.view(np.uint8), host.array.view(np.uint8))
    finally:
        if graph:
            cvs.cvs_graph_destroy(graph)
        shared.free()
        out.free()
        cvs.cvs_pool_trim()
