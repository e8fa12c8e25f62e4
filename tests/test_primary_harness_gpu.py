"""The two device entries of include/canvas_primary.h through the harnesses that run the catalogue of device-entry calls, with no
harness code of their own: the cases of tests/primary_cases.py on frames and tables packed into a guarded arena at every
placement (tests/test_placement_gpu.py run_case), recorded into a graph and replayed on the recorded and on other contents
(tests/test_graph_replay_gpu.py run_case: the graph keeps the tables' pointers, the frames' contents change), far from the origin
up to the corners of the coordinate bound (tests/test_far_windows_gpu.py run_equivariant: byte for byte the origin's result at ANY
offset, since nothing here depends on coordinates), and with every frame operand bent one past the bound and onto INT_MIN /
INT_MAX (refused, nothing written).  Then windows wider and taller than a picture, against the numpy model.  Both arithmetic
flavours."""
import ctypes as C

import numpy as np
import pytest

from canvas_amd import _lib
from canvas_amd.abi import HostFrame
from canvas_amd.device import DeviceFrame
from tests import entry_cases as ec
from tests import primary_cases as sc
from tests import primary_model as pm
from tests.test_entry_cases_cpu import HostOnly, Recorder
from tests.test_far_windows_gpu import Bent, _refused, run_equivariant
from tests.test_graph_replay_gpu import run_case as run_recorded
from tests.test_graph_replay_gpu import stream  # noqa: F401  (the module's stream fixture)
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
    assert picked
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

def _run(cvs, full, codes, pre, matrix, post):
    """One f16 call over the whole of `full`, with device copies of the curves made for it -> the target's codes"""
    held = []

    def dev(cv):
        if cv is None:
            return None
        flat = cv.planar()
        ptr = cvs.cvs_malloc(flat.nbytes)
        assert ptr
        held.append(ptr)
        _lib.check(cvs.cvs_memcpy_h2d(ptr, flat.ctypes.data, flat.nbytes, None), "h2d")
        return ptr
    source = DeviceFrame.from_host(HostFrame(full, np.uint16, codes, full))
    target = DeviceFrame(full, np.uint16)
    try:
        p = _lib.primary((pre.size,) + pre.domain if pre else None, matrix, (post.size,) + post.domain if post else None)
        rc = cvs.cvs_primary_f16_dev(target.ref(), source.ref(), C.byref(p), dev(pre), dev(post), None)
        _lib.check(cvs.cvs_stream_sync(None), "sync")
        assert rc == 0 and target.current_window.tuple() == full, _lib.last_error()
        return target.download().array
    finally:
        source.free(); target.free()
        for ptr in held:
            cvs.cvs_free(ptr)


def test_a_window_of_131073_columns(cvs):
    """a row of more than 2^16 columns: 1025 one-wave blocks along x, two pixels a lane"""
    full = (0, 0, 131072, 2)
    pre, post = pm.distinct(1025, pm.SKEWED, 1), pm.distinct(17, pm.WIDE, 2)
    codes = pm.picture(np.random.default_rng(41), 131073, 3, True, 1025, pm.SKEWED)
    got = _run(cvs, full, codes, pre, sc.MATRIX, post)
    assert np.array_equal(ec_canon(got), ec_canon(pm.apply_pixels(codes, pre, sc.MATRIX, post)))


def test_a_window_of_4194305_rows(cvs):
    """the first row count past the row stream's grid fold (65 535 blocks of 64 rows): the launcher makes the segments longer, and
    the persistent workgroups walk more blocks than there are waves.  One column, a tile of 4099 rows repeated: the pass is
    pixelwise, so the model of the picture is the model of the tile, repeated."""
    height, period = 4194305, 4099
    pre = pm.distinct(4097, pm.SKEWED, 1)
    tile = pm.picture(np.random.default_rng(42), 1, period, True, 4097, pm.SKEWED)
    codes = np.tile(tile, (-(-height // period), 1, 1))[:height]
    full = (0, 0, 0, height - 1)
    got = _run(cvs, full, codes, pre, None, None)
    want = np.tile(pm.apply_pixels(tile, pre), (-(-height // period), 1, 1))[:height]
    if not np.array_equal(ec_canon(got), ec_canon(want)):
        rows = np.flatnonzero((ec_canon(got) != ec_canon(want)).any(axis=(1, 2)))
        raise AssertionError("%d rows differ, from row %d to row %d" % (rows.size, rows[0], rows[-1]))


def ec_canon(codes):
    from tests.util import canon_f16
    return canon_f16(codes).reshape(codes.shape)
