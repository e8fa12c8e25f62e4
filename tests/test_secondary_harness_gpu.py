"""The four device entries of include/canvas_secondary.h through the harnesses that run the catalogue of device-entry calls, with
no harness code of their own: the cases of tests/secondary_cases.py on frames packed into a guarded arena at every placement
(tests/test_placement_gpu.py run_case), recorded into a graph and replayed on the recorded and on other contents
(tests/test_graph_replay_gpu.py run_case), far from the origin up to the corners of the coordinate bound
(tests/test_far_windows_gpu.py run_equivariant: byte for byte the origin's result at ANY offset, since nothing here depends on
coordinates), and with every frame operand bent one past the bound and onto INT_MIN / INT_MAX (refused, nothing written).  Then
windows wider and taller than a picture, against the numpy model.  Both arithmetic flavours."""
import ctypes as C

import numpy as np
import pytest

from canvas_amd import _lib
from canvas_amd.abi import HostFrame
from canvas_amd.device import DeviceFrame
from tests import entry_cases as ec
from tests import secondary_cases as sc
from tests import secondary_model as sm
from tests.test_entry_cases_cpu import HostOnly, Recorder
from tests.test_far_windows_gpu import Bent, _refused, run_equivariant
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
    assert picked and len(picked[0][1]) == (3 if gid.startswith("qualify") else 4)       # every frame operand of the entry
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

def _canon(codes):
    return canon_f16(codes).reshape(codes.shape)


def _run(cvs, full, a, b, m, q=None, mix=None):
    """One f16 call over the whole of `full`: the qualifier q on source a with the key frame b, or the mix (luma, invert) of a and
    b through m -> the target's codes"""
    frames = [DeviceFrame.from_host(HostFrame(full, np.uint16, codes, full)) for codes in (a, b, m) if codes is not None]
    target = DeviceFrame(full, np.uint16)
    try:
        if q is not None:
            p = sc.params(q)
            rc = cvs.cvs_qualify_f16_dev(target.ref(), frames[0].ref(), frames[1].ref(), C.byref(p), None)
        else:
            p = _lib.matte_mix(*mix)
            rc = cvs.cvs_matte_mix_f16_dev(target.ref(), frames[0].ref(), frames[1].ref(), frames[2].ref(), C.byref(p), None)
        _lib.check(cvs.cvs_stream_sync(None), "sync")
        assert rc == 0 and target.current_window.tuple() == full, _lib.last_error()
        return target.download().array
    finally:
        target.free()
        for f in frames:
            f.free()


def _pictures(seed, width, height, count):
    rng = np.random.default_rng(seed)
    return [sc.picture(rng, True, (0, 0, width - 1, height - 1)).array for _ in range(count)]


def test_a_window_of_131073_columns(cvs):
    """a row of more than 2^16 columns: 1025 one-wave blocks along x, two pixels a lane"""
    full = (0, 0, 131072, 2)
    a, b, m = _pictures(51, 131073, 3, 3)
    q = sc.QUALIFIERS[7]
    assert np.array_equal(_canon(_run(cvs, full, a, b, None, q=q)), _canon(sm.qualify_pixels(a, b, q)))
    assert np.array_equal(_canon(_run(cvs, full, a, b, m, mix=(True, False))), _canon(sm.mix_pixels(a, b, m, True, False)))


def test_a_window_of_4194305_rows(cvs):
    """the first row count past the row stream's grid fold (65 535 blocks of 64 rows): the launcher makes the segments longer.
    One column, a tile of 4099 rows repeated: the passes are pixelwise, so the model of the picture is the model of the tile,
    repeated."""
    height, period = 4194305, 4099
    tiles = _pictures(52, 1, period, 3)
    a, b, m = (np.tile(t, (-(-height // period), 1, 1))[:height] for t in tiles)
    full = (0, 0, 0, height - 1)
    q = sc.QUALIFIERS[8]
    for got, tile in ((_run(cvs, full, a, b, None, q=q), sm.qualify_pixels(tiles[0], tiles[1], q)),
                      (_run(cvs, full, a, b, m, mix=(False, True)), sm.mix_pixels(tiles[0], tiles[1], tiles[2], False, True))):
        want = np.tile(tile, (-(-height // period), 1, 1))[:height]
        if not np.array_equal(_canon(got), _canon(want)):
            rows = np.flatnonzero((_canon(got) != _canon(want)).any(axis=(1, 2)))
            raise AssertionError("%d rows differ, from row %d to row %d" % (rows.size, rows[0], rows[-1]))
