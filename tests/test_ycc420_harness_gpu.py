"""The device entries of include/canvas_ycc420.h through the harnesses that run the catalogue of device-entry calls, with no
harness code of their own: the cases of tests/ycc420_cases.py on operands packed into a guarded arena at every placement
(tests/test_placement_gpu.py run_case: the 8-bit layouts' planes at any byte address, the 10-bit layouts' on residues that keep
their alignment but leave the 16-byte grid, the frame at 8 modulo 16, which sends the kernels down their sample-by-sample and
8-byte forms), recorded into a graph and replayed on the recorded and on other contents (tests/test_graph_replay_gpu.py run_case),
and far from the origin by the "anchored" rule of the DV and MPEG-2 cases (tests/test_far_windows_gpu.py: the raster stays at the
origin, so a frame far outside it comes back untouched with an empty window, and the planes are those of a frame without
pixels); then the frame operand bent one past the coordinate bound and onto INT_MIN / INT_MAX (refused, nothing written).  Both
arithmetic flavours."""
import pytest

from canvas_amd import _lib
from tests import entry_cases as ec
from tests import ycc420_cases as yc
from tests.test_entry_cases_cpu import HostOnly, Recorder
from tests.test_far_windows_gpu import Bent, _refused
from tests.test_far_windows_gpu import test_anchored_far_outside_the_raster as run_anchored
from tests.test_graph_replay_gpu import run_case as run_recorded
from tests.test_graph_replay_gpu import stream  # noqa: F401  (the module's stream fixture)
from tests.test_placement_gpu import run_case as run_packed

pytestmark = pytest.mark.gpu

GROUP_IDS = [g[0] for g in yc.GROUPS]


@pytest.fixture(scope="module", params=["separate", "contracted"])
def flavour(request, cvs):
    before = cvs.cvs_set_arithmetic(_lib.ARITH_CONTRACTED if request.param == "contracted" else _lib.ARITH_SEPARATE)
    yield request.param
    cvs.cvs_set_arithmetic(before if before >= 0 else _lib.ARITH_SEPARATE)


@pytest.mark.parametrize("gid,build", yc.GROUPS, ids=GROUP_IDS)
def test_packed_into_a_guarded_arena(cvs, flavour, gid, build):
    for what, case in build(cvs):
        run_packed(cvs, what, case)


@pytest.mark.parametrize("gid,build", yc.GROUPS, ids=GROUP_IDS)
def test_recorded_and_replayed(cvs, flavour, stream, gid, build):  # noqa: F811
    for what, case in build(cvs):
        run_recorded(cvs, stream, what, case)


@pytest.mark.parametrize("gid,build", yc.GROUPS, ids=GROUP_IDS)
def test_far_outside_the_raster(cvs, flavour, gid, build):
    assert yc.FAR_RULE is ec.FAR_CLASSES["mpeg2"][1] is ec.FAR_CLASSES["dv"][1]           # "anchored": no offsets of its own
    run_anchored(cvs, flavour, gid, _lib.FIR_PATH_AUTO, build)


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


@pytest.mark.parametrize("gid,build", yc.GROUPS, ids=GROUP_IDS)
def test_one_past_the_bound_is_refused(cvs, flavour, gid, build):
    lim = ec.MAX_COORD
    cases = build(cvs)
    picked = _first_case_of_each_entry(build)
    assert len(picked) == len(yc.ENTRIES)
    for extreme in (False, True):
        for k, is_frame, reads in picked:
            what, case = cases[k]
            frames = [i for i, f in enumerate(is_frame) if f]
            assert len(frames) == 1
            for index in frames:
                bends = [("full", "max", lim + 1), ("full", "min", -lim - 1)]
                if reads[index]:
                    bends += [("current", "max", lim + 1), ("current", "min", -lim - 1)]
                if extreme:
                    bends = [("full", "max", ec.INT_MAX), ("full", "min", ec.INT_MIN)] + ([("current", "max", ec.INT_MAX), ("current", "min", ec.INT_MIN)] if reads[index] else [])
                for which, side, value in bends:
                    _refused(cvs, "%s, operand %d, %s_window's %s on %d" % (what, index, which, side, value), case,
                             lambda twin: Bent(twin, index, which, side, value),
                             ("beyond", "no int holds") if which == "full" else ("beyond", "outside"))
