"""Every frame-taking cvs_*_dev entry point on windows taller or wider than a picture (DESIGN.md "Extents"; include/canvas_hip.h,
the extent contract beside the coordinate contract): every entry computes any non-empty window its coordinate bounds admit,
whatever its height and width.

Elsewhere in the suite the tallest window has 4320 rows and the widest 7680 columns.  Here one catalogue call
(tests/extent_cases.py) is made on frames packed into the guarded arena of tests/arena.py, all at residue 0, under both
poisons, at 65 535, 65 536 and 70 001 rows, at 70 001 and 131 073 columns, and at the row counts where a launcher's own
arithmetic changes: a launcher that mis-forms a row index writes into a guard and is reported by name.  The expectation is the
reference side's (tests/reference_library.py: the CPU oracle in the flavour of the run, or the numpy models), never another run
of the library; tests/test_extents_cpu.py proves it without a GPU.  The entries of the extension headers run at the lines of their
own launchers: the row-stream pair and the edges up to four million rows, the corner pin into the second band of its launcher.

Per case: return code 0, cvs_last_error() empty, every reported window the reference's, every output the reference's (code for
code, or canonical codes where the object's cmp says so; inside the reported window alone for extent_cases.WINDOW_ONLY -- the
scaler between half frames, the crossfade of halfs, the chain, blur + over, the workspace stack -- as tests/test_gpu_parity.py
compares them), the same bytes under both poisons, inputs and guards untouched, and
cvs_fir_fell_through_count() where it was: a fused kernel that failed to launch and was rescued by a slower one is a finding.

Both arithmetic flavours, set here as tests/test_placement_gpu.py does."""
import numpy as np
import pytest

import oracle
from canvas_amd import _lib
from tests import arena as ar
from tests import entry_cases as ec
from tests import extent_cases as xc
from tests import reference_library as rl
from tests.test_placement_gpu import Packed, _canon
from tests.util import same_window

pytestmark = pytest.mark.gpu

# groups whose reference is a numpy model, the same in both flavours: computed once from 2^19 rows on, where it takes seconds
MODELLED = ("field_conversions", "chroma_key", "matte", "transform", "lut3d", "deinterlace_adaptive", "temporal", "perspective", "ycc422", "ycc420")
_kept = {}              # case name -> its reference, from the first flavour that asks until the other one has; emptied with the module


@pytest.fixture(scope="module", params=["separate", "contracted"])
def flavour(request, cvs):
    before = cvs.cvs_set_arithmetic(_lib.ARITH_CONTRACTED if request.param == "contracted" else _lib.ARITH_SEPARATE)
    yield request.param
    cvs.cvs_set_arithmetic(before if before >= 0 else _lib.ARITH_SEPARATE)
    cvs.cvs_fir_path_override(_lib.FIR_PATH_AUTO)


@pytest.fixture(scope="module", autouse=True)
def _forget_references():
    """Whatever flavours were selected, no kept reference outlives the module."""
    yield
    _kept.clear()


def _reference(gid, flavour, what, ref_case, height):
    """-> [(class, bytes, row bytes, is output, cmp, name)], [window or None], [buffer] of the case on the reference side"""
    key = what if gid.split("[")[0] in MODELLED and height >= 1 << 19 else None
    if key is not None and key in _kept and _kept[key][0] != flavour:
        return _kept.pop(key)[1]
    with oracle.flavour("fma" if flavour == "contracted" else "gcc"):
        host = rl.OnHostWithBuffers(None)
        assert ref_case(host) == 0
    spec = [(o.cls, o.nbytes, o.row_bytes, o.out, o.cmp, o.name) for o in host.objects]
    windows = [o.frame.current_window if o.frame is not None else None for o in host.objects]
    out = (spec, windows, [(o.frame.array if o.frame is not None else o.array) if o.out else None for o in host.objects])
    if key is not None:
        _kept[key] = (flavour, out)
    return out


def _sentinel_rows(got, o):
    """The rows of a buffer that still hold the sentinel in some pixel."""
    sentinel = ec.SENT16 if o.cls == "f16" else ec.SENT32
    a = got.view(np.uint16 if o.cls == "f16" else np.float32).reshape(-1, o.row_bytes // (8 if o.cls == "f16" else 16), 4)
    return np.flatnonzero((a == sentinel).all(axis=2).any(axis=1))


def run_case(cvs, gid, flavour, what, case, ref_case, height):
    spec, want_windows, want = _reference(gid, flavour, what, ref_case, height)
    guard = ar.guard_bytes([s[2] for s in spec])
    arena = ar.Arena(cvs, ar.capacity_for([s[1] for s in spec], guard), guard)
    window_only = what.startswith(xc.WINDOW_ONLY)
    try:
        runs = {}
        for pname, poison in ar.POISONS:
            label = "%s, %s poison" % (what, pname)
            arena.fill(poison)
            fac = Packed(cvs, arena, (0,) * len(spec))
            fell = cvs.cvs_fir_fell_through_count()
            cvs.cvs_clear_last_error()
            rc = case(fac)
            got = fac.collect()
            assert [(o.cls, o.nbytes, o.row_bytes, o.out, o.cmp, o.name) for o in fac.objects] == spec, label + ": the case is not the reference's case"
            assert rc == 0, "%s: returned %r (%s)" % (label, rc, _lib.last_error())
            assert _lib.last_error() == "", "%s: returned 0 and left the message %r" % (label, _lib.last_error())
            assert cvs.cvs_fir_fell_through_count() == fell, "%s: a kernel did not launch and the next in line took the call" % label
            try:
                arena.check()
            except AssertionError as e:
                raise AssertionError("%s: %s" % (label, e))
            for o, ww in zip(fac.objects, want_windows):
                if ww is None:
                    continue
                w = o.frame.current_window
                assert same_window(w, ww), "%s: %s reports window %r, the reference %r" % (label, o.name, w.tuple(), ww.tuple())
            for o, g, w, ww in zip(fac.objects, got, want, want_windows):
                if not o.out:
                    continue
                a, b = _canon(g, o.cmp), _canon(w.reshape(-1).view(np.uint8), o.cmp)
                if window_only and ww is not None:
                    inside = np.zeros(w.shape, bool)
                    inside[ww.min.y:ww.max.y + 1, ww.min.x:ww.max.x + 1] = True         # (every buffer here starts at (0, 0))
                    a, b = a.reshape(-1)[inside.reshape(-1)], b.reshape(-1)[inside.reshape(-1)]
                if not np.array_equal(a, b):
                    bad = np.flatnonzero(a != b)
                    left = _sentinel_rows(g, o) if ww is not None and not o.reads else np.zeros(0, int)
                    inside_rows = left[(left >= ww.min.y) & (left <= ww.max.y)] if left.size else left
                    note = "; sentinel left in %d rows of the window, from row %d" % (inside_rows.size, inside_rows[0]) if inside_rows.size else ""
                    raise AssertionError("%s: %s differs from the reference in %d of %d elements, first at element %d: 0x%x, the reference 0x%x%s" % (
                        label, o.name, bad.size, a.size, bad[0], a[bad[0]], b[bad[0]], note))
            runs[pname] = (fac.objects, got)
        for o, a, b in zip(runs["nan"][0], runs["nan"][1], runs["finite"][1]):
            assert not o.out or np.array_equal(a, b), "%s: %s depends on what lies outside the buffers" % (what, o.name)
    finally:
        arena.free()


PAIRS = [(gid, pin, build, extent) for gid, pin, build, extents, _halo in xc.GROUPS for extent in extents]


@pytest.mark.parametrize("gid,pin,build,extent", PAIRS, ids=["%s-%dx%d" % (gid, e[0], e[1]) for gid, _p, _b, e in PAIRS])
def test_extent(cvs, flavour, gid, pin, build, extent):
    width, height = extent
    cvs.cvs_fir_path_override(pin)
    try:
        cases, ref_cases = build(cvs, width, height), build(rl.ReferenceLibrary(), width, height)
        assert cases
        for (what, case), (_, ref_case) in zip(cases, ref_cases):
            run_case(cvs, gid, flavour, what, case, ref_case, height)
    finally:
        cvs.cvs_fir_path_override(_lib.FIR_PATH_AUTO)
