"""Every windowed cvs_*_dev entry point on frames far from the origin (DESIGN.md "Coordinates"; include/canvas_hip.h, the
coordinate contract beside the frame structs).

Elsewhere in the suite a frame lies within a few hundred pixels of (0, 0), where every coordinate is exact in a float, in 16
bits and in any sum a kernel forms.  Here one catalogue call (tests/entry_cases.py) is made at the origin on frames with
allocations of their own (the twin, which the other GPU tests tie to the oracle and the models) and again with every operand
translated (entry_cases.Shifted) onto frames packed into the guarded arena of tests/arena.py, all at residue 0, under both
poisons: across the 16-bit lines, past 2^24, and with the case's bounding box on either corner of the bound.

  equivariant groups   return code, every reported window translated back, every output buffer whole (code for code, or through
                       canon_f16 / canon_f32 per the object's cmp) equal to the twin's; identical bytes under the two poisons;
                       every guard byte; every input.  The field conversions and the weave move by an even dy (row parity is that
                       of the absolute coordinate); the bilinear scaler runs at factor 2.0 and the Lanczos resamplers at 0.5 inside
                       +-RESAMPLE_MAX_COORD, where every position they form in float is exact, the Lanczos source moved by twice
                       the target's offset.
  modelled groups      the transform, against tests/transform_model.py at the same far arguments, inside
                       +-TRANSFORM_MAX_COORD; the field conversions at an odd dy, which swaps the fields, against
                       tests/fields_model.py, and the weave at an odd dy against the oracle.  The resamplers at the other
                       factors (and the bilinear scaler at 0.5) in every form -- f32 and f16, single and batch, blur + Lanczos
                       and config 3 -- against the oracle's build of the flavour (entry_cases.MODELLED_CASES).
  anchored groups      DV and MPEG-2: a frame far outside the raster gives an untouched frame with an empty window, or the planes
                       of a frame without pixels.
  refusals             one past the bound on a minimum and on a maximum, on full_window, current_window and a point: -1, a
                       message, empty output windows, every byte of every operand as uploaded -- and only then INT_MAX / INT_MIN.

Both arithmetic flavours, set here as tests/test_placement_gpu.py does."""
import ctypes as C

import numpy as np
import pytest

from canvas_amd import _lib
from canvas_amd.abi import HostFrame, box2i, v2f
from tests import arena as ar
from tests import entry_cases as ec
from tests import fields_model as fm
from tests import transform_model as tm
from tests.entry_cases import Shifted, Twin
from tests.test_entry_cases_cpu import HostOnly, Recorder
from tests.test_far_windows_cpu import OnHost, OracleAsLibrary
from tests.test_fields_gpu import _compare, _rows_mask
from tests.test_key_gpu import _same
from tests.test_placement_gpu import Packed, _canon
from tests.util import same_window

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["separate", "contracted"])
def flavour(request, cvs):
    before = cvs.cvs_set_arithmetic(_lib.ARITH_CONTRACTED if request.param == "contracted" else _lib.ARITH_SEPARATE)
    yield request.param
    cvs.cvs_set_arithmetic(before if before >= 0 else _lib.ARITH_SEPARATE)
    cvs.cvs_fir_path_override(_lib.FIR_PATH_AUTO)


def _prefix(gid):
    return gid.split("[")[0]


def _groups(classes):
    return [g for g in ec.GROUPS if ec.FAR_CLASSES[_prefix(g[0])][0] in classes]


def _origin(cvs, case):
    """The twin's run: return code, buffers, windows, what the objects are, and every frame's (is output, full window)."""
    twin = Twin(cvs)
    probe = Shifted(twin, (0, 0))
    try:
        rc = case(probe)
        got = twin.collect()
        windows = probe.windows_back()
        spec = [(o.cls, o.nbytes, o.row_bytes, o.out, o.cmp) for o in twin.objects]
        boxes = [(o.out, h.full_window.tuple()) for o, h in zip(twin.objects, probe.hosts) if h is not None]
    finally:
        twin.free()
    return rc, got, windows, spec, boxes


def _far_runs(cvs, what, case, spec, offsets):
    """The case through Shifted(Packed(arena)) at every offset under both poisons -> yields (label, fac, rc, {poison: buffers})
    after the checks no expectation is needed for: the case is the same case, guards and inputs intact, poisons agree."""
    guard = ar.guard_bytes([s[2] for s in spec])
    arena = ar.Arena(cvs, ar.capacity_for([s[1] for s in spec], guard), guard)
    try:
        for name, d, s in offsets:
            runs, last = {}, None
            for pname, poison in ar.POISONS:
                label = "%s, %s: target moved by %r, source by %r, %s poison" % (what, name, d, s, pname)
                arena.fill(poison)
                inner = Packed(cvs, arena, (0,) * len(spec))
                fac = Shifted(inner, d, s)
                rc = case(fac)
                got = inner.collect()
                assert [(o.cls, o.nbytes, o.row_bytes, o.out, o.cmp) for o in inner.objects] == spec, label + ": the case is not the same case"
                try:
                    arena.check()
                except AssertionError as e:
                    raise AssertionError("%s: %s" % (label, e))
                if last is not None:
                    assert rc == last[1] and all(same_window(a, b) for a, b in zip(fac.windows_back(), last[0].windows_back()) if a is not None), label
                runs[pname], last = got, (fac, rc)
            for o, a, b in zip(fac.objects, runs["nan"], runs["finite"]):
                assert not o.out or np.array_equal(a, b), "%s, %s: %s depends on what lies outside the buffers" % (what, name, o.name)
            yield "%s, %s: target moved by %r, source by %r" % (what, name, d, s), fac, rc, runs["finite"]
    finally:
        arena.free()


def run_equivariant(cvs, what, case, rule):
    want_rc, want, want_windows, spec, boxes = _origin(cvs, case)
    offsets = ec.far_offsets(rule, boxes)
    assert len(offsets) >= 4, offsets
    for label, fac, rc, got in _far_runs(cvs, what, case, spec, offsets):
        assert rc == want_rc, "%s: returned %r, at the origin %r (%s)" % (label, rc, want_rc, _lib.last_error())
        for o, w, ww in zip(fac.objects, fac.windows_back(), want_windows):
            assert w is None or same_window(w, ww), "%s: %s reports window %r (translated back), at the origin %r" % (label, o.name, w.tuple(), ww.tuple())
        for o, g, w in zip(fac.objects, got, want):
            if not o.out:
                continue
            a, b = _canon(g, o.cmp), _canon(w, o.cmp)
            if not np.array_equal(a, b):
                bad = np.flatnonzero(a != b)
                raise AssertionError("%s: %s differs from the origin's in %d of %d elements, first at element %d: 0x%x, at the origin 0x%x" % (
                    label, o.name, bad.size, a.size, bad[0], a[bad[0]], b[bad[0]]))


def _run_group(cvs, gid, pin, build, cls, runner):
    cvs.cvs_fir_path_override(pin)
    ran = 0
    try:
        for what, case in build(cvs):
            c, rule = ec.far_class(gid, what)
            if c == cls:
                runner(cvs, what, case, rule)
                ran += 1
    finally:
        cvs.cvs_fir_path_override(_lib.FIR_PATH_AUTO)
    return ran


EQUIVARIANT = _groups(["equivariant"])
# (the groups all of whose cases are modelled have nothing to run here)
ALL_MODELLED = {"lanczos_resample[%s-%dx%d-%s]" % (pin, s[0][0], s[0][1], s[2]) for pin in ec.LANCZOS_PINS for s in ec.LANCZOS_SHAPES if s[2:] != (0.5, 0.5)} | \
               {"scale_bilinear[%s-%d]" % (h, k) for h in ("f16", "f32") for k, c in enumerate(ec.SCALE_CASES) if c[0] != (2.0, 2.0)}


@pytest.mark.parametrize("gid,pin,build", [g for g in EQUIVARIANT if g[0] not in ALL_MODELLED], ids=[g[0] for g in EQUIVARIANT if g[0] not in ALL_MODELLED])
def test_equivariant(cvs, flavour, gid, pin, build):
    assert _run_group(cvs, gid, pin, build, "equivariant", run_equivariant) > 0


# ------------------------------------------------------------------ modelled: the transform at the same far arguments

def run_transform(cvs, what, case, rule):
    filt = tm.BILINEAR if "bilinear" in what else tm.NEAREST
    _rc, _got, _windows, spec, boxes = _origin(cvs, case)
    offsets = ec.far_offsets(rule, boxes)
    assert len(offsets) >= 4, offsets
    for label, fac, rc, got in _far_runs(cvs, what, case, spec, offsets):
        source, target = fac.hosts
        half = source.dtype == np.uint16
        want, win = tm.expected(target.array, target.full_window.tuple(), source.array, source.full_window.tuple(), source.current_window.tuple(),
                                fac.matrices[0], filt)
        assert rc == 0, "%s: %s" % (label, _lib.last_error())
        w = fac.objects[1].frame.current_window
        assert (None if w.is_empty() else w.tuple()) == win, "%s: window %r, the model's %r" % (label, w.tuple(), win)
        _same(got[1].view(source.dtype).reshape(want.shape), want, half, label)


MODELLED = _groups(["modelled"])                  # (the transform: the one group every case of which is modelled)


@pytest.mark.parametrize("gid,pin,build", MODELLED, ids=[g[0] for g in MODELLED])
def test_modelled_transform(cvs, flavour, gid, pin, build):
    assert _prefix(gid) == "transform"
    assert _run_group(cvs, gid, pin, build, "modelled", run_transform) > 0


# ------------------------------------------------------------------ modelled: the field conversions at an odd dy

def _triple(h):
    return (h.array, h.full_window.tuple(), None if h.current_window.is_empty() else h.current_window.tuple())


def run_fields_at_odd_dy(cvs, what, case, rule, op):
    """An odd dy swaps the fields: the expectation is tests/fields_model.py at the far arguments, compared as
    tests/test_fields_gpu.py compares (copied rows code for code, computed rows through canon_f16)."""
    import oracle
    _rc, _got, _windows, spec, boxes = _origin(cvs, case)
    offsets = ec.odd_dy_offsets(rule, boxes)
    assert len(offsets) >= 4 and all(d[1] % 2 for _n, d, _s in offsets)
    for label, fac, rc, got in _far_runs(cvs, what, case, spec, offsets):
        assert rc == 0, "%s: %s" % (label, _lib.last_error())
        target = fac.hosts[-1]
        tfull = target.full_window.tuple()
        if op == "interlace":
            want, win = fm.expected_interlace(target.array, tfull, _triple(fac.hosts[0]), _triple(fac.hosts[1]))
            exact = lambda y: True
        elif op == "soften":
            want, win = fm.expected_one_input(target.array, tfull, _triple(fac.hosts[0]), lambda cur, y0: fm.soften(cur, oracle.float_to_half))
            exact = lambda y: False
        else:
            field = int(op[-1])
            want, win = fm.expected_one_input(target.array, tfull, _triple(fac.hosts[0]), lambda cur, y0: fm.field_to_frame(cur, y0, field, oracle.float_to_half))
            exact = lambda y: (y & 1) == field
        w = fac.objects[-1].frame.current_window
        assert (None if w.is_empty() else w.tuple()) == win, "%s: window %r, the model's %r" % (label, w.tuple(), win)
        _compare(got[-1].view(np.uint16).reshape(want.shape), want, _rows_mask(tfull, win, exact), label)


@pytest.mark.parametrize("width", ec.STREAM_WIDTHS)
@pytest.mark.parametrize("op", ec.FIELD_OPS)
def test_modelled_field_conversions_at_an_odd_dy(cvs, flavour, op, width):
    gid = "field_conversions[%s-%d]" % (op, width)
    rule = ec.FAR_CLASSES["field_conversions"][1]
    for what, case in ec.field_conversions(cvs, op, width):
        run_fields_at_odd_dy(cvs, what, case, rule, op)


# ------------------------------------------------------------------ modelled: the resamplers and the weave against the oracle

def run_against_the_oracle(cvs, flavour, what, case, oracle_case, offsets, window_only=False):
    """The expectation is the oracle's at the same far arguments, in the flavour's build, compared as
    tests/test_gpu_parity.py compares: windows, then canonical codes -- of the whole buffer, or (window_only: the scaler
    between half frames, test_scale_bilinear_f16_twin) of the reported window."""
    import oracle
    _rc, _got, _windows, spec, _boxes = _origin(cvs, case)
    assert len(offsets) >= 4, offsets
    for label, fac, rc, got in _far_runs(cvs, what, case, spec, offsets):
        assert rc == 0, "%s: %s" % (label, _lib.last_error())
        with oracle.flavour("fma" if flavour == "contracted" else "gcc"):
            host = OnHost(OracleAsLibrary())
            model = Shifted(host, fac.offset, fac.source_offset)
            assert oracle_case(model) == 0
        for o, g, m in zip(fac.objects, got, host.objects):
            if not o.out:
                continue
            w, full = m.frame.current_window, m.frame.full_window
            assert same_window(o.frame.current_window, w), "%s: %s reports window %r, the oracle %r" % (label, o.name, o.frame.current_window.tuple(), w.tuple())
            a, b = _canon(g, o.cmp), _canon(m.frame.array.reshape(-1).view(np.uint8), o.cmp)
            if window_only:
                inside = np.zeros(m.frame.array.shape, bool)
                if not w.is_empty():
                    inside[w.min.y - full.min.y:w.max.y - full.min.y + 1, w.min.x - full.min.x:w.max.x - full.min.x + 1] = True
                a, b = a.reshape(-1)[inside.reshape(-1)], b.reshape(-1)[inside.reshape(-1)]
            if not np.array_equal(a, b):
                bad = np.flatnonzero(a != b)
                raise AssertionError("%s: %s differs from the oracle's in %d of %d elements, first at element %d: 0x%x, the oracle 0x%x" % (
                    label, o.name, bad.size, a.size, bad[0], a[bad[0]], b[bad[0]]))


WITH_MODELLED_RESAMPLERS = [g for g in ec.GROUPS if _prefix(g[0]) in {m[0] for m in ec.MODELLED_CASES}
                            and any(ec.far_class(g[0], what)[0] == "modelled" for what, _ in g[2](None))]


@pytest.mark.parametrize("gid,pin,build", WITH_MODELLED_RESAMPLERS, ids=[g[0] for g in WITH_MODELLED_RESAMPLERS])
def test_modelled_resamplers(cvs, flavour, gid, pin, build):
    """Every case of entry_cases.MODELLED_CASES in every form -- f32 and f16, single and batch: the bilinear scaler (its points
    move with the frames, so everything moves by one offset) and Lanczos, blur + Lanczos and config 3 (no points: offsets
    that line the far source up with the far target, entry_cases.lined_up)."""
    ran = 0
    cvs.cvs_fir_path_override(pin)
    try:
        for (what, case), (_, oracle_case) in zip(build(cvs), build(OracleAsLibrary())):
            if ec.far_class(gid, what)[0] != "modelled":
                continue
            _rc, _got, _windows, _spec, boxes = _origin(cvs, case)
            run_against_the_oracle(cvs, flavour, what, case, oracle_case, ec.far_offsets_for(gid, what, boxes),
                                   window_only=_prefix(gid) == "scale_bilinear" and " f16 " in what)
            ran += 1
    finally:
        cvs.cvs_fir_path_override(_lib.FIR_PATH_AUTO)
    assert ran > 0


def test_modelled_weave_at_an_odd_dy(cvs, flavour):
    """An odd dy swaps which rows the weave replaces: the oracle's weave at the same far arguments (dx stays 0), whole buffer,
    code for code, as tests/test_gpu_parity.py test_weave_fields compares."""
    rule = ec.FAR_CLASSES["weave_fields"][1]
    for (what, case), (_, oracle_case) in zip(ec.weave_fields(cvs), ec.weave_fields(OracleAsLibrary())):
        _rc, _got, _windows, _spec, boxes = _origin(cvs, case)
        offsets = ec.odd_dy_offsets(rule, boxes)
        assert all(d[0] == 0 and d[1] % 2 for _n, d, _s in offsets)
        run_against_the_oracle(cvs, flavour, what, case, oracle_case, offsets)


# ------------------------------------------------------------------ anchored: far outside the raster

class NoPixels(Shifted):
    """Every input frame with an empty current window, where it was."""

    def frame(self, host, out=False, **kw):
        if not out:
            host = HostFrame(host.full_window.tuple(), host.dtype, host.array, (0, 0, -1, -1))
        return Shifted.frame(self, host, out=out, **kw)


ANCHORED = _groups(["anchored"])
FAR_FROM_THE_RASTER = [("past 2^24", (2 ** 24 + 1, -2 ** 24 - 2)), ("near the top corner", (ec.MAX_COORD - 1024, ec.MAX_COORD - 1024)),
                       ("near the bottom corner", (-ec.MAX_COORD + 1024, -ec.MAX_COORD + 1024))]


@pytest.mark.parametrize("gid,pin,build", ANCHORED, ids=[g[0] for g in ANCHORED])
def test_anchored_far_outside_the_raster(cvs, flavour, gid, pin, build):
    """The raster of the coded planes sits at the origin; the frame is moved, the planes are not.  A reconstruction then
    leaves the frame as it was, its window empty; a subsampling writes the planes of a frame without pixels."""
    for what, case in build(cvs):
        twin = Twin(cvs)
        try:
            probe = NoPixels(twin, (0, 0))
            want_rc = case(probe)
            want = twin.collect()
            spec = [(o.cls, o.nbytes, o.row_bytes, o.out, o.cmp) for o in twin.objects]
        finally:
            twin.free()
        offsets = [(name, d, d) for name, d in FAR_FROM_THE_RASTER]
        for label, fac, rc, got in _far_runs(cvs, what, case, spec, offsets):
            assert rc == want_rc == 0, "%s: returned %r (%s)" % (label, rc, _lib.last_error())
            for o, h, g, w in zip(fac.objects, fac.hosts, got, want):
                if not o.out:
                    continue
                if h is not None:
                    assert o.frame.current_window.is_empty(), "%s: %s reports window %r" % (label, o.name, o.frame.current_window.tuple())
                    assert g.tobytes() == h.array.tobytes(), "%s: %s was written" % (label, o.name)
                else:
                    assert np.array_equal(g, w), "%s: %s is not what a frame without pixels gives" % (label, o.name)


# ------------------------------------------------------------------ refusals

class Bent(Shifted):
    """Nothing moved but ONE window of ONE frame (object `index`): translated whole, so that it keeps its size, until its
    `side` ('min' or 'max') corner sits on `value` -- the full window and the current window together (which='full'), or the
    current window alone (which='current').  Keeps what every operand was uploaded with."""

    def __init__(self, inner, index, which, side, value):
        Shifted.__init__(self, inner, (0, 0))
        self.index, self.which, self.side, self.value = index, which, side, value
        self.uploaded = []

    def frame(self, host, out=False, **kw):
        if len(self.objects) == self.index:
            full, cur = host.full_window.tuple(), host.current_window.tuple()
            if cur[2] < cur[0] or cur[3] < cur[1]:
                cur = full if self.which == "current" else cur          # (a window to bend: the whole buffer)
            ref = full if self.which == "full" else cur
            d = (self.value - ref[0], self.value - ref[1]) if self.side == "min" else (self.value - ref[2], self.value - ref[3])
            host = HostFrame(ec.move_box(full, d) if self.which == "full" else full, host.dtype, host.array, ec.move_box(cur, d))
        self.uploaded.append(host.array.tobytes())
        return Shifted.frame(self, host, out=out, **kw)

    def buffer(self, data, cls, **kw):
        self.uploaded.append(np.ascontiguousarray(data).tobytes())
        return Shifted.buffer(self, data, cls, **kw)


class BentPoint(Shifted):
    """Nothing moved but one point: the target's (source=False) or the source's, its x put on `value`."""

    def __init__(self, inner, source, value):
        Shifted.__init__(self, inner, (0, 0))
        self.bend_source, self.value, self.uploaded = source, value, []

    def frame(self, host, out=False, **kw):
        self.uploaded.append(host.array.tobytes())
        return Shifted.frame(self, host, out=out, **kw)

    def point(self, x, y, source=False):
        return v2f(self.value, y) if source == self.bend_source else v2f(x, y)


def _refused(cvs, label, case, make, words=("beyond", "no int holds")):
    """The call on a twin bent by make(twin): -1, a message with one of `words`, every output window empty, every byte as
    uploaded."""
    twin = Twin(cvs)
    try:
        fac = make(twin)
        rc = case(fac)
        message = _lib.last_error()
        got = twin.collect()
        assert rc == -1, "%s: returned %r, not -1 (%s)" % (label, rc, message)
        assert message and any(w in message for w in words), "%s: the message is %r" % (label, message)
        for o in twin.objects:
            if o.out and o.frame is not None:
                assert o.frame.current_window.is_empty(), "%s: %s reports window %r" % (label, o.name, o.frame.current_window.tuple())
        for o, g, up in zip(twin.objects, got, fac.uploaded):
            assert g.tobytes() == up, "%s: %s was written" % (label, o.name)
    finally:
        twin.free()


def _one_case_per_entry(gid, build):
    """The first case of the group that calls each device entry the group calls (found on the stand-in, without a device)."""
    rec, seen, picked = Recorder(), set(), []
    for k, (what, case) in enumerate(build(rec)):
        before = len(rec.calls)
        fac = HostOnly(rec, 1)
        case(fac)
        names = {n for n, _ in rec.calls[before:] if n.startswith("cvs_") and n.endswith("_dev")} - seen
        if names:
            seen |= names
            picked.append((k, [o.frame is not None for o in fac.objects], [o.reads for o in fac.objects]))
    return picked


REFUSING = [g for g in ec.GROUPS if _prefix(g[0]) not in ("flat_arrays", "workspace_stack")]
# (the workspace's device slot is no cvs_*_dev entry: its pull hands the bent frame to entries the other groups bend; a
# flat array has no window)


def _groups_that_reach_every_entry():
    """In catalogue order, the first group of each kind and every later group that calls a device entry none before it
    calls (found on the stand-in, without a device): every frame-taking entry is bent at least once."""
    rec, seen, kinds, picked = Recorder(), set(), set(), {}
    for g in REFUSING:
        before = len(rec.calls)
        for _what, case in g[2](rec):
            case(HostOnly(rec, 1))
        names = {n for n, _ in rec.calls[before:] if n.startswith("cvs_") and n.endswith("_dev")}
        if names - seen or _prefix(g[0]) not in kinds:
            picked[g[0]] = g
        seen |= names
        kinds.add(_prefix(g[0]))
    return picked


_FIRST_OF = _groups_that_reach_every_entry()


@pytest.mark.parametrize("gid,pin,build", list(_FIRST_OF.values()), ids=list(_FIRST_OF))
def test_one_past_the_bound_is_refused(cvs, flavour, gid, pin, build):
    """Every frame operand of one case per entry of the group, bent one past the bound of the entry's family (and one past
    CVS_MAX_COORD): refused, nothing launched.  Only when every such refusal has been seen -- a broken refusal fails the
    function before -- the same calls at INT_MAX and INT_MIN, where a kernel's row walk would not end."""
    rule = ec.FAR_CLASSES[_prefix(gid)][1]
    limits = sorted({rule["limit"] if rule else ec.MAX_COORD, ec.MAX_COORD})
    cases = build(cvs)
    picked = _one_case_per_entry(gid, build)
    assert picked
    cvs.cvs_fir_path_override(pin)
    try:
        for extreme in (False, True):
            for k, is_frame, reads in picked:
                what, case = cases[k]
                for index in [i for i, f in enumerate(is_frame) if f]:
                    bends = [("full", "max", lim + 1) for lim in limits] + [("full", "min", -lim - 1) for lim in limits]
                    if reads[index]:
                        bends += [("current", "max", limits[-1] + 1), ("current", "min", -limits[-1] - 1)]
                    if extreme:
                        bends = [("full", "max", ec.INT_MAX), ("full", "min", ec.INT_MIN)] + ([("current", "max", ec.INT_MAX), ("current", "min", ec.INT_MIN)] if reads[index] else [])
                    for which, side, value in bends:
                        # A bent full_window takes its current_window along: only the coordinate contract (the "beyond" of
                        # cvs_coords_refused, or the transform's own bound) can refuse it.  A current_window bent alone leaves
                        # its buffer, which the entries refused before there was a bound ("outside"): whichever check comes
                        # first in the entry, the call must still be refused and write nothing.
                        _refused(cvs, "%s, operand %d, %s_window's %s on %d" % (what, index, which, side, value), case,
                                 lambda twin: Bent(twin, index, which, side, value),
                                 ("beyond", "no int holds") if which == "full" else ("beyond", "outside"))
                if _prefix(gid) == "scale_bilinear":
                    for source in (False, True):
                        for value in ([float(ec.INT_MAX), float(ec.INT_MIN), float("inf")] if extreme else [ec.RESAMPLE_MAX_COORD + 1.0, -ec.RESAMPLE_MAX_COORD - 1.0]):
                            _refused(cvs, "%s, the %s point's x on %r" % (what, "source" if source else "target", value), case,
                                     lambda twin: BentPoint(twin, source, value))
    finally:
        cvs.cvs_fir_path_override(_lib.FIR_PATH_AUTO)


@pytest.mark.parametrize("half", [True, False], ids=["f16", "f32"])
def test_a_fill_everywhere_still_fills_the_frame(cvs, flavour, half):
    """The window of cvs_fill_solid_* is clipped, not refused: INT_MIN..INT_MAX ("everywhere", what the Python layer's solid
    source passes by default) fills the whole frame, at the origin and on the corners of the bound."""
    class Everywhere(Shifted):
        def box(self, x0, y0, x1, y1):
            return box2i.of(ec.INT_MIN, ec.INT_MIN, ec.INT_MAX, ec.INT_MAX)
    colour = _lib.rgba_f32(1.0, 0.5, 0.333333, 0.2)
    for full in [(-5, -5, 5, 6), (0, 0, 128, 6)]:
        def case(fac, full=full):
            f = fac.frame(ec.blank(half, full), out=True)
            b = fac.box(*full)
            entry = cvs.cvs_fill_solid_f16_dev if half else cvs.cvs_fill_solid_f32_dev
            return entry(f.ref(), C.byref(b), C.byref(colour), fac.stream)
        want_rc, want, want_windows, spec, boxes = _origin(cvs, case)           # the frame's own box as the window: all of it
        assert want_rc == 0 and want_windows[0].tuple() == full
        for d in [(0, 0), (ec.MAX_COORD - full[2], ec.MAX_COORD - full[3]), (-ec.MAX_COORD - full[0], -ec.MAX_COORD - full[1])]:
            twin = Twin(cvs)
            try:
                fac = Everywhere(twin, d)
                assert case(fac) == 0, _lib.last_error()
                got = twin.collect()
                assert fac.windows_back()[0].tuple() == full, (d, fac.windows_back()[0].tuple())
                assert np.array_equal(got[0], want[0]), "fill everywhere, frame moved by %r" % (d,)
            finally:
                twin.free()


def test_host_entries_move_and_refuse_alike(cvs, flavour):
    """The video_* entries on host frames go through the same bound before a byte is staged: a copy and an over at the top
    corner give the origin's bytes, one pixel further they give an empty window, a message and an untouched target."""
    rng = np.random.default_rng(77)
    full, cur = (0, 0, 40, 8), (3, 1, 37, 7)
    src16, src32 = ec.px16(rng, full, cur), ec.px32(rng, full, cur)

    def run(d):
        out16, out32 = ec.blank(True, full), ec.px32(np.random.default_rng(78), full, (0, 0, 20, 5))
        a16 = HostFrame(ec.move_box(full, d), np.uint16, src16.array.copy(), ec.move_box(cur, d))
        a32 = HostFrame(ec.move_box(full, d), np.float32, src32.array.copy(), ec.move_box(cur, d))
        o16 = HostFrame(ec.move_box(full, d), np.uint16, out16.array.copy(), (0, 0, -1, -1))
        o32 = HostFrame(ec.move_box(full, d), np.float32, out32.array.copy(), ec.move_box((0, 0, 20, 5), d))
        cvs.video_copy_frame_f16(o16.ref(), a16.ref())
        m16 = _lib.last_error()
        cvs.video_mix_over_f32(o32.ref(), a32.ref(), C.c_float(0.35))
        return (o16, out16, m16), (o32, out32, _lib.last_error())
    (w16, _, _), (w32, _, _) = run((0, 0))
    corner = (ec.MAX_COORD - full[2], ec.MAX_COORD - full[3])
    (g16, _, _), (g32, _, _) = run(corner)
    for g, w in ((g16, w16), (g32, w32)):
        assert g.current_window.tuple() == ec.move_box(w.current_window.tuple(), corner)
        assert g.array.tobytes() == w.array.tobytes()
    for beyond in ((corner[0] + 1, corner[1]), (corner[0], corner[1] + 1), (-ec.MAX_COORD - 1, 0), (ec.INT_MAX - full[2], 0), (0, ec.INT_MIN)):
        for got, before, message in run(beyond):
            assert got.current_window.is_empty(), (beyond, got.current_window.tuple())
            assert "beyond" in message, (beyond, message)
            assert got.array.tobytes() == before.array.tobytes(), beyond
