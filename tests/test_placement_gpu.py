"""Every windowed cvs_*_dev entry point on frames packed into a guarded arena (tests/arena.py; DESIGN.md "Placement").

Elsewhere in the suite a frame is a DeviceFrame with its own allocation: it starts on a boundary of 256 bytes or more and what
lies around it is allocator slack nobody reads back.  Here one call is made twice over: on frames with allocations of their own
(the twin, which the other GPU tests tie to the oracle and the models) and on the same frames placed in one arena at chosen
addresses modulo 256, each between two guard bands of poison.  Per placement the return code, every reported window and every
output buffer -- the whole buffer -- must equal the twin's (copies code for code, computed pixels through tests/util.py
canon_f16 / canon_f32, because another instance of the kernel may run at another alignment); the outputs must be the same bytes
under a NaN poison and a finite one (a tap taken outside the buffer changes one of them); every guard byte must still hold the
poison and every input must be byte-identical to what was uploaded (arena.check()).

Placements: half frames at 0, 8, 24 and 136 modulo 256, float frames at 0, 16, 48 and 144, coded planes at 0, 1, 2, 3 and 7,
byte targets at 0, 4 and 12.  The launchers' fast-path predicates AND their operands, so a case runs with everything aligned,
with each object alone off the 16-byte (for bytes: the element) grid, and with all of them off it at each residue in turn.
Addresses below the pixel's own alignment are outside the contract (include/canvas_hip.h) and are not run.

The calls themselves -- the case builders, their geometries and pixels -- are the catalogue of tests/entry_cases.py, which
tests/test_graph_replay_gpu.py runs a second way.

Both arithmetic flavours, set here (tests/conftest.py parametrises two other modules only)."""
import numpy as np
import pytest

from canvas_amd import _lib
from canvas_amd.abi import box2i
from tests import arena as ar
from tests import entry_cases as ec
from tests.entry_cases import Factory, Twin
from tests.util import canon_f16, canon_f32, same_window

pytestmark = pytest.mark.gpu

RESIDUES = {"f16": (0, 8, 24, 136), "f32": (0, 16, 48, 144), "plane": (0, 1, 2, 3, 7), "bytes": (0, 4, 12)}


@pytest.fixture(scope="module", params=["separate", "contracted"])
def flavour(request, cvs):
    before = cvs.cvs_set_arithmetic(_lib.ARITH_CONTRACTED if request.param == "contracted" else _lib.ARITH_SEPARATE)
    yield request.param
    cvs.cvs_set_arithmetic(before if before >= 0 else _lib.ARITH_SEPARATE)
    cvs.cvs_fir_path_override(_lib.FIR_PATH_AUTO)


# ------------------------------------------------------------------ the arena's factory (the twin's is tests/entry_cases.py Twin)

class Packed(Factory):
    """Every object in the arena, object k at residues[k] modulo 256."""

    def __init__(self, cvs, arena, residues):
        Factory.__init__(self, cvs)
        self.arena, self.residues = arena, residues

    def _make_frame(self, o, host):
        k = len(self.objects) - 1
        o.frame = self.arena.place(host.full_window, host.dtype, self.residues[k], host.current_window, name=o.name)
        o.ptr, o.placed = o.frame.ptr, o.frame.placed
        self.arena.upload(o.placed, host.array, is_input=not o.out)

    def _make_buffer(self, o, data):
        k = len(self.objects) - 1
        o.ptr, o.placed = self.arena.place_bytes(data.size, self.residues[k], name=o.name)
        self.arena.upload(o.placed, data, is_input=not o.out)

    def collect(self):
        self.arena.download()
        return [self.arena.read(o.placed) for o in self.objects]


def placements(classes):
    """Residue tuples for objects of these classes: all aligned; each alone on its first off-grid residue; all off the grid,
    at each residue of their class in turn."""
    out = [tuple(0 for _ in classes)]
    if len(classes) > 1:
        for i in range(len(classes)):
            out.append(tuple(RESIDUES[c][1] if k == i else 0 for k, c in enumerate(classes)))
    for r in range(1, max(len(RESIDUES[c]) for c in classes)):
        out.append(tuple(RESIDUES[c][min(r, len(RESIDUES[c]) - 1)] for c in classes))
    return out


def _canon(raw, cmp):
    if cmp == "f16":
        return canon_f16(raw.view(np.uint16))
    if cmp == "f32":
        return canon_f32(raw.view(np.float32))
    return raw


def _windows(fac):
    return [o.frame.current_window if o.frame is not None else None for o in fac.objects]


def run_case(cvs, what, case):
    """case(fac) makes ONE call on operands it takes from fac, in the same order every time, and returns its return code."""
    twin = Twin(cvs)
    try:
        want_rc = case(twin)
        want = twin.collect()
        want_windows = [None if w is None else box2i.of(*w.tuple()) for w in _windows(twin)]
        spec = [(o.cls, o.nbytes, o.row_bytes, o.out, o.cmp) for o in twin.objects]
    finally:
        twin.free()
    guard = ar.guard_bytes([s[2] for s in spec])
    arena = ar.Arena(cvs, ar.capacity_for([s[1] for s in spec], guard), guard)
    try:
        for residues in placements([s[0] for s in spec]):
            runs = {}
            for pname, poison in ar.POISONS:
                label = "%s, residues %r, %s poison" % (what, residues, pname)
                arena.fill(poison)
                fac = Packed(cvs, arena, residues)
                rc = case(fac)
                got = fac.collect()
                assert [(o.cls, o.nbytes, o.row_bytes, o.out, o.cmp) for o in fac.objects] == spec, label + ": the case is not the same case"
                for o, r in zip(fac.objects, residues):
                    assert o.ptr % 256 == r
                assert rc == want_rc, "%s: returned %r, the twin %r (%s)" % (label, rc, want_rc, _lib.last_error())
                for o, w, ww in zip(fac.objects, _windows(fac), want_windows):
                    assert w is None or same_window(w, ww), "%s: %s reports window %r, the twin %r" % (label, o.name, w.tuple(), ww.tuple())
                try:
                    arena.check()
                except AssertionError as e:
                    raise AssertionError("%s: %s" % (label, e))
                runs[pname] = (fac.objects, got)
            for o, a, b in zip(runs["nan"][0], runs["nan"][1], runs["finite"][1]):
                assert not o.out or np.array_equal(a, b), "%s, residues %r: %s depends on what lies outside the buffers" % (what, residues, o.name)
            for pname, (objects, got) in runs.items():
                for o, g, w in zip(objects, got, want):
                    if not o.out:
                        continue
                    a, b = _canon(g, o.cmp), _canon(w, o.cmp)
                    if not np.array_equal(a, b):
                        bad = np.flatnonzero(a != b)
                        raise AssertionError("%s, residues %r, %s poison: %s differs from the twin in %d of %d elements, first at element %d: 0x%x, twin 0x%x" % (
                            what, residues, pname, o.name, bad.size, a.size, bad[0], a[bad[0]], b[bad[0]]))
    finally:
        arena.free()


def _run_all(cvs, cases, pin=_lib.FIR_PATH_AUTO):
    cvs.cvs_fir_path_override(pin)
    try:
        for what, case in cases:
            run_case(cvs, what, case)
    finally:
        cvs.cvs_fir_path_override(_lib.FIR_PATH_AUTO)


# ------------------------------------------------------------------ copies, conversions, fills, gain, colour

def test_copies_and_conversions(cvs, flavour):
    _run_all(cvs, ec.copies_and_conversions(cvs))


def test_weave_fields(cvs, flavour):
    _run_all(cvs, ec.weave_fields(cvs))


def test_solid_fills(cvs, flavour):
    _run_all(cvs, ec.solid_fills(cvs))


@pytest.mark.parametrize("pre,post", ec.COLOUR_MATRIX_TABLES)
def test_colour_matrix(cvs, flavour, pre, post):
    _run_all(cvs, ec.colour_matrix(cvs, pre, post))


# ------------------------------------------------------------------ mixers

@pytest.mark.parametrize("full", ec.MIXER_FULLS)
def test_mixers_f32(cvs, flavour, full):
    _run_all(cvs, ec.mixers_f32(cvs, full))


def test_mix_cross_f16(cvs, flavour):
    _run_all(cvs, ec.mix_cross_f16(cvs))


# ------------------------------------------------------------------ the fused chain

@pytest.mark.parametrize("plain", [False, True])
@pytest.mark.parametrize("nlayers", ec.CHAIN_LAYERS)
@pytest.mark.parametrize("size", ec.CHAIN_SIZES)
def test_chain(cvs, flavour, size, nlayers, plain):
    """The fused kernel moves 16 bytes per lane: one layer or the output off a 16-byte boundary sends the call node by node
    (host/color.c), which must be reported and must give the same bits."""
    fused = []

    def after(fac, out, dl):
        was = cvs.cvs_chain_last_was_fused()
        if isinstance(fac, Twin):
            fused.append(was)
        else:
            assert was == (fused[0] if fac.aligned16(out, *dl) else 0), "fused: %d with residues %r" % (was, fac.residues)
    _run_all(cvs, ec.chain(cvs, size, nlayers, plain, after))
    assert fused[0] == 1, "the twin's call was not fused"


# ------------------------------------------------------------------ row streams: fields and key

@pytest.mark.parametrize("width", ec.STREAM_WIDTHS)
@pytest.mark.parametrize("op", ec.FIELD_OPS)
def test_field_conversions(cvs, flavour, op, width):
    _run_all(cvs, ec.field_conversions(cvs, op, width))


@pytest.mark.parametrize("width", ec.STREAM_WIDTHS)
@pytest.mark.parametrize("half", [True, False], ids=["f16", "f32"])
def test_chroma_key(cvs, flavour, half, width):
    _run_all(cvs, ec.chroma_key(cvs, half, width))


# ------------------------------------------------------------------ matte: the LDS halo at the buffer's edge

@pytest.mark.parametrize("width", ec.MATTE_WIDTHS)
@pytest.mark.parametrize("half", [True, False], ids=["f16", "f32"])
def test_matte(cvs, flavour, half, width):
    """Source window = the whole buffer: every halo pixel of the border tiles lies outside the allocation."""
    _run_all(cvs, ec.matte(cvs, half, width))


# ------------------------------------------------------------------ transform: clamped taps on the buffer's first and last pixel

@pytest.mark.parametrize("tw", ec.TRANSFORM_WIDTHS)
@pytest.mark.parametrize("half", [True, False], ids=["f16", "f32"])
def test_transform(cvs, flavour, half, tw):
    _run_all(cvs, ec.transform(cvs, half, tw))


# ------------------------------------------------------------------ blur, unsharp mask, blur + stack

@pytest.mark.parametrize("ntaps", ec.BLUR_TAPS)
@pytest.mark.parametrize("half", [True, False], ids=["f16", "f32"])
def test_blur_and_unsharp(cvs, flavour, half, ntaps):
    """Source window = the whole buffer; 3, 9, 13: the register window, two columns per lane where the predicate allows;
    15, 31: k_blur; even counts: the table kernels."""
    _run_all(cvs, ec.blur_and_unsharp(cvs, half, ntaps))


@pytest.mark.parametrize("columns", [None, 1, 2])
@pytest.mark.parametrize("ntaps", ec.BLUR_OVER_TAPS)
def test_blur_over(cvs, flavour, ntaps, columns):
    """cvs_blur_over_f16_dev with 1 and 3 overlays (each misaligned in turn by the placements) and its batch form."""
    _run_all(cvs, ec.blur_over(cvs, ntaps), ec.COLUMN_PINS[columns])


# ------------------------------------------------------------------ Lanczos

@pytest.mark.parametrize("pin", ec.LANCZOS_PINS)
@pytest.mark.parametrize("ssize,tsize,fx,fy", ec.LANCZOS_SHAPES)
def test_lanczos_resample(cvs, flavour, pin, ssize, tsize, fx, fy):
    _run_all(cvs, ec.lanczos_resample(cvs, pin, ssize, tsize, fx, fy), ec.PINS[pin])


@pytest.mark.parametrize("pin", ec.BLUR_LANCZOS_PINS)
@pytest.mark.parametrize("ntaps", ec.BLUR_LANCZOS_TAPS)
def test_blur_lanczos(cvs, flavour, ntaps, pin):
    """Factor 1/2 on both axes: the halving sweeps, two source columns per lane (pinned, or where the predicate allows) and
    one; 13 taps: no one-sweep form.  Single calls and the batch form; 0.4 x 0.35 goes through the table kernels."""
    _run_all(cvs, ec.blur_lanczos(cvs, ntaps, pin), ec.PINS[pin])


# ------------------------------------------------------------------ the bilinear scaler

@pytest.mark.parametrize("fac_,tsize,pin,k_aligned,k_other", ec.SCALE_CASES)
@pytest.mark.parametrize("half", [True, False], ids=["f16", "f32"])
def test_scale_bilinear(cvs, flavour, half, fac_, tsize, pin, k_aligned, k_other):
    def after(fac, out):
        if k_aligned is not None:
            tiles_ok = not half or (fac.aligned16(out) and tsize[0] % 2 == 0)
            assert cvs.cvs_fir_last_kernel() == (k_aligned if tiles_ok else k_other), (cvs.cvs_fir_last_kernel(), out.ptr & 15)
    _run_all(cvs, ec.scale_bilinear(cvs, half, fac_, tsize, pin, after), ec.PINS[pin])


# ------------------------------------------------------------------ coded planes: DV and MPEG-2

@pytest.mark.parametrize("pads", ec.PLANE_PADS)
def test_dv(cvs, flavour, pads):
    """The DV raster is fixed (720 x 480, first line at y = -1); the frames over it are small: 2 x 4, 130 x 8, 64 x 36, and the
    raster's last rows and columns."""
    _run_all(cvs, ec.dv(cvs, pads))


@pytest.mark.parametrize("pads,extra", ec.MPEG2_PADS)
@pytest.mark.parametrize("width,height", ec.MPEG2_SIZES)
def test_mpeg2(cvs, flavour, width, height, pads, extra):
    _run_all(cvs, ec.mpeg2(cvs, width, height, pads, extra))


# ------------------------------------------------------------------ display bytes

@pytest.mark.parametrize("pre", ec.DISPLAY_TABLES)
def test_display_bytes(cvs, flavour, pre):
    _run_all(cvs, ec.display_bytes(cvs, pre))
