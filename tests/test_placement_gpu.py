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

Both arithmetic flavours, set here (tests/conftest.py parametrises two other modules only)."""
import ctypes as C
import math

import numpy as np
import pytest

from canvas_amd import _lib, synth
from canvas_amd.abi import HostFrame, box2i, v2f
from canvas_amd.device import DeviceFrame
from tests import arena as ar
from tests.util import canon_f16, canon_f32, f32p, same_window

pytestmark = pytest.mark.gpu

RESIDUES = {"f16": (0, 8, 24, 136), "f32": (0, 16, 48, 144), "plane": (0, 1, 2, 3, 7), "bytes": (0, 4, 12)}
SENT16 = np.array([0x7E17, 0x1234, 0xFBCD, 0x0001], np.uint16)
SENT32 = np.array([1234.5, -7.25, 3.0e-5, 0.4375], np.float32)
SPECIALS16 = np.array([0x0000, 0x8000, 0x0001, 0x83FF, 0x0400, 0x7BFF, 0xFBFF, 0x7C00, 0xFC00, 0x7E00, 0x7C01, 0x3C00, 0xBC00], np.uint16)
SPECIALS32 = np.array([0.0, -0.0, 1e-42, -3e38, np.inf, -np.inf, np.nan, 1.0, -1.0, 65520.0], np.float32)
REC709_RGB_TO_YPBPR = [0.2126, 0.7152, 0.0722, -0.114572, -0.385428, 0.5, 0.5, -0.454153, -0.045847]
PAD = 0xA5


@pytest.fixture(scope="module", params=["separate", "contracted"])
def flavour(request, cvs):
    before = cvs.cvs_set_arithmetic(_lib.ARITH_CONTRACTED if request.param == "contracted" else _lib.ARITH_SEPARATE)
    yield request.param
    cvs.cvs_set_arithmetic(before if before >= 0 else _lib.ARITH_SEPARATE)
    cvs.cvs_fir_path_override(_lib.FIR_PATH_AUTO)


# ------------------------------------------------------------------ the two factories

def _box(full):
    return (full[3] - full[1] + 1, full[2] - full[0] + 1)


class _Object:
    def __init__(self, cls, name, out, cmp, nbytes, row_bytes):
        self.cls, self.name, self.out, self.cmp, self.nbytes, self.row_bytes = cls, name, out, cmp, nbytes, row_bytes
        self.frame = None      # DeviceFrame, for frames
        self.ptr = None
        self.placed = None


class Factory:
    """What a case asks its operands from.  frame(): a device frame holding `host`'s pixels and window; buffer(): device bytes
    holding `data`.  out=True marks what the call may write; cmp says how an output is compared with the twin's ('exact': code
    for code, 'f16' / 'f32': canonical codes).  An input must come back unwritten."""

    def __init__(self, cvs):
        self.cvs = cvs
        self.objects = []

    def frame(self, host, out=False, cmp="exact", name=None):
        cls = "f16" if host.dtype == np.uint16 else "f32"
        o = _Object(cls, name or "%s %s %d" % ("output" if out else "input", cls, len(self.objects)), out, cmp, host.array.nbytes,
                    host.array.shape[1] * 4 * host.dtype.itemsize)
        self.objects.append(o)
        self._make_frame(o, host)
        return o.frame

    def buffer(self, data, cls, out=False, name=None):
        data = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        o = _Object(cls, name or "%s %s %d" % ("output" if out else "input", cls, len(self.objects)), out, "exact", data.size, 0)
        self.objects.append(o)
        self._make_buffer(o, data)
        return o.ptr

    def aligned16(self, *frames):
        return all((f.ptr & 15) == 0 for f in frames)


class Twin(Factory):
    """Every object in an allocation of its own."""

    def _make_frame(self, o, host):
        o.frame = DeviceFrame.from_host(host)
        o.ptr = o.frame.ptr

    def _make_buffer(self, o, data):
        o.ptr = self.cvs.cvs_malloc(max(data.size, 1))
        assert o.ptr
        if data.size:
            _lib.check(self.cvs.cvs_memcpy_h2d(o.ptr, data.ctypes.data, data.size, None), "h2d")

    def collect(self):
        _lib.check(self.cvs.cvs_stream_sync(None), "sync")
        got = []
        for o in self.objects:
            a = np.empty(o.nbytes, np.uint8)
            if o.nbytes:
                _lib.check(self.cvs.cvs_memcpy_d2h(a.ctypes.data, o.ptr, o.nbytes, None), "d2h")
            got.append(a)
        return got

    def free(self):
        for o in self.objects:
            if o.frame is not None:
                o.frame.free()
            elif o.ptr:
                self.cvs.cvs_free(o.ptr)
            o.ptr = None


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


# ------------------------------------------------------------------ pixels

def px16(rng, full, cur=None):
    h, w = _box(full)
    codes = rng.integers(0, 0x3C01, (h, w, 4), dtype=np.uint16)
    hit = rng.uniform(size=codes.shape) < 0.02
    codes[hit] = SPECIALS16[rng.integers(0, len(SPECIALS16), int(hit.sum()))]
    return HostFrame(full, np.uint16, codes, full if cur is None else cur)


def px32(rng, full, cur=None):
    h, w = _box(full)
    a = rng.uniform(-0.25, 1.25, (h, w, 4)).astype(np.float32)
    hit = rng.uniform(size=a.shape) < 0.01
    a[hit] = SPECIALS32[rng.integers(0, len(SPECIALS32), int(hit.sum()))]
    return HostFrame(full, np.float32, a, full if cur is None else cur)


def px(rng, half, full, cur=None):
    return px16(rng, full, cur) if half else px32(rng, full, cur)


def blank(half, full, cur=None):
    """A target: the sentinel in every pixel, so that what a call leaves alone is seen to be left alone."""
    h, w = _box(full)
    a = np.broadcast_to(SENT16 if half else SENT32, (h, w, 4)).copy()
    return HostFrame(full, np.uint16 if half else np.float32, a, (0, 0, -1, -1) if cur is None else cur)


def _table(frames, cls=_lib.rgba_frame_f16_t):
    return (C.POINTER(cls) * max(len(frames), 1))(*[C.pointer(f.c) for f in frames])


def _run_all(cvs, cases):
    for what, case in cases:
        run_case(cvs, what, case)


# ------------------------------------------------------------------ copies, conversions, fills, gain, colour

COPY_GEOMETRIES = [
    ((0, 0, 15, 8), (0, 0, 15, 8), (0, 0, 15, 8)),             # out.full, in.full, in.current: whole, even width
    ((0, 0, 128, 8), (0, 0, 128, 8), (0, 0, 128, 8)),          # odd width: every second row starts off a 16-byte boundary
    ((0, 0, 129, 4), (0, 0, 129, 4), (1, 0, 129, 4)),          # an odd first column, up to the buffer's last pixel
    ((0, 0, 15, 8), (-4, -4, 20, 12), (-2, -3, 18, 11)),       # the target clips a larger source
    ((-1, -1, 1, 1), (0, 0, 3, 3), (0, 0, 2, 2)),
    ((0, 0, 0, 0), (0, 0, 0, 0), (0, 0, 0, 0)),                # one pixel
    ((0, 0, 15, 8), (0, 0, 15, 8), (0, 0, -1, -1)),            # empty input
]


def test_copies_and_conversions(cvs, flavour):
    cases = []
    for g, (ofull, ifull, icur) in enumerate(COPY_GEOMETRIES):
        def make(entry, out_half, in_half, cmp, extra=(), g=g, ofull=ofull, ifull=ifull, icur=icur):
            def case(fac):
                rng = np.random.default_rng(100 + g)
                src = fac.frame(px(rng, in_half, ifull, icur))
                out = fac.frame(blank(out_half, ofull), out=True, cmp=cmp)
                return getattr(cvs, entry)(out.ref(), src.ref(), *extra, None)
            return ("%s %r" % (entry, (ofull, ifull, icur)), case)
        cases += [make("cvs_copy_frame_f16_dev", True, True, "exact"),
                  make("cvs_copy_frame_alpha_f32_dev", False, False, "f32", (C.c_float(0.4),)),
                  make("cvs_copy_frame_alpha_f32_dev", False, False, "f32", (C.c_float(1.0),)),
                  make("cvs_frame_f16_to_f32_dev", False, True, "f32"),
                  make("cvs_frame_f32_to_f16_dev", True, False, "f16"),
                  make("cvs_gain_offset_f16_dev", True, True, "f16", (C.c_float(1.5), C.c_float(0.0625)))]
    _run_all(cvs, cases)


WEAVE_GEOMETRIES = [
    ((0, 0, 31, 17), (0, 0, 31, 17), (0, 0, 31, 17)),          # full, current, the other field's current: whole frame
    ((0, -1, 128, 16), (0, -1, 128, 16), (0, -1, 128, 16)),    # odd width, first line at y = -1
    ((-4, -3, 40, 20), (3, 2, 29, 14), (3, 2, 29, 14)),        # min.x > 0: the reference's row address starts 3 pixels early
    ((-8, -3, 40, 20), (-5, 2, 20, 9), (-5, 2, 20, 9)),        # min.x < 0: it starts 5 pixels late and runs into the next row
    ((-8, -3, 40, 9), (-5, 2, 40, 9), (-5, 2, 40, 9)),         # ... in the buffer's LAST rows, up to its last column
    ((0, 0, 31, 17), (0, 0, 31, 17), (4, 3, 20, 9)),
]


def test_weave_fields(cvs, flavour):
    cases = []
    for g, (full, cur, ocur) in enumerate(WEAVE_GEOMETRIES):
        def case(fac, g=g, full=full, cur=cur, ocur=ocur):
            rng = np.random.default_rng(200 + g)
            frame = fac.frame(px16(rng, full, cur), out=True)
            other = fac.frame(px16(rng, cur, ocur))
            return cvs.cvs_weave_fields_f16_dev(frame.ref(), other.ref(), None)
        cases.append(("weave %r" % ((full, cur, ocur),), case))
    _run_all(cvs, cases)


def test_solid_fills(cvs, flavour):
    color = _lib.rgba_f32(1.0, 0.5, 0.333333, 0.2)
    cases = []
    for full, win in [((-5, -5, 5, 6), (-3, -3, 1, 4)), ((0, 0, 128, 6), (0, 0, 128, 6)), ((0, 0, 128, 6), (1, 0, 128, 6)),
                      ((0, 0, 129, 6), (1, 1, 128, 5)), ((0, 0, 3, 3), (-2, -2, 9, 9)), ((0, 0, 0, 0), (0, 0, 0, 0))]:
        for half in (True, False):
            def case(fac, full=full, win=win, half=half):
                f = fac.frame(blank(half, full), out=True)
                b = box2i.of(*win)
                entry = cvs.cvs_fill_solid_f16_dev if half else cvs.cvs_fill_solid_f32_dev
                return entry(f.ref(), C.byref(b), C.byref(color), None)
            cases.append(("fill %s %r" % ("f16" if half else "f32", (full, win)), case))
    _run_all(cvs, cases)


@pytest.mark.parametrize("pre,post", [(-1, -1), (0, 2)])
def test_colour_matrix(cvs, flavour, pre, post):
    m = np.array(REC709_RGB_TO_YPBPR, np.float32)
    cases = []
    for full, cur in [((0, 0, 63, 35), (0, 0, 63, 35)), ((0, 0, 62, 34), (0, 0, 62, 34)), ((-3, -2, 60, 33), (0, 0, 57, 30)),
                      ((0, 0, 128, 6), (1, 0, 128, 6)), ((0, 0, 1, 0), (0, 0, 1, 0))]:
        def in_place(fac, full=full, cur=cur):
            f = fac.frame(px16(np.random.default_rng(300), full, cur), out=True, cmp="f16")
            return cvs.cvs_color_matrix_f16_dev(f.ref(), f32p(m), pre, post, None)
        cases.append(("colour matrix in place %r" % ((full, cur),), in_place))
    for ofull, ifull, icur in [((0, 0, 63, 35), (0, 0, 63, 35), (0, 0, 63, 35)), ((0, 0, 62, 34), (0, 0, 62, 34), (0, 0, 62, 34)),
                               ((-2, -2, 50, 30), (0, 0, 63, 35), (3, 1, 60, 33)), ((0, 0, 128, 6), (0, 0, 128, 6), (1, 0, 128, 6))]:
        def to(fac, ofull=ofull, ifull=ifull, icur=icur):
            src = fac.frame(px16(np.random.default_rng(301), ifull, icur))
            out = fac.frame(blank(True, ofull), out=True, cmp="f16")
            return cvs.cvs_color_matrix_f16_to_dev(out.ref(), src.ref(), f32p(m), pre, post, None)
        cases.append(("colour matrix out of place %r" % ((ofull, ifull, icur),), to))
    _run_all(cvs, cases)


# ------------------------------------------------------------------ mixers

FULL = (0, 0, 23, 11)
MIX_WINDOWS = [(FULL, FULL), (FULL, (3, 2, 10, 6)), ((2, 1, 12, 7), (6, 4, 20, 10)),
               ((6, 4, 20, 10), (2, 1, 12, 7)),            # the `left` selector quirk: addresses before the rows they belong to
               ((0, 5, 12, 9), (5, 0, 20, 7)), ((1, 1, 6, 3), (9, 6, 14, 9)), ((4, 0, 9, 11), (0, 3, 23, 8)),
               ((0, 0, 23, 3), (1, 8, 23, 11))]             # first rows against last rows, up to the last pixel


@pytest.mark.parametrize("full", [FULL, (0, 0, 22, 11)])
def test_mixers_f32(cvs, flavour, full):
    cases = []
    for g, (pw, qw) in enumerate(MIX_WINDOWS):
        pw, qw = [tuple(min(v, full[2]) if k == 2 else v for k, v in enumerate(w)) for w in (pw, qw)]

        def over(fac, g=g, pw=pw, qw=qw):
            rng = np.random.default_rng(400 + g)
            out = fac.frame(px32(rng, full, pw), out=True, cmp="f32")
            upper = fac.frame(px32(rng, full, qw))
            return cvs.cvs_mix_over_f32_dev(out.ref(), upper.ref(), C.c_float(0.35), None)

        def cross(fac, g=g, pw=pw, qw=qw):
            rng = np.random.default_rng(450 + g)
            a, b = fac.frame(px32(rng, full, pw)), fac.frame(px32(rng, full, qw))
            out = fac.frame(blank(False, full), out=True, cmp="f32")
            return cvs.cvs_mix_cross_f32_dev(out.ref(), a.ref(), b.ref(), C.c_float(0.2), None)
        cases += [("mix over %r" % ((pw, qw),), over), ("mix cross %r" % ((pw, qw),), cross)]
    _run_all(cvs, cases)


def test_mix_cross_f16(cvs, flavour):
    cases = []
    for size in [(96, 54), (33, 7), (1, 1), (2, 1)]:
        full = (0, 0, size[0] - 1, size[1] - 1)

        def whole(fac, full=full):
            rng = np.random.default_rng(500)
            a, b = fac.frame(px16(rng, full)), fac.frame(px16(rng, full))
            out = fac.frame(blank(True, full), out=True, cmp="f16")
            return cvs.cvs_mix_cross_f16_dev(out.ref(), a.ref(), b.ref(), C.c_float(0.3), None)
        cases.append(("cross f16 %r" % (size,), whole))
    for g, (pw, qw) in enumerate(MIX_WINDOWS):
        def windowed(fac, g=g, pw=pw, qw=qw):
            rng = np.random.default_rng(520 + g)
            a, b = fac.frame(px16(rng, FULL, pw)), fac.frame(px16(rng, FULL, qw))
            out = fac.frame(blank(True, FULL), out=True, cmp="f16")
            return cvs.cvs_mix_cross_f16_dev(out.ref(), a.ref(), b.ref(), C.c_float(0.3), None)
        cases.append(("cross f16 %r" % ((pw, qw),), windowed))
    _run_all(cvs, cases)


# ------------------------------------------------------------------ the fused chain

@pytest.mark.parametrize("plain", [False, True])
@pytest.mark.parametrize("nlayers", [1, 2, 4, 5, 7, 8])
@pytest.mark.parametrize("size", [(64, 36), (2, 1)])
def test_chain(cvs, flavour, size, nlayers, plain):
    """The fused kernel moves 16 bytes per lane: one layer or the output off a 16-byte boundary sends the call node by node
    (host/color.c), which must be reported and must give the same bits."""
    w, h = size
    m = None if plain else np.array(REC709_RGB_TO_YPBPR, np.float32)
    pre = _lib.LUT_NONE if plain else _lib.LUT_REC709_TO_LINEAR_SCENE
    layers = [synth.layer_frame(w, h, k, 0) for k in range(nlayers)]
    fused = []

    def case(fac):
        dl = [fac.frame(l, name="layer %d" % k) for k, l in enumerate(layers)]
        out = fac.frame(blank(True, (0, 0, w - 1, h - 1)), out=True, cmp="f16", name="chain output")
        jobs = (_lib.chain_job * 1)()
        jobs[0].out = C.pointer(out.c)
        for k, l in enumerate(dl):
            jobs[0].layers[k] = C.pointer(l.c)
        jobs[0].nlayers = nlayers
        rc = cvs.cvs_chain_color_over_f16_dev(jobs, 1, None if m is None else f32p(m), pre, _lib.LUT_NONE, None)
        was = cvs.cvs_chain_last_was_fused()
        if isinstance(fac, Twin):
            fused.append(was)
        else:
            assert was == (fused[0] if fac.aligned16(out, *dl) else 0), "fused: %d with residues %r" % (was, fac.residues)
        return rc
    run_case(cvs, "chain %dx%d, %d layers%s" % (w, h, nlayers, ", plain" if plain else ""), case)
    assert fused[0] == 1, "the twin's call was not fused"


# ------------------------------------------------------------------ row streams: fields and key

def _stream_geometries(w, h):
    """(source full, source current, target full): a window that touches all four edges of the buffer, one whose first column
    is odd and one whose first column is even relative to the buffer's, and a buffer with an odd origin."""
    full = (0, 0, w - 1, h - 1)
    out = [(full, full, full)]
    if w > 2:
        out.append((full, (1, 0, w - 1, h - 1), full))                 # odd first column, up to the last pixel
        out.append((full, (2 if w > 3 else 0, 0, w - 2, h - 1), full))  # even first column, an odd or even last one
    out.append(((-3, -1, w - 4, h - 2), (-3, -1, w - 4, h - 2), (-3, -1, w - 4, h - 2)))
    if h > 2:
        out.append((full, (0, 1, w - 1, h - 2), (-1, 0, w, h - 1)))    # rows inside, a target with an odd base column
    return out


@pytest.mark.parametrize("width", [1, 2, 129, 130])
@pytest.mark.parametrize("op", ["field0", "field1", "soften", "interlace"])
def test_field_conversions(cvs, flavour, op, width):
    cases = []
    for height in (1, 9, 17):
        for g, (sfull, scur, tfull) in enumerate(_stream_geometries(width, height)):
            def case(fac, g=g, sfull=sfull, scur=scur, tfull=tfull):
                rng = np.random.default_rng(600 + g + height)
                a = fac.frame(px16(rng, sfull, scur))
                b = fac.frame(px16(rng, sfull, scur)) if op == "interlace" else None
                out = fac.frame(blank(True, tfull), out=True, cmp="exact" if op == "interlace" else "f16")
                if op == "interlace":
                    return cvs.cvs_interlace_fields_f16_dev(out.ref(), a.ref(), b.ref(), None)
                if op == "soften":
                    return cvs.cvs_soften_fields_f16_dev(out.ref(), a.ref(), None)
                return cvs.cvs_field_to_frame_f16_dev(out.ref(), a.ref(), int(op[-1]), None)
            cases.append(("%s %dx%d %r" % (op, width, height, (sfull, scur, tfull)), case))
    _run_all(cvs, cases)


KEY_SETTINGS = [dict(key=(0.1, 0.8, 0.15), tolerance=0.08, softness=0.25, spill=0.8, spill_range=0.4, flags=0),
                dict(key=(0.9, -0.1, 1.2), tolerance=0.0, softness=0.1, spill=0.5, spill_range=0.3, flags=_lib.KEY_SHOW_MATTE)]


@pytest.mark.parametrize("width", [1, 2, 129, 130])
@pytest.mark.parametrize("half", [True, False], ids=["f16", "f32"])
def test_chroma_key(cvs, flavour, half, width):
    cases = []
    for height in (1, 9, 17):
        for g, (sfull, scur, tfull) in enumerate(_stream_geometries(width, height)):
            p = KEY_SETTINGS[(g + height) % 2]
            params = _lib.chroma_key((C.c_float * 3)(*p["key"]), p["tolerance"], p["softness"], p["spill"], p["spill_range"], p["flags"])

            def case(fac, g=g, sfull=sfull, scur=scur, tfull=tfull, params=params):
                rng = np.random.default_rng(700 + g + height)
                src = fac.frame(px(rng, half, sfull, scur))
                out = fac.frame(blank(half, tfull), out=True, cmp="f16" if half else "f32")
                entry = cvs.cvs_chroma_key_f16_dev if half else cvs.cvs_chroma_key_f32_dev
                return entry(out.ref(), src.ref(), C.byref(params), None)
            cases.append(("key %dx%d %r" % (width, height, (sfull, scur, tfull)), case))
    _run_all(cvs, cases)


# ------------------------------------------------------------------ matte: the LDS halo at the buffer's edge

ROUGH25 = np.array([0.01 * (1 + (k * 7) % 5) for k in range(25)], np.float32)
ROUGH25 = (ROUGH25 / ROUGH25.sum()).astype(np.float32)


@pytest.mark.parametrize("width", [63, 64, 65, 129])
@pytest.mark.parametrize("half", [True, False], ids=["f16", "f32"])
def test_matte(cvs, flavour, half, width):
    """Source window = the whole buffer: every halo pixel of the border tiles lies outside the allocation."""
    cases = []
    for height in (5, 36):
        for choke in (0, 16, -16):
            for feather in (None, ROUGH25):
                if height == 5 and (choke == 0) != (feather is None):
                    continue                                           # the small height: nothing at all, and everything
                full = (0, 0, width - 1, height - 1)
                m = _lib.matte(choke, feather, 0.1, 0.9)

                def case(fac, full=full, m=m):
                    rng = np.random.default_rng(800 + width)
                    src = fac.frame(px(rng, half, full))
                    out = fac.frame(blank(half, full), out=True, cmp="f16" if half else "f32")
                    entry = cvs.cvs_matte_refine_f16_dev if half else cvs.cvs_matte_refine_f32_dev
                    return entry(out.ref(), src.ref(), C.byref(m), None)
                cases.append(("matte %dx%d choke %d feather %d" % (width, height, choke, 0 if feather is None else 25), case))
    _run_all(cvs, cases)


# ------------------------------------------------------------------ transform: clamped taps on the buffer's first and last pixel

def _transforms(tw, th, sfull):
    cx, cy = (tw - 1) / 2.0, (th - 1) / 2.0
    sx, sy = (sfull[0] + sfull[2]) / 2.0, (sfull[1] + sfull[3]) / 2.0
    out = [("half-pixel shift", (1.0, 0.0, 0.5, 0.0, 1.0, 0.5))]
    for name, deg in (("30 degrees", 30.0), ("90 degrees", 90.0)):
        c, s = (0.0, 1.0) if deg == 90.0 else (math.cos(math.radians(deg)), math.sin(math.radians(deg)))
        out.append((name, (c, -s, sx - c * cx + s * cy, s, c, sy - s * cx - c * cy)))
    return out


@pytest.mark.parametrize("tw", [31, 33, 65])
@pytest.mark.parametrize("half", [True, False], ids=["f16", "f32"])
def test_transform(cvs, flavour, half, tw):
    cases = []
    for th in (7, 9):
        tfull = (0, 0, tw - 1, th - 1)
        sfull = (3, 1, tw - 6, th - 2)                                  # smaller than the target, window = whole buffer
        for name, m in _transforms(tw, th, sfull):
            for filt in (_lib.TRANSFORM_NEAREST, _lib.TRANSFORM_BILINEAR):
                t = _lib.transform(m, filt)

                def case(fac, tfull=tfull, sfull=sfull, t=t):
                    rng = np.random.default_rng(900 + tw + th)
                    src = fac.frame(px(rng, half, sfull))
                    out = fac.frame(blank(half, tfull), out=True, cmp="f16" if half else "f32")
                    entry = cvs.cvs_transform_f16_dev if half else cvs.cvs_transform_f32_dev
                    return entry(out.ref(), src.ref(), C.byref(t), None)
                cases.append(("transform %dx%d %s %s" % (tw, th, name, "bilinear" if filt else "nearest"), case))
    _run_all(cvs, cases)


# ------------------------------------------------------------------ blur, unsharp mask, blur + stack

def _taps(n):
    return synth.gaussian_taps(n | 1, max(1.0, n / 5.0))[:n].copy()


@pytest.mark.parametrize("ntaps", [3, 9, 13, 15, 31, 4, 10])
@pytest.mark.parametrize("half", [True, False], ids=["f16", "f32"])
def test_blur_and_unsharp(cvs, flavour, half, ntaps):
    """Source window = the whole buffer; 3, 9, 13: the register window, two columns per lane where the predicate allows;
    15, 31: k_blur; even counts: the table kernels."""
    taps = _taps(ntaps)
    cases = []
    for width in (130, 131):
        for height in (5, 40):
            full = (0, 0, width - 1, height - 1)

            def blur(fac, full=full):
                src = fac.frame(px(np.random.default_rng(1000 + width), half, full))
                out = fac.frame(blank(half, full), out=True, cmp="f16" if half else "f32")
                entry = cvs.cvs_fir_blur_f16_dev if half else cvs.cvs_fir_blur_f32_dev
                return entry(out.ref(), src.ref(), f32p(taps), ntaps, None)

            def unsharp(fac, full=full):
                src = fac.frame(px(np.random.default_rng(1001 + width), half, full))
                out = fac.frame(blank(half, full), out=True, cmp="f16" if half else "f32")
                entry = cvs.cvs_unsharp_mask_f16_dev if half else cvs.cvs_unsharp_mask_f32_dev
                return entry(out.ref(), src.ref(), f32p(taps), ntaps, C.c_float(0.7), C.c_float(0.01), None)
            cases.append(("blur %d taps %dx%d" % (ntaps, width, height), blur))
            if ntaps % 2:
                cases.append(("unsharp %d taps %dx%d" % (ntaps, width, height), unsharp))
    _run_all(cvs, cases)


@pytest.mark.parametrize("columns", [None, 1, 2])
@pytest.mark.parametrize("ntaps", [3, 9, 15])
def test_blur_over(cvs, flavour, ntaps, columns):
    """cvs_blur_over_f16_dev with 1 and 3 overlays (each misaligned in turn by the placements) and its batch form."""
    taps = _taps(ntaps)
    mode = {1: _lib.FIR_PATH_ONE_COLUMN, 2: _lib.FIR_PATH_TWO_COLUMNS, None: _lib.FIR_PATH_AUTO}[columns]
    cases = []
    for width, height in ((130, 5), (131, 40), (130, 40)):
        full = (0, 0, width - 1, height - 1)
        for nover in (1, 3):
            def single(fac, full=full, nover=nover):
                rng = np.random.default_rng(1100 + width)
                src = fac.frame(px16(rng, full), name="blur source")
                ov = [fac.frame(px16(rng, full), name="overlay %d" % k) for k in range(nover)]
                out = fac.frame(blank(True, full), out=True, cmp="f16", name="blur output")
                return cvs.cvs_blur_over_f16_dev(out.ref(), src.ref(), f32p(taps), ntaps, _table(ov), nover, None)
            cases.append(("blur over, %d taps, %d overlays, %dx%d" % (ntaps, nover, width, height), single))

        def batch(fac, full=full):
            rng = np.random.default_rng(1150 + width)
            srcs = [fac.frame(px16(rng, full), name="blur source %d" % k) for k in range(3)]
            ovs = [fac.frame(px16(rng, full), name="overlay of frame %d" % k) for k in range(3)]
            outs = [fac.frame(blank(True, full), out=True, cmp="f16", name="blur output %d" % k) for k in range(3)]
            return cvs.cvs_blur_over_f16_batch_dev(_table(outs), _table(srcs), f32p(taps), ntaps, _table(ovs), 1, 3, None)
        cases.append(("blur over batch, %d taps, %dx%d" % (ntaps, width, height), batch))
    cvs.cvs_fir_path_override(mode)
    try:
        _run_all(cvs, cases)
    finally:
        cvs.cvs_fir_path_override(_lib.FIR_PATH_AUTO)


# ------------------------------------------------------------------ Lanczos

_PINS = {None: _lib.FIR_PATH_AUTO, "hv": _lib.FIR_PATH_TABLES | _lib.FIR_PATH_HV, "passes": _lib.FIR_PATH_TABLES | _lib.FIR_PATH_PASSES,
         "tiled": _lib.FIR_PATH_TABLES | _lib.FIR_PATH_TILED, "strips": _lib.FIR_PATH_STRIPS, "tiles": _lib.FIR_PATH_TILES,
         "one column": _lib.FIR_PATH_ONE_COLUMN, "two columns": _lib.FIR_PATH_TWO_COLUMNS}


@pytest.mark.parametrize("pin", [None, "hv", "passes", "tiled"])
@pytest.mark.parametrize("ssize,tsize,fx,fy", [((130, 40), (65, 20), 0.5, 0.5), ((131, 41), (66, 21), 0.5, 0.5), ((130, 40), (52, 14), 0.4, 0.35),
                                               ((64, 20), (128, 30), 2.0, 1.5)])
def test_lanczos_resample(cvs, flavour, pin, ssize, tsize, fx, fy):
    sfull, tfull = (0, 0, ssize[0] - 1, ssize[1] - 1), (0, 0, tsize[0] - 1, tsize[1] - 1)
    cases = []
    for half in (True, False):
        def case(fac, half=half):
            src = fac.frame(px(np.random.default_rng(1200), half, sfull))
            out = fac.frame(blank(half, tfull), out=True, cmp="f16" if half else "f32")
            entry = cvs.cvs_resample_lanczos_f16_dev if half else cvs.cvs_resample_lanczos_f32_dev
            return entry(out.ref(), src.ref(), C.c_float(fx), C.c_float(fy), 3, None)
        cases.append(("lanczos %s %r -> %r pinned %r" % ("f16" if half else "f32", ssize, tsize, pin), case))
    cvs.cvs_fir_path_override(_PINS[pin])
    try:
        _run_all(cvs, cases)
    finally:
        cvs.cvs_fir_path_override(_lib.FIR_PATH_AUTO)


@pytest.mark.parametrize("pin", [None, "one column", "two columns"])
@pytest.mark.parametrize("ntaps", [1, 5, 13])
def test_blur_lanczos(cvs, flavour, ntaps, pin):
    """Factor 1/2 on both axes: the halving sweeps, two source columns per lane (pinned, or where the predicate allows) and
    one; 13 taps: no one-sweep form.  Single calls and the batch form; 0.4 x 0.35 goes through the table kernels."""
    taps = np.array([1.0], np.float32) if ntaps == 1 else _taps(ntaps)
    cases = []
    for ssize, tsize, fx, fy in [((200, 18), (100, 9), 0.5, 0.5), ((131, 41), (66, 21), 0.5, 0.5), ((130, 40), (52, 14), 0.4, 0.35)]:
        sfull, tfull = (0, 0, ssize[0] - 1, ssize[1] - 1), (0, 0, tsize[0] - 1, tsize[1] - 1)

        def single(fac, sfull=sfull, tfull=tfull, fx=fx, fy=fy):
            src = fac.frame(px16(np.random.default_rng(1300), sfull))
            out = fac.frame(blank(True, tfull), out=True, cmp="f16")
            return cvs.cvs_blur_lanczos_f16_dev(out.ref(), src.ref(), f32p(taps), ntaps, C.c_float(fx), C.c_float(fy), 3, None)

        def batch(fac, sfull=sfull, tfull=tfull, fx=fx, fy=fy):
            rng = np.random.default_rng(1301)
            srcs = [fac.frame(px16(rng, sfull), name="source %d" % k) for k in range(3)]
            outs = [fac.frame(blank(True, tfull), out=True, cmp="f16", name="target %d" % k) for k in range(3)]
            return cvs.cvs_blur_lanczos_f16_batch_dev(_table(outs), _table(srcs), 3, f32p(taps), ntaps, C.c_float(fx), C.c_float(fy), 3, None)
        cases += [("blur + lanczos %d taps %r -> %r pinned %r" % (ntaps, ssize, tsize, pin), single),
                  ("blur + lanczos batch %d taps %r -> %r pinned %r" % (ntaps, ssize, tsize, pin), batch)]
    cvs.cvs_fir_path_override(_PINS[pin])
    try:
        _run_all(cvs, cases)
    finally:
        cvs.cvs_fir_path_override(_lib.FIR_PATH_AUTO)


# ------------------------------------------------------------------ the bilinear scaler

# (factors, target size, pin, the kernel a 16-byte-aligned f16 target implies, the one any other target implies; None: not told apart)
SCALE_CASES = [
    ((2.0, 2.0), (260, 21), "tiles", _lib.FIR_KERNEL_TILE_VH, _lib.FIR_KERNEL_VH),     # the tile kernel: one 16-byte store per pair of halfs
    ((1.5, 1.5), (258, 19), "tiles", _lib.FIR_KERNEL_TILE_VH, _lib.FIR_KERNEL_VH),
    ((2.0, 2.0), (1026, 5), "strips", _lib.FIR_KERNEL_VH, _lib.FIR_KERNEL_VH),         # two pixels per lane on the strips (same kernel id either way)
    ((2.0, 2.0), (1025, 5), "strips", _lib.FIR_KERNEL_VH, _lib.FIR_KERNEL_VH),         # an odd pitch
    ((2.0, 2.0), (260, 21), None, None, None),
    ((0.5, 0.5), (65, 20), None, None, None),
    ((0.75, 1.5), (99, 30), None, None, None),                                         # horizontal first
    ((0.4, 0.35), (52, 14), None, None, None),                                         # two passes
]


@pytest.mark.parametrize("fac_,tsize,pin,k_aligned,k_other", SCALE_CASES)
@pytest.mark.parametrize("half", [True, False], ids=["f16", "f32"])
def test_scale_bilinear(cvs, flavour, half, fac_, tsize, pin, k_aligned, k_other):
    tw, th = tsize
    sw, sh = int(tw / fac_[0]) + 2, int(th / fac_[1]) + 2
    sfull, tfull = (0, 0, sw - 1, sh - 1), (0, 0, tw - 1, th - 1)
    cls = _lib.rgba_frame_f16_t if half else _lib.rgba_frame_f32_t

    def single(fac):
        src = fac.frame(px(np.random.default_rng(1400), half, sfull))
        out = fac.frame(blank(half, tfull), out=True, cmp="f16" if half else "f32")
        entry = cvs.cvs_scale_bilinear_f16_dev if half else cvs.cvs_scale_bilinear_f32_dev
        rc = entry(out.ref(), v2f(0, 0), src.ref(), v2f(0, 0), v2f(*fac_), None)
        if k_aligned is not None:
            tiles_ok = not half or (fac.aligned16(out) and tw % 2 == 0)
            assert cvs.cvs_fir_last_kernel() == (k_aligned if tiles_ok else k_other), (cvs.cvs_fir_last_kernel(), out.ptr & 15)
        return rc

    def batch(fac):
        rng = np.random.default_rng(1401)
        srcs = [fac.frame(px(rng, half, sfull), name="source %d" % k) for k in range(3)]
        outs = [fac.frame(blank(half, tfull), out=True, cmp="f16" if half else "f32", name="target %d" % k) for k in range(3)]
        entry = cvs.cvs_scale_bilinear_f16_batch_dev if half else cvs.cvs_scale_bilinear_f32_batch_dev
        return entry(_table(outs, cls), v2f(0, 0), _table(srcs, cls), v2f(0, 0), v2f(*fac_), 3, None)
    cvs.cvs_fir_path_override(_PINS[pin])
    try:
        run_case(cvs, "scale %s x%r -> %r pinned %r" % ("f16" if half else "f32", fac_, tsize, pin), single)
        run_case(cvs, "scale batch %s x%r -> %r pinned %r" % ("f16" if half else "f32", fac_, tsize, pin), batch)
    finally:
        cvs.cvs_fir_path_override(_lib.FIR_PATH_AUTO)


# ------------------------------------------------------------------ coded planes: DV and MPEG-2

DV_W, DV_H = 720, 480
PLANE_PADS = [(0, 0, 0), (13, 5, 64), (1, 1, 0)]


def _image(ptrs, strides, lines):
    img = _lib.coded_image()
    for p in range(3):
        img.data[p], img.stride[p], img.line_count[p] = ptrs[p], strides[p], lines[p]
    return img


@pytest.mark.parametrize("pads", PLANE_PADS)
def test_dv(cvs, flavour, pads):
    """The DV raster is fixed (720 x 480, first line at y = -1); the frames over it are small: 2 x 4, 130 x 8, 64 x 36, and the
    raster's last rows and columns."""
    strides = [DV_W + pads[0], DV_W // 4 + pads[1], DV_W // 4 + pads[2]]
    rng = np.random.default_rng(1500)
    planes = [rng.integers(0, 256, (DV_H, s), dtype=np.uint8) for s in strides]
    cases = []
    for full in [(0, -1, 1, 2), (3, 1, 132, 8), (0, -1, 63, 34), (655, 470, 719, 478), (650, 440, 730, 490)]:
        def reconstruct(fac, full=full):
            ptrs = [fac.buffer(p, "plane", name="plane %d" % k) for k, p in enumerate(planes)]
            out = fac.frame(blank(True, full), out=True, cmp="f16")
            return cvs.cvs_reconstruct_dv_dev(out.ref(), C.byref(_image(ptrs, strides, [DV_H] * 3)), None)

        def subsample(fac, full=full):
            cur = (full[0] + 1, full[1], full[2], full[3]) if full[2] - full[0] > 2 else full
            frame = fac.frame(px16(np.random.default_rng(1501), full, cur))
            ptrs = [fac.buffer(np.full((DV_H, s), PAD, np.uint8), "plane", out=True, name="plane %d" % k) for k, s in enumerate(strides)]
            return cvs.cvs_subsample_dv_dev(C.byref(_image(ptrs, strides, [DV_H] * 3)), frame.ref(), 0, None)
        cases += [("DV reconstruct %r pads %r" % (full, pads), reconstruct), ("DV subsample %r pads %r" % (full, pads), subsample)]
    _run_all(cvs, cases)


@pytest.mark.parametrize("pads,extra", [((0, 0, 0), (0, 0, 0)), ((13, 5, 64), (2, 1, 3)), ((1, 1, 0), (0, 0, 1))])
@pytest.mark.parametrize("width,height", [(2, 4), (130, 8), (64, 36)])
def test_mpeg2(cvs, flavour, width, height, pads, extra):
    strides = [width + pads[0], width // 2 + pads[1], width // 2 + pads[2]]
    lines = [height + extra[0], height // 2 + extra[1], height // 2 + extra[2]]
    rng = np.random.default_rng(1600 + width)
    planes = [rng.integers(0, 256, (n, s), dtype=np.uint8) for n, s in zip(lines, strides)]
    cases = []
    for full in [(0, 0, width - 1, height - 1), (-3, -1, width + 1, height), (1, 1, width - 1, height - 1)]:
        for flags in (0, _lib.YCC_PROGRESSIVE | _lib.YCC_REC709):
            def reconstruct(fac, full=full, flags=flags):
                ptrs = [fac.buffer(p, "plane", name="plane %d" % k) for k, p in enumerate(planes)]
                out = fac.frame(blank(True, full), out=True, cmp="f16")
                return cvs.cvs_reconstruct_mpeg2_dev(out.ref(), C.byref(_image(ptrs, strides, lines)), width, height, flags, None)
            cases.append(("MPEG-2 reconstruct %dx%d %r flags %d" % (width, height, full, flags), reconstruct))

        def subsample(fac, full=full):
            cur = (max(full[0], 0) + (1 if width > 2 else 0), max(full[1], 0), min(full[2], width - 1), min(full[3], height - 1))
            frame = fac.frame(px16(np.random.default_rng(1601), full, cur))
            ptrs = [fac.buffer(np.full((n, s), PAD, np.uint8), "plane", out=True, name="plane %d" % k) for k, (n, s) in enumerate(zip(lines, strides))]
            return cvs.cvs_subsample_mpeg2_dev(C.byref(_image(ptrs, strides, lines)), frame.ref(), width, height, None)
        cases.append(("MPEG-2 subsample %dx%d %r" % (width, height, full), subsample))
    _run_all(cvs, cases)


# ------------------------------------------------------------------ display bytes

DISPLAY_GEOMETRIES = [((0, 0, 255, 71), (0, 0, 255, 71)), ((0, 0, 254, 70), (0, 0, 254, 70)), ((-3, -2, 200, 90), (5, 1, 150, 77)),
                      ((0, 0, 9, 9), (4, 4, 4, 4))]


@pytest.mark.parametrize("pre", [_lib.LUT_NONE, _lib.LUT_LINEAR_TO_SRGB])
def test_display_bytes(cvs, flavour, pre):
    cases = []
    for full, cur in DISPLAY_GEOMETRIES:
        n = (cur[2] - cur[0] + 1) * (cur[3] - cur[1] + 1) * 4

        def make(call, what):
            def case(fac, full=full, cur=cur, n=n):
                h, w = _box(full)
                codes = (np.arange(h * w * 4, dtype=np.uint64) * 40503 % 65536).astype(np.uint16).reshape(h, w, 4)
                frame = fac.frame(HostFrame(full, np.uint16, codes, cur))
                out = fac.buffer(np.full(n, PAD, np.uint8), "bytes", out=True, name="byte target")
                return call(out, frame)
            return ("%s %r" % (what, (full, cur)), case)
        for mode in (_lib.DISPLAY_RGBA8, _lib.DISPLAY_ARGB32_PREMUL):
            cases.append(make(lambda out, f, mode=mode: cvs.cvs_frame_to_bytes_dev(out, f.ref(), pre, mode, None), "frame to bytes, mode %d" % mode))
        cases.append(make(lambda out, f: cvs.cvs_frame_to_rgba8_intent_dev(out, f.ref(), pre, C.c_float(1.25), None), "frame to rgba8, intent 1.25"))
    _run_all(cvs, cases)
