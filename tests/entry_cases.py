"""The catalogue of device-entry calls: one well-chosen call of every `cvs_*_dev` entry point (and of the workspace's device
slot), on small frames with special values among the pixels and a sentinel in every pixel of every target.

A case is a function case(fac) that makes ONE call on operands it takes from a factory `fac` -- frames through fac.frame(),
coded planes and flat arrays through fac.buffer(), in the same order every time -- on the stream fac.stream, and returns the
entry's return code.  What a case is run ON is the factory's business, so the same call can be made on frames with allocations
of their own (Twin, below), on frames packed into a guarded arena (tests/test_placement_gpu.py) and through an earlier call's
operands again while a stream is capturing (tests/test_graph_replay_gpu.py).  One function per group of entries returns
[(what, case), ...]; GROUPS lists every group at every parameter the GPU modules run it at, and tests/test_entry_cases_cpu.py
holds that list to include/canvas_hip.h without a GPU."""
import ctypes as C
import math

import numpy as np

from canvas_amd import _lib, synth
from canvas_amd.abi import GET_FRAME_F16, GET_FRAME_F32, HostFrame, box2i, v2f, video_frame_source_funcs, video_source
from tests.util import f32p

SENT16 = np.array([0x7E17, 0x1234, 0xFBCD, 0x0001], np.uint16)
SENT32 = np.array([1234.5, -7.25, 3.0e-5, 0.4375], np.float32)
SPECIALS16 = np.array([0x0000, 0x8000, 0x0001, 0x83FF, 0x0400, 0x7BFF, 0xFBFF, 0x7C00, 0xFC00, 0x7E00, 0x7C01, 0x3C00, 0xBC00], np.uint16)
SPECIALS32 = np.array([0.0, -0.0, 1e-42, -3e38, np.inf, -np.inf, np.nan, 1.0, -1.0, 65520.0], np.float32)
REC709_RGB_TO_YPBPR = [0.2126, 0.7152, 0.0722, -0.114572, -0.385428, 0.5, 0.5, -0.454153, -0.045847]
PAD = 0xA5


# ------------------------------------------------------------------ factories

def _box(full):
    return (full[3] - full[1] + 1, full[2] - full[0] + 1)


class _Object:
    def __init__(self, cls, name, out, cmp, nbytes, row_bytes, reads):
        self.cls, self.name, self.out, self.cmp, self.nbytes, self.row_bytes = cls, name, out, cmp, nbytes, row_bytes
        self.reads = reads     # the call reads what the object holds (every input; an output worked on in place)
        self.frame = None      # DeviceFrame, for frames
        self.ptr = None
        self.placed = None


class Factory:
    """What a case asks its operands from.  frame(): a device frame holding `host`'s pixels and window; buffer(): device bytes
    holding `data`.  out=True marks what the call may write; cmp says how an output is compared with the twin's ('exact': code
    for code, 'f16' / 'f32': canonical codes); in_place=True marks an output the call also reads.  An input must come back
    unwritten.  `stream` is what the case hands its entry as the stream argument."""

    def __init__(self, cvs, stream=None):
        self.cvs = cvs
        self.stream = stream
        self.objects = []

    def frame(self, host, out=False, cmp="exact", name=None, in_place=False):
        cls = "f16" if host.dtype == np.uint16 else "f32"
        o = _Object(cls, name or "%s %s %d" % ("output" if out else "input", cls, len(self.objects)), out, cmp, host.array.nbytes,
                    host.array.shape[1] * 4 * host.dtype.itemsize, in_place or not out)
        self.objects.append(o)
        self._make_frame(o, host)
        return o.frame

    def buffer(self, data, cls, out=False, name=None):
        data = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        o = _Object(cls, name or "%s %s %d" % ("output" if out else "input", cls, len(self.objects)), out, "exact", data.size, 0, not out)
        self.objects.append(o)
        self._make_buffer(o, data)
        return o.ptr

    def aligned16(self, *frames):
        return all((f.ptr & 15) == 0 for f in frames)

    # explicit geometry: every window, point and transform a case hands its entry beside the frames goes through these, so
    # that a factory which moves the frames (Shifted, below) can move it with them
    def box(self, x0, y0, x1, y1):
        return box2i.of(x0, y0, x1, y1)

    def point(self, x, y, source=False):
        """A v2f in the target's coordinates, or (source=True) in the source's."""
        return v2f(x, y)

    def matrix(self, m):
        """The six coefficients of a cvs_transform: target coordinates -> source coordinates."""
        return tuple(m)


class Twin(Factory):
    """Every object in an allocation of its own."""

    def _make_frame(self, o, host):
        from canvas_amd.device import DeviceFrame
        o.frame = DeviceFrame.from_host(host)
        o.ptr = o.frame.ptr

    def _make_buffer(self, o, data):
        o.ptr = self.cvs.cvs_malloc(max(data.size, 1))
        assert o.ptr
        if data.size:
            _lib.check(self.cvs.cvs_memcpy_h2d(o.ptr, data.ctypes.data, data.size, None), "h2d")

    def collect(self):
        _lib.check(self.cvs.cvs_stream_sync(self.stream), "sync")
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


def copies_and_conversions(cvs):
    cases = []
    for g, (ofull, ifull, icur) in enumerate(COPY_GEOMETRIES):
        def make(entry, out_half, in_half, cmp, extra=(), g=g, ofull=ofull, ifull=ifull, icur=icur):
            def case(fac):
                rng = np.random.default_rng(100 + g)
                src = fac.frame(px(rng, in_half, ifull, icur))
                out = fac.frame(blank(out_half, ofull), out=True, cmp=cmp)
                return getattr(cvs, entry)(out.ref(), src.ref(), *extra, fac.stream)
            return ("%s %r" % (entry, (ofull, ifull, icur)), case)
        cases += [make("cvs_copy_frame_f16_dev", True, True, "exact"),
                  make("cvs_copy_frame_alpha_f32_dev", False, False, "f32", (C.c_float(0.4),)),
                  make("cvs_copy_frame_alpha_f32_dev", False, False, "f32", (C.c_float(1.0),)),
                  make("cvs_frame_f16_to_f32_dev", False, True, "f32"),
                  make("cvs_frame_f32_to_f16_dev", True, False, "f16"),
                  make("cvs_gain_offset_f16_dev", True, True, "f16", (C.c_float(1.5), C.c_float(0.0625)))]
    return cases


def attenuate_in_place(cvs):
    """video_attenuate_f32's device form: cvs_copy_frame_alpha_f32_dev with the frame as its own source."""
    cases = []
    for full, cur in [((0, 0, 15, 8), (0, 0, 15, 8)), ((0, 0, 128, 8), (1, 0, 128, 8)), ((-4, -4, 20, 12), (-2, -3, 18, 11))]:
        for alpha in (0.4, 1.0, 0.0):
            def case(fac, full=full, cur=cur, alpha=alpha):
                f = fac.frame(px32(np.random.default_rng(150), full, cur), out=True, cmp="f32", in_place=True)
                return cvs.cvs_copy_frame_alpha_f32_dev(f.ref(), f.ref(), C.c_float(alpha), fac.stream)
            cases.append(("attenuate %r alpha %r" % ((full, cur), alpha), case))
    return cases


WEAVE_GEOMETRIES = [
    ((0, 0, 31, 17), (0, 0, 31, 17), (0, 0, 31, 17)),          # full, current, the other field's current: whole frame
    ((0, -1, 128, 16), (0, -1, 128, 16), (0, -1, 128, 16)),    # odd width, first line at y = -1
    ((-4, -3, 40, 20), (3, 2, 29, 14), (3, 2, 29, 14)),        # min.x > 0: the reference's row address starts 3 pixels early
    ((-8, -3, 40, 20), (-5, 2, 20, 9), (-5, 2, 20, 9)),        # min.x < 0: it starts 5 pixels late and runs into the next row
    ((-8, -3, 40, 9), (-5, 2, 40, 9), (-5, 2, 40, 9)),         # ... in the buffer's LAST rows, up to its last column
    ((0, 0, 31, 17), (0, 0, 31, 17), (4, 3, 20, 9)),
]


def weave_fields(cvs):
    cases = []
    for g, (full, cur, ocur) in enumerate(WEAVE_GEOMETRIES):
        def case(fac, g=g, full=full, cur=cur, ocur=ocur):
            rng = np.random.default_rng(200 + g)
            frame = fac.frame(px16(rng, full, cur), out=True, in_place=True)
            other = fac.frame(px16(rng, cur, ocur))
            return cvs.cvs_weave_fields_f16_dev(frame.ref(), other.ref(), fac.stream)
        cases.append(("weave %r" % ((full, cur, ocur),), case))
    return cases


def solid_fills(cvs):
    color = _lib.rgba_f32(1.0, 0.5, 0.333333, 0.2)
    cases = []
    for full, win in [((-5, -5, 5, 6), (-3, -3, 1, 4)), ((0, 0, 128, 6), (0, 0, 128, 6)), ((0, 0, 128, 6), (1, 0, 128, 6)),
                      ((0, 0, 129, 6), (1, 1, 128, 5)), ((0, 0, 3, 3), (-2, -2, 9, 9)), ((0, 0, 0, 0), (0, 0, 0, 0))]:
        for half in (True, False):
            def case(fac, full=full, win=win, half=half):
                f = fac.frame(blank(half, full), out=True)
                b = fac.box(*win)
                entry = cvs.cvs_fill_solid_f16_dev if half else cvs.cvs_fill_solid_f32_dev
                return entry(f.ref(), C.byref(b), C.byref(color), fac.stream)
            cases.append(("fill %s %r" % ("f16" if half else "f32", (full, win)), case))
    return cases


COLOUR_MATRIX_TABLES = [(-1, -1), (0, 2)]


def colour_matrix(cvs, pre, post):
    m = np.array(REC709_RGB_TO_YPBPR, np.float32)
    cases = []
    for full, cur in [((0, 0, 63, 35), (0, 0, 63, 35)), ((0, 0, 62, 34), (0, 0, 62, 34)), ((-3, -2, 60, 33), (0, 0, 57, 30)),
                      ((0, 0, 128, 6), (1, 0, 128, 6)), ((0, 0, 1, 0), (0, 0, 1, 0))]:
        def in_place(fac, full=full, cur=cur):
            f = fac.frame(px16(np.random.default_rng(300), full, cur), out=True, cmp="f16", in_place=True)
            return cvs.cvs_color_matrix_f16_dev(f.ref(), f32p(m), pre, post, fac.stream)
        cases.append(("colour matrix in place %r" % ((full, cur),), in_place))
    for ofull, ifull, icur in [((0, 0, 63, 35), (0, 0, 63, 35), (0, 0, 63, 35)), ((0, 0, 62, 34), (0, 0, 62, 34), (0, 0, 62, 34)),
                               ((-2, -2, 50, 30), (0, 0, 63, 35), (3, 1, 60, 33)), ((0, 0, 128, 6), (0, 0, 128, 6), (1, 0, 128, 6))]:
        def to(fac, ofull=ofull, ifull=ifull, icur=icur):
            src = fac.frame(px16(np.random.default_rng(301), ifull, icur))
            out = fac.frame(blank(True, ofull), out=True, cmp="f16")
            return cvs.cvs_color_matrix_f16_to_dev(out.ref(), src.ref(), f32p(m), pre, post, fac.stream)
        cases.append(("colour matrix out of place %r" % ((ofull, ifull, icur),), to))
    return cases


# ------------------------------------------------------------------ mixers

FULL = (0, 0, 23, 11)
MIXER_FULLS = [FULL, (0, 0, 22, 11)]
MIX_WINDOWS = [(FULL, FULL), (FULL, (3, 2, 10, 6)), ((2, 1, 12, 7), (6, 4, 20, 10)),
               ((6, 4, 20, 10), (2, 1, 12, 7)),            # the `left` selector quirk: addresses before the rows they belong to
               ((0, 5, 12, 9), (5, 0, 20, 7)), ((1, 1, 6, 3), (9, 6, 14, 9)), ((4, 0, 9, 11), (0, 3, 23, 8)),
               ((0, 0, 23, 3), (1, 8, 23, 11))]             # first rows against last rows, up to the last pixel


def mixers_f32(cvs, full):
    cases = []
    for g, (pw, qw) in enumerate(MIX_WINDOWS):
        pw, qw = [tuple(min(v, full[2]) if k == 2 else v for k, v in enumerate(w)) for w in (pw, qw)]

        def over(fac, g=g, pw=pw, qw=qw):
            rng = np.random.default_rng(400 + g)
            out = fac.frame(px32(rng, full, pw), out=True, cmp="f32", in_place=True)
            upper = fac.frame(px32(rng, full, qw))
            return cvs.cvs_mix_over_f32_dev(out.ref(), upper.ref(), C.c_float(0.35), fac.stream)

        def cross(fac, g=g, pw=pw, qw=qw):
            rng = np.random.default_rng(450 + g)
            a, b = fac.frame(px32(rng, full, pw)), fac.frame(px32(rng, full, qw))
            out = fac.frame(blank(False, full), out=True, cmp="f32")
            return cvs.cvs_mix_cross_f32_dev(out.ref(), a.ref(), b.ref(), C.c_float(0.2), fac.stream)
        cases += [("mix over %r" % ((pw, qw),), over), ("mix cross %r" % ((pw, qw),), cross)]
    return cases


def mix_cross_f16(cvs):
    cases = []
    for size in [(96, 54), (33, 7), (1, 1), (2, 1)]:
        full = (0, 0, size[0] - 1, size[1] - 1)

        def whole(fac, full=full):
            rng = np.random.default_rng(500)
            a, b = fac.frame(px16(rng, full)), fac.frame(px16(rng, full))
            out = fac.frame(blank(True, full), out=True, cmp="f16")
            return cvs.cvs_mix_cross_f16_dev(out.ref(), a.ref(), b.ref(), C.c_float(0.3), fac.stream)
        cases.append(("cross f16 %r" % (size,), whole))
    for g, (pw, qw) in enumerate(MIX_WINDOWS):
        def windowed(fac, g=g, pw=pw, qw=qw):
            rng = np.random.default_rng(520 + g)
            a, b = fac.frame(px16(rng, FULL, pw)), fac.frame(px16(rng, FULL, qw))
            out = fac.frame(blank(True, FULL), out=True, cmp="f16")
            return cvs.cvs_mix_cross_f16_dev(out.ref(), a.ref(), b.ref(), C.c_float(0.3), fac.stream)
        cases.append(("cross f16 %r" % ((pw, qw),), windowed))
    return cases


# ------------------------------------------------------------------ the fused chain

CHAIN_SIZES = [(64, 36), (2, 1)]
CHAIN_LAYERS = [1, 2, 4, 5, 7, 8]


def chain(cvs, size, nlayers, plain, after=None):
    """One job.  after(fac, out, layers), when given, runs right after the call (what a module asserts about how it ran)."""
    w, h = size
    m = None if plain else np.array(REC709_RGB_TO_YPBPR, np.float32)
    pre = _lib.LUT_NONE if plain else _lib.LUT_REC709_TO_LINEAR_SCENE
    layers = [synth.layer_frame(w, h, k, 0) for k in range(nlayers)]

    def case(fac):
        dl = [fac.frame(l, name="layer %d" % k) for k, l in enumerate(layers)]
        out = fac.frame(blank(True, (0, 0, w - 1, h - 1)), out=True, cmp="f16", name="chain output")
        jobs = (_lib.chain_job * 1)()
        jobs[0].out = C.pointer(out.c)
        for k, l in enumerate(dl):
            jobs[0].layers[k] = C.pointer(l.c)
        jobs[0].nlayers = nlayers
        rc = cvs.cvs_chain_color_over_f16_dev(jobs, 1, None if m is None else f32p(m), pre, _lib.LUT_NONE, fac.stream)
        if after is not None:
            after(fac, out, dl)
        return rc
    return [("chain %dx%d, %d layers%s" % (w, h, nlayers, ", plain" if plain else ""), case)]


def chain_batches(cvs):
    """Several jobs in one call: frames of one size with both tables (tests/test_gpu_parity.py
    test_chain_batch_and_lut_variants), frames of different sizes, odd pixel counts among them, and a ragged job, which sends
    its call node by node through three pooled f32 frames."""
    m = np.array(REC709_RGB_TO_YPBPR, np.float32)

    def make(what, sizes, nlayers, pre, post, windows=None):
        def case(fac):
            jobs = (_lib.chain_job * len(sizes))()
            for j, (w, h) in enumerate(sizes):
                full = (0, 0, w - 1, h - 1)
                layers = [synth.layer_frame(w, h, k, j) for k in range(nlayers)]
                for k, win in enumerate(windows or ()):
                    layers[k] = HostFrame(full, np.uint16, layers[k].array, win)
                dl = [fac.frame(l, name="job %d layer %d" % (j, k)) for k, l in enumerate(layers)]
                out = fac.frame(blank(True, full), out=True, cmp="f16", name="job %d output" % j)
                jobs[j].out = C.pointer(out.c)
                for k, l in enumerate(dl):
                    jobs[j].layers[k] = C.pointer(l.c)
                jobs[j].nlayers = nlayers
            return cvs.cvs_chain_color_over_f16_dev(jobs, len(sizes), f32p(m), pre, post, fac.stream)
        return ("chain batch, %s" % what, case)
    return [make("3 frames of 48x20, no tables", [(48, 20)] * 3, 2, _lib.LUT_NONE, _lib.LUT_NONE),
            make("3 frames of 48x20, both tables", [(48, 20)] * 3, 2, _lib.LUT_REC709_TO_LINEAR_SCENE, _lib.LUT_LINEAR_TO_SRGB),
            make("frames of different sizes", [(64, 36), (33, 7), (1, 2), (513, 1), (3, 1)], 3, _lib.LUT_REC709_TO_LINEAR_SCENE, _lib.LUT_NONE),
            make("a ragged job", [(48, 20)], 3, _lib.LUT_REC709_TO_LINEAR_SCENE, _lib.LUT_NONE, [(0, 0, 47, 19), (5, 3, 30, 15), (20, 2, 47, 10)])]


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


STREAM_WIDTHS = [1, 2, 129, 130]
FIELD_OPS = ["field0", "field1", "soften", "interlace"]


def field_conversions(cvs, op, width):
    cases = []
    for height in (1, 9, 17):
        for g, (sfull, scur, tfull) in enumerate(_stream_geometries(width, height)):
            def case(fac, g=g, sfull=sfull, scur=scur, tfull=tfull):
                rng = np.random.default_rng(600 + g + height)
                a = fac.frame(px16(rng, sfull, scur))
                b = fac.frame(px16(rng, sfull, scur)) if op == "interlace" else None
                out = fac.frame(blank(True, tfull), out=True, cmp="exact" if op == "interlace" else "f16")
                if op == "interlace":
                    return cvs.cvs_interlace_fields_f16_dev(out.ref(), a.ref(), b.ref(), fac.stream)
                if op == "soften":
                    return cvs.cvs_soften_fields_f16_dev(out.ref(), a.ref(), fac.stream)
                return cvs.cvs_field_to_frame_f16_dev(out.ref(), a.ref(), int(op[-1]), fac.stream)
            cases.append(("%s %dx%d %r" % (op, width, height, (sfull, scur, tfull)), case))
    return cases


KEY_SETTINGS = [dict(key=(0.1, 0.8, 0.15), tolerance=0.08, softness=0.25, spill=0.8, spill_range=0.4, flags=0),
                dict(key=(0.9, -0.1, 1.2), tolerance=0.0, softness=0.1, spill=0.5, spill_range=0.3, flags=_lib.KEY_SHOW_MATTE)]


def chroma_key(cvs, half, width):
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
                return entry(out.ref(), src.ref(), C.byref(params), fac.stream)
            cases.append(("key %dx%d %r" % (width, height, (sfull, scur, tfull)), case))
    return cases


# ------------------------------------------------------------------ matte: the LDS halo at the buffer's edge

ROUGH25 = np.array([0.01 * (1 + (k * 7) % 5) for k in range(25)], np.float32)
ROUGH25 = (ROUGH25 / ROUGH25.sum()).astype(np.float32)
MATTE_WIDTHS = [63, 64, 65, 129]


def matte(cvs, half, width):
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
                    return entry(out.ref(), src.ref(), C.byref(m), fac.stream)
                cases.append(("matte %dx%d choke %d feather %d" % (width, height, choke, 0 if feather is None else 25), case))
    return cases


# ------------------------------------------------------------------ transform: clamped taps on the buffer's first and last pixel

def _transforms(tw, th, sfull):
    cx, cy = (tw - 1) / 2.0, (th - 1) / 2.0
    sx, sy = (sfull[0] + sfull[2]) / 2.0, (sfull[1] + sfull[3]) / 2.0
    out = [("half-pixel shift", (1.0, 0.0, 0.5, 0.0, 1.0, 0.5))]
    for name, deg in (("30 degrees", 30.0), ("90 degrees", 90.0)):
        c, s = (0.0, 1.0) if deg == 90.0 else (math.cos(math.radians(deg)), math.sin(math.radians(deg)))
        out.append((name, (c, -s, sx - c * cx + s * cy, s, c, sy - s * cx - c * cy)))
    return out


TRANSFORM_WIDTHS = [31, 33, 65]


def transform(cvs, half, tw):
    cases = []
    for th in (7, 9):
        tfull = (0, 0, tw - 1, th - 1)
        sfull = (3, 1, tw - 6, th - 2)                                  # smaller than the target, window = whole buffer
        for name, m in _transforms(tw, th, sfull):
            for filt in (_lib.TRANSFORM_NEAREST, _lib.TRANSFORM_BILINEAR):
                def case(fac, tfull=tfull, sfull=sfull, m=m, filt=filt):
                    t = _lib.transform(fac.matrix(m), filt)
                    rng = np.random.default_rng(900 + tw + th)
                    src = fac.frame(px(rng, half, sfull))
                    out = fac.frame(blank(half, tfull), out=True, cmp="f16" if half else "f32")
                    entry = cvs.cvs_transform_f16_dev if half else cvs.cvs_transform_f32_dev
                    return entry(out.ref(), src.ref(), C.byref(t), fac.stream)
                cases.append(("transform %dx%d %s %s" % (tw, th, name, "bilinear" if filt else "nearest"), case))
    return cases


# ------------------------------------------------------------------ blur, unsharp mask, blur + stack

def _taps(n):
    return synth.gaussian_taps(n | 1, max(1.0, n / 5.0))[:n].copy()


BLUR_TAPS = [3, 9, 13, 15, 31, 4, 10]


def blur_and_unsharp(cvs, half, ntaps):
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
                return entry(out.ref(), src.ref(), f32p(taps), ntaps, fac.stream)

            def unsharp(fac, full=full):
                src = fac.frame(px(np.random.default_rng(1001 + width), half, full))
                out = fac.frame(blank(half, full), out=True, cmp="f16" if half else "f32")
                entry = cvs.cvs_unsharp_mask_f16_dev if half else cvs.cvs_unsharp_mask_f32_dev
                return entry(out.ref(), src.ref(), f32p(taps), ntaps, C.c_float(0.7), C.c_float(0.01), fac.stream)
            cases.append(("blur %d taps %dx%d" % (ntaps, width, height), blur))
            if ntaps % 2:
                cases.append(("unsharp %d taps %dx%d" % (ntaps, width, height), unsharp))
    return cases


BLUR_OVER_TAPS = [3, 9, 15]
COLUMN_PINS = {1: _lib.FIR_PATH_ONE_COLUMN, 2: _lib.FIR_PATH_TWO_COLUMNS, None: _lib.FIR_PATH_AUTO}


def blur_over(cvs, ntaps):
    """cvs_blur_over_f16_dev with 1 and 3 overlays and its batch form (run under each of COLUMN_PINS)."""
    taps = _taps(ntaps)
    cases = []
    for width, height in ((130, 5), (131, 40), (130, 40)):
        full = (0, 0, width - 1, height - 1)
        for nover in (1, 3):
            def single(fac, full=full, nover=nover):
                rng = np.random.default_rng(1100 + width)
                src = fac.frame(px16(rng, full), name="blur source")
                ov = [fac.frame(px16(rng, full), name="overlay %d" % k) for k in range(nover)]
                out = fac.frame(blank(True, full), out=True, cmp="f16", name="blur output")
                return cvs.cvs_blur_over_f16_dev(out.ref(), src.ref(), f32p(taps), ntaps, _table(ov), nover, fac.stream)
            cases.append(("blur over, %d taps, %d overlays, %dx%d" % (ntaps, nover, width, height), single))

        def batch(fac, full=full):
            rng = np.random.default_rng(1150 + width)
            srcs = [fac.frame(px16(rng, full), name="blur source %d" % k) for k in range(3)]
            ovs = [fac.frame(px16(rng, full), name="overlay of frame %d" % k) for k in range(3)]
            outs = [fac.frame(blank(True, full), out=True, cmp="f16", name="blur output %d" % k) for k in range(3)]
            return cvs.cvs_blur_over_f16_batch_dev(_table(outs), _table(srcs), f32p(taps), ntaps, _table(ovs), 1, 3, fac.stream)
        cases.append(("blur over batch, %d taps, %dx%d" % (ntaps, width, height), batch))
    return cases


def blur_over_forms(cvs):
    """Blur + over where it is one launch (whole windows, odd lists up to 23 taps, up to four overlays; two strips and one) and
    where it goes node by node through pooled f32 frames: ragged overlays, an even list, five overlays, none, a source window
    inside its buffer -- the shapes of tests/test_gpu_parity.py test_blur_over_fused and test_blur_over_node_by_node."""
    cases = []

    def make(what, full, scur, ntaps, wins):
        taps = synth.gaussian_taps(ntaps | 1, 1.5)[:ntaps].copy()

        def case(fac):
            rng = np.random.default_rng(1180 + ntaps + len(wins))
            src = fac.frame(px16(rng, full, scur), name="blur source")
            ov = [fac.frame(px16(rng, full, w), name="overlay %d" % k) for k, w in enumerate(wins)]
            out = fac.frame(blank(True, full), out=True, cmp="f16", name="blur output")
            return cvs.cvs_blur_over_f16_dev(out.ref(), src.ref(), f32p(taps), ntaps, _table(ov), len(wins), fac.stream)
        return ("blur over %s" % what, case)
    for (w, h), ntaps, nover in [((300, 41), 9, 3), ((64, 36), 3, 1), ((300, 41), 23, 4), ((64, 36), 15, 4)]:
        full = (0, 0, w - 1, h - 1)
        cases.append(make("in one launch, %dx%d, %d taps, %d overlays" % (w, h, ntaps, nover), full, full, ntaps, [full] * nover))
    full = (0, 0, 59, 33)
    cases += [make("node by node, ragged overlays", full, full, 9, [(5, 3, 40, 25), (20, 2, 59, 20)]),
              make("node by node, 4 taps", full, full, 4, [full] * 2),
              make("node by node, five overlays", full, full, 9, [full] * 5),
              make("node by node, no overlay", full, full, 9, []),
              make("node by node, a small source window", full, (4, 2, 50, 30), 9, [full] * 2)]
    return cases


# ------------------------------------------------------------------ Lanczos

PINS = {None: _lib.FIR_PATH_AUTO, "hv": _lib.FIR_PATH_TABLES | _lib.FIR_PATH_HV, "passes": _lib.FIR_PATH_TABLES | _lib.FIR_PATH_PASSES,
        "tiled": _lib.FIR_PATH_TABLES | _lib.FIR_PATH_TILED, "strips": _lib.FIR_PATH_STRIPS, "tiles": _lib.FIR_PATH_TILES,
        "one column": _lib.FIR_PATH_ONE_COLUMN, "two columns": _lib.FIR_PATH_TWO_COLUMNS}
LANCZOS_PINS = [None, "hv", "passes", "tiled"]
LANCZOS_SHAPES = [((130, 40), (65, 20), 0.5, 0.5), ((131, 41), (66, 21), 0.5, 0.5), ((130, 40), (52, 14), 0.4, 0.35), ((64, 20), (128, 30), 2.0, 1.5)]


def lanczos_resample(cvs, pin, ssize, tsize, fx, fy):
    sfull, tfull = (0, 0, ssize[0] - 1, ssize[1] - 1), (0, 0, tsize[0] - 1, tsize[1] - 1)
    cases = []
    for half in (True, False):
        def case(fac, half=half):
            src = fac.frame(px(np.random.default_rng(1200), half, sfull))
            out = fac.frame(blank(half, tfull), out=True, cmp="f16" if half else "f32")
            entry = cvs.cvs_resample_lanczos_f16_dev if half else cvs.cvs_resample_lanczos_f32_dev
            return entry(out.ref(), src.ref(), C.c_float(fx), C.c_float(fy), 3, fac.stream)
        cases.append(("lanczos %s %r -> %r pinned %r" % ("f16" if half else "f32", ssize, tsize, pin), case))
    return cases


BLUR_LANCZOS_PINS = [None, "one column", "two columns"]
BLUR_LANCZOS_TAPS = [1, 5, 13]


def blur_lanczos(cvs, ntaps, pin):
    """Factor 1/2 on both axes: the halving sweeps, two source columns per lane (pinned, or where the predicate allows) and
    one; 13 taps: no one-sweep form.  Single calls and the batch form; 0.4 x 0.35 goes through the table kernels."""
    taps = np.array([1.0], np.float32) if ntaps == 1 else _taps(ntaps)
    cases = []
    for ssize, tsize, fx, fy in [((200, 18), (100, 9), 0.5, 0.5), ((131, 41), (66, 21), 0.5, 0.5), ((130, 40), (52, 14), 0.4, 0.35)]:
        sfull, tfull = (0, 0, ssize[0] - 1, ssize[1] - 1), (0, 0, tsize[0] - 1, tsize[1] - 1)

        def single(fac, sfull=sfull, tfull=tfull, fx=fx, fy=fy):
            src = fac.frame(px16(np.random.default_rng(1300), sfull))
            out = fac.frame(blank(True, tfull), out=True, cmp="f16")
            return cvs.cvs_blur_lanczos_f16_dev(out.ref(), src.ref(), f32p(taps), ntaps, C.c_float(fx), C.c_float(fy), 3, fac.stream)

        def batch(fac, sfull=sfull, tfull=tfull, fx=fx, fy=fy):
            rng = np.random.default_rng(1301)
            srcs = [fac.frame(px16(rng, sfull), name="source %d" % k) for k in range(3)]
            outs = [fac.frame(blank(True, tfull), out=True, cmp="f16", name="target %d" % k) for k in range(3)]
            return cvs.cvs_blur_lanczos_f16_batch_dev(_table(outs), _table(srcs), 3, f32p(taps), ntaps, C.c_float(fx), C.c_float(fy), 3, fac.stream)
        cases += [("blur + lanczos %d taps %r -> %r pinned %r" % (ntaps, ssize, tsize, pin), single),
                  ("blur + lanczos batch %d taps %r -> %r pinned %r" % (ntaps, ssize, tsize, pin), batch)]
    return cases


def config3_pipeline(cvs):
    """cvs_blur_lanczos_f16_dev on the shapes of tests/test_gpu_parity.py test_config3_pipeline_f16; the last one does not fit
    an LDS tile and runs the two passes through a pooled f32 frame."""
    taps = synth.gaussian_taps(9, 1.5)
    cases = []
    for ssize, tsize, fx, fy in [((128, 72), (64, 36), 0.5, 0.5), ((97, 55), (49, 28), 0.5, 0.5), ((64, 36), (128, 54), 2.0, 1.5), ((200, 40), (20, 40), 0.1, 1.0)]:
        def case(fac, ssize=ssize, tsize=tsize, fx=fx, fy=fy):
            src = fac.frame(synth.layer_frame(ssize[0], ssize[1], 1, 0))
            out = fac.frame(blank(True, (0, 0, tsize[0] - 1, tsize[1] - 1)), out=True, cmp="f16")
            return cvs.cvs_blur_lanczos_f16_dev(out.ref(), src.ref(), f32p(taps), 9, C.c_float(fx), C.c_float(fy), 3, fac.stream)
        cases.append(("config 3 %r -> %r" % (ssize, tsize), case))
    return cases


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


def scale_bilinear(cvs, half, fac_, tsize, pin, after=None):
    """[single call, batch of three].  after(fac, out), when given, runs right after the single call."""
    tw, th = tsize
    sw, sh = int(tw / fac_[0]) + 2, int(th / fac_[1]) + 2
    sfull, tfull = (0, 0, sw - 1, sh - 1), (0, 0, tw - 1, th - 1)
    cls = _lib.rgba_frame_f16_t if half else _lib.rgba_frame_f32_t

    def single(fac):
        src = fac.frame(px(np.random.default_rng(1400), half, sfull))
        out = fac.frame(blank(half, tfull), out=True, cmp="f16" if half else "f32")
        entry = cvs.cvs_scale_bilinear_f16_dev if half else cvs.cvs_scale_bilinear_f32_dev
        rc = entry(out.ref(), fac.point(0, 0), src.ref(), fac.point(0, 0, source=True), v2f(*fac_), fac.stream)
        if after is not None:
            after(fac, out)
        return rc

    def batch(fac):
        rng = np.random.default_rng(1401)
        srcs = [fac.frame(px(rng, half, sfull), name="source %d" % k) for k in range(3)]
        outs = [fac.frame(blank(half, tfull), out=True, cmp="f16" if half else "f32", name="target %d" % k) for k in range(3)]
        entry = cvs.cvs_scale_bilinear_f16_batch_dev if half else cvs.cvs_scale_bilinear_f32_batch_dev
        return entry(_table(outs, cls), fac.point(0, 0), _table(srcs, cls), fac.point(0, 0, source=True), v2f(*fac_), 3, fac.stream)
    return [("scale %s x%r -> %r pinned %r" % ("f16" if half else "f32", fac_, tsize, pin), single),
            ("scale batch %s x%r -> %r pinned %r" % ("f16" if half else "f32", fac_, tsize, pin), batch)]


# ------------------------------------------------------------------ coded planes: DV and MPEG-2

DV_W, DV_H = 720, 480
PLANE_PADS = [(0, 0, 0), (13, 5, 64), (1, 1, 0)]


def _image(ptrs, strides, lines):
    img = _lib.coded_image()
    for p in range(3):
        img.data[p], img.stride[p], img.line_count[p] = ptrs[p], strides[p], lines[p]
    return img


def dv(cvs, pads):
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
            return cvs.cvs_reconstruct_dv_dev(out.ref(), C.byref(_image(ptrs, strides, [DV_H] * 3)), fac.stream)

        def subsample(fac, full=full):
            cur = (full[0] + 1, full[1], full[2], full[3]) if full[2] - full[0] > 2 else full
            frame = fac.frame(px16(np.random.default_rng(1501), full, cur))
            ptrs = [fac.buffer(np.full((DV_H, s), PAD, np.uint8), "plane", out=True, name="plane %d" % k) for k, s in enumerate(strides)]
            return cvs.cvs_subsample_dv_dev(C.byref(_image(ptrs, strides, [DV_H] * 3)), frame.ref(), 0, fac.stream)
        cases += [("DV reconstruct %r pads %r" % (full, pads), reconstruct), ("DV subsample %r pads %r" % (full, pads), subsample)]
    return cases


MPEG2_PADS = [((0, 0, 0), (0, 0, 0)), ((13, 5, 64), (2, 1, 3)), ((1, 1, 0), (0, 0, 1))]
MPEG2_SIZES = [(2, 4), (130, 8), (64, 36)]


def mpeg2(cvs, width, height, pads, extra):
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
                return cvs.cvs_reconstruct_mpeg2_dev(out.ref(), C.byref(_image(ptrs, strides, lines)), width, height, flags, fac.stream)
            cases.append(("MPEG-2 reconstruct %dx%d %r flags %d" % (width, height, full, flags), reconstruct))

        def subsample(fac, full=full):
            cur = (max(full[0], 0) + (1 if width > 2 else 0), max(full[1], 0), min(full[2], width - 1), min(full[3], height - 1))
            frame = fac.frame(px16(np.random.default_rng(1601), full, cur))
            ptrs = [fac.buffer(np.full((n, s), PAD, np.uint8), "plane", out=True, name="plane %d" % k) for k, (n, s) in enumerate(zip(lines, strides))]
            return cvs.cvs_subsample_mpeg2_dev(C.byref(_image(ptrs, strides, lines)), frame.ref(), width, height, fac.stream)
        cases.append(("MPEG-2 subsample %dx%d %r" % (width, height, full), subsample))
    return cases


# ------------------------------------------------------------------ display bytes

DISPLAY_GEOMETRIES = [((0, 0, 255, 71), (0, 0, 255, 71)), ((0, 0, 254, 70), (0, 0, 254, 70)), ((-3, -2, 200, 90), (5, 1, 150, 77)),
                      ((0, 0, 9, 9), (4, 4, 4, 4))]
DISPLAY_TABLES = [_lib.LUT_NONE, _lib.LUT_LINEAR_TO_SRGB]


def all_codes(full, cur):
    """Every half code in every channel position at least once (from 64 x 64 up)."""
    h, w = _box(full)
    codes = (np.arange(h * w * 4, dtype=np.uint64) * 40503 % 65536).astype(np.uint16).reshape(h, w, 4)
    return HostFrame(full, np.uint16, codes, cur)


def display_bytes(cvs, pre):
    cases = []
    for full, cur in DISPLAY_GEOMETRIES:
        n = (cur[2] - cur[0] + 1) * (cur[3] - cur[1] + 1) * 4

        def make(call, what):
            def case(fac, full=full, cur=cur, n=n):
                frame = fac.frame(all_codes(full, cur))
                out = fac.buffer(np.full(n, PAD, np.uint8), "bytes", out=True, name="byte target")
                return call(out, frame, fac.stream)
            return ("%s %r" % (what, (full, cur)), case)
        for mode in (_lib.DISPLAY_RGBA8, _lib.DISPLAY_ARGB32_PREMUL):
            cases.append(make(lambda out, f, s, mode=mode: cvs.cvs_frame_to_bytes_dev(out, f.ref(), pre, mode, s), "frame to bytes, mode %d" % mode))
        cases.append(make(lambda out, f, s: cvs.cvs_frame_to_rgba8_intent_dev(out, f.ref(), pre, C.c_float(1.25), s), "frame to rgba8, intent 1.25"))
    return cases


# ------------------------------------------------------------------ flat arrays

def flat_arrays(cvs):
    """The five entries on flat arrays: 4099 elements with both buffers off the 16-byte grid (tests/test_gpu_parity.py
    test_flat_dev_entry_points_with_unaligned_buffers) and 7, fewer than one vector."""
    cases = []
    for n in (4099, 7):
        def widen(fac, entry, n=n):
            codes = np.random.default_rng(1700).integers(0, 65536, n + 3).astype(np.uint16)
            src = fac.buffer(codes, "plane", name="half array")
            out = fac.buffer(np.full(4 * (n + 1), PAD, np.uint8), "plane", out=True, name="float array")
            return getattr(cvs, entry)(out + 4, src + 6, n, fac.stream)

        def narrow(fac, entry, n=n):
            values = px32(np.random.default_rng(1701), (0, 0, (n + 1 + 3) // 4 - 1, 0)).array.reshape(-1)[:n + 1]
            src = fac.buffer(values, "plane", name="float array")
            out = fac.buffer(np.full(2 * (n + 3), PAD, np.uint8), "plane", out=True, name="half array")
            return getattr(cvs, entry)(out + 6, src + 4, n, fac.stream)

        def lookup(fac, n=n):
            rng = np.random.default_rng(1702)
            table = fac.buffer(rng.integers(0, 65536, 65536).astype(np.uint16), "plane", name="table")
            src = fac.buffer(rng.integers(0, 65536, n + 3).astype(np.uint16), "plane", name="half array")
            out = fac.buffer(np.full(2 * (n + 1), PAD, np.uint8), "plane", out=True, name="looked-up array")
            return cvs.cvs_half_lookup_dev(table, out + 2, src + 6, n, fac.stream)
        for entry in ("cvs_half_to_float_dev", "cvs_half_to_float_fast_dev"):
            cases.append(("%s, %d elements" % (entry, n), lambda fac, entry=entry, widen=widen: widen(fac, entry)))
        for entry in ("cvs_float_to_half_dev", "cvs_float_to_half_fast_dev"):
            cases.append(("%s, %d elements" % (entry, n), lambda fac, entry=entry, narrow=narrow: narrow(fac, entry)))
        cases.append(("cvs_half_lookup_dev, %d elements" % n, lookup))
    return cases


# ------------------------------------------------------------------ the workspace stack through the device slot

GET_FRAME_DEV = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.POINTER(_lib.rgba_frame_dev))
FORMAT_F16, FORMAT_F32 = 1, 2


def _device_source(cvs, layer, half_native):
    """A video_source whose device slot hands out `layer` (a device frame of halfs): a copy into an f16 target, widened into
    an f32 one, on the stream the puller names.  Its host slots are never reached (video_get_frame_dev goes to slot 3 first);
    they say which formats the source is native in, which is what the workspace picks its form by."""
    def slot(_self, _index, fp):
        d = fp.contents
        if d.format == FORMAT_F16:
            target = _lib.rgba_frame_f16_t(d.data, d.full_window, d.full_window)
            rc = cvs.cvs_copy_frame_f16_dev(C.byref(target), layer.ref(), d.stream)
        else:
            target = _lib.rgba_frame_f32_t(d.data, d.full_window, d.full_window)
            rc = cvs.cvs_frame_f16_to_f32_dev(C.byref(target), layer.ref(), d.stream)
        d.current_window = target.current_window if rc == 0 else box2i.empty()

    def no16(_self, _index, fp):
        fp.contents.current_window = box2i.empty()

    def no32(_self, _index, fp):
        fp.contents.current_window = box2i.empty()
    dev, cb16 = GET_FRAME_DEV(slot), GET_FRAME_F16(no16)
    cb32 = C.cast(None, GET_FRAME_F32) if half_native else GET_FRAME_F32(no32)
    funcs = video_frame_source_funcs(1, cb16, cb32, C.cast(dev, C.c_void_p).value)
    return video_source(None, C.pointer(funcs)), (dev, cb16, cb32, funcs)


def workspace_stack(cvs):
    """The workspace's device slot over three device-resident layers (z order 0, 7, 3; the shapes of tests/test_gpu_parity.py
    test_workspace_stack_host_and_device): half-native sources pulled as f16 (one plain chain call, ragged windows: node by node
    through pooled frames), the same pulled as f32 (into the caller's frame), and sources native in both formats pulled as f16
    (the f32 stack through two pooled frames, then narrowed)."""
    full = (0, 0, 31, 15)
    wins = [full, (4, 2, 20, 12), (10, 1, 31, 9)]
    cases = []
    for half_native, half_target in ((True, True), (True, False), (False, True)):
        def case(fac, half_native=half_native, half_target=half_target):
            rng = np.random.default_rng(1800)
            layers = [fac.frame(px16(rng, full, w), name="layer %d" % k) for k, w in enumerate(wins)]
            out = fac.frame(blank(half_target, full, full), out=True, cmp="f16" if half_target else "f32", name="pulled frame")
            sources = [_device_source(cvs, l, half_native) for l in layers]
            ws = cvs.workspace_create()
            try:
                for (src, _keep), z in zip(sources, (0, 7, 3)):
                    cvs.workspace_add_item(ws, C.cast(C.pointer(src), C.c_void_p), 0, 10, 0, z, None)
                vs = video_source()
                cvs.workspace_as_video_source(ws, C.byref(vs))
                d = _lib.rgba_frame_dev(out.ptr, FORMAT_F16 if half_target else FORMAT_F32, out.c.full_window, out.c.full_window, fac.stream)
                cvs.video_get_frame_dev(C.byref(vs), 4, C.byref(d))
                out.c.current_window = d.current_window
            finally:
                cvs.workspace_free(ws)
            return 0
        cases.append(("workspace stack, %s sources, pulled as %s" % ("half-native" if half_native else "two-format", "f16" if half_target else "f32"), case))
    return cases


# ------------------------------------------------------------------ every group at every parameter

def _groups():
    """(id, FIR path pin, builder): builder(cvs) -> [(what, case), ...], to be run with cvs_fir_path_override(pin) in force."""
    auto = _lib.FIR_PATH_AUTO
    g = [("copies_and_conversions", auto, copies_and_conversions), ("attenuate_in_place", auto, attenuate_in_place),
         ("weave_fields", auto, weave_fields), ("solid_fills", auto, solid_fills)]
    g += [("colour_matrix[%d-%d]" % (pre, post), auto, lambda cvs, pre=pre, post=post: colour_matrix(cvs, pre, post)) for pre, post in COLOUR_MATRIX_TABLES]
    g += [("mixers_f32[%d]" % full[2], auto, lambda cvs, full=full: mixers_f32(cvs, full)) for full in MIXER_FULLS]
    g += [("mix_cross_f16", auto, mix_cross_f16)]
    g += [("chain[%dx%d-%d-%s]" % (size[0], size[1], n, "plain" if plain else "colour"), auto, lambda cvs, size=size, n=n, plain=plain: chain(cvs, size, n, plain))
          for size in CHAIN_SIZES for n in CHAIN_LAYERS for plain in (False, True)]
    g += [("chain_batches", auto, chain_batches)]
    g += [("field_conversions[%s-%d]" % (op, w), auto, lambda cvs, op=op, w=w: field_conversions(cvs, op, w)) for op in FIELD_OPS for w in STREAM_WIDTHS]
    for name, fn, widths in (("chroma_key", chroma_key, STREAM_WIDTHS), ("matte", matte, MATTE_WIDTHS), ("transform", transform, TRANSFORM_WIDTHS)):
        g += [("%s[%s-%d]" % (name, "f16" if half else "f32", w), auto, lambda cvs, fn=fn, half=half, w=w: fn(cvs, half, w)) for half in (True, False) for w in widths]
    g += [("blur_and_unsharp[%s-%d]" % ("f16" if half else "f32", n), auto, lambda cvs, half=half, n=n: blur_and_unsharp(cvs, half, n))
          for half in (True, False) for n in BLUR_TAPS]
    g += [("blur_over[%d-%s]" % (n, columns), COLUMN_PINS[columns], lambda cvs, n=n: blur_over(cvs, n)) for n in BLUR_OVER_TAPS for columns in (None, 1, 2)]
    g += [("blur_over_forms", auto, blur_over_forms)]
    g += [("lanczos_resample[%s-%dx%d-%s]" % (pin, s[0][0], s[0][1], s[2]), PINS[pin], lambda cvs, pin=pin, s=s: lanczos_resample(cvs, pin, *s))
          for pin in LANCZOS_PINS for s in LANCZOS_SHAPES]
    g += [("blur_lanczos[%d-%s]" % (n, pin), PINS[pin], lambda cvs, n=n, pin=pin: blur_lanczos(cvs, n, pin)) for n in BLUR_LANCZOS_TAPS for pin in BLUR_LANCZOS_PINS]
    g += [("config3_pipeline", auto, config3_pipeline)]
    g += [("scale_bilinear[%s-%d]" % ("f16" if half else "f32", k), PINS[c[2]], lambda cvs, half=half, c=c: scale_bilinear(cvs, half, c[0], c[1], c[2]))
          for half in (True, False) for k, c in enumerate(SCALE_CASES)]
    g += [("dv[%d]" % k, auto, lambda cvs, pads=pads: dv(cvs, pads)) for k, pads in enumerate(PLANE_PADS)]
    g += [("mpeg2[%dx%d-%d]" % (w, h, k), auto, lambda cvs, w=w, h=h, p=p: mpeg2(cvs, w, h, p[0], p[1])) for (w, h) in MPEG2_SIZES for k, p in enumerate(MPEG2_PADS)]
    g += [("display_bytes[%d]" % pre, auto, lambda cvs, pre=pre: display_bytes(cvs, pre)) for pre in DISPLAY_TABLES]
    g += [("flat_arrays", auto, flat_arrays), ("workspace_stack", auto, workspace_stack)]
    return g


GROUPS = _groups()


# ------------------------------------------------------------------ far from the origin (DESIGN.md "Coordinates")

MAX_COORD, RESAMPLE_MAX_COORD = _lib.MAX_COORD, _lib.RESAMPLE_MAX_COORD
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def move_box(b, d):
    """(x0, y0, x1, y1) translated by d = (dx, dy); an empty box stays what it is (only emptiness is contractual)."""
    if b[2] < b[0] or b[3] < b[1]:
        return tuple(b)
    return tuple(min(max(v + d[k & 1], INT_MIN), INT_MAX) for k, v in enumerate(b))


class Shifted(Factory):
    """Another factory's operands, moved: every frame's full_window and current_window translated by `offset` -- inputs by
    `source_offset` where a class moves the source by another amount than the target (a resampler at factor f reads source
    column t / f) -- and every explicit box, point and transform with them.  Pixels, coded planes and flat arrays are handed
    on as they are.  The objects are the wrapped factory's (collect them there); windows_back() reports every frame's window
    translated back, to compare with an unmoved run's directly.  `hosts` keeps what each frame() handed on (None for a
    buffer) and `matrices` what matrix() returned, for expectations computed at the far arguments."""

    def __init__(self, inner, offset, source_offset=None):
        Factory.__init__(self, inner.cvs, inner.stream)
        self.inner, self.offset = inner, tuple(offset)
        self.source_offset = self.offset if source_offset is None else tuple(source_offset)
        self.objects = inner.objects
        self.moves, self.hosts, self.matrices = [], [], []

    def frame(self, host, out=False, **kw):
        d = self.offset if out else self.source_offset
        moved = HostFrame(move_box(host.full_window.tuple(), d), host.dtype, host.array, move_box(host.current_window.tuple(), d))
        self.moves.append(d)
        self.hosts.append(moved)
        return self.inner.frame(moved, out=out, **kw)

    def buffer(self, data, cls, **kw):
        self.moves.append(None)
        self.hosts.append(None)
        return self.inner.buffer(data, cls, **kw)

    def box(self, x0, y0, x1, y1):
        return box2i.of(*move_box((x0, y0, x1, y1), self.offset))

    def point(self, x, y, source=False):
        d = self.source_offset if source else self.offset
        return v2f(x + d[0], y + d[1])

    def matrix(self, m):
        """source = M target + c  ->  source + Ds = M (target + Dt) + (c - M Dt + Ds)"""
        (dx, dy), (sx, sy) = self.offset, self.source_offset
        far = (m[0], m[1], m[2] - (m[0] * dx + m[1] * dy) + sx, m[3], m[4], m[5] - (m[3] * dx + m[4] * dy) + sy)
        self.matrices.append(far)
        return far

    def windows_back(self):
        out = []
        for o, d in zip(self.objects, self.moves):
            w = o.frame.current_window if o.frame is not None else None
            out.append(None if w is None else box2i.of(*move_box(w.tuple(), (-d[0], -d[1]))))
        return out


# Every group of GROUPS in exactly one class, by the part of its id before '[':
#   equivariant  the far result is the origin result, byte for byte
#   modelled     the far result is the model's at the same far arguments (float positions: the bits differ from the origin's)
#   anchored     coded planes whose raster sits at the origin: a frame far outside it gives black planes / an untouched frame
#   unwindowed   flat arrays: nothing to move
# with the rule its offsets follow: `even_dy` (row parity is that of the absolute coordinate), `limit` (the bound of the
# entry's family), `source_scale` k (the source moves by k times the target's offset: Lanczos at factor 1 / k), `zero_dx`
# (nothing moves along x), `diagonal` (dx == dy).
_ANY = dict(even_dy=False, limit=MAX_COORD, source_scale=1, zero_dx=False, diagonal=False)
# video_mix.c:137,265 picks its `left` frame by comparing one window's min.x with the other's min.Y (frames.c plan_mix keeps
# that): what the mixers compute is unchanged only by an offset with dx == dy.  So for everything that reaches them with
# ragged windows: the chain and blur + over node by node, the crossfade of halfs outside its fused form, the workspace stack.
_DIAG = dict(_ANY, diagonal=True)
_EVEN = dict(_ANY, even_dy=True)
_FLOAT = dict(_ANY, limit=RESAMPLE_MAX_COORD)
FAR_CLASSES = {
    "copies_and_conversions": ("equivariant", _ANY), "attenuate_in_place": ("equivariant", _ANY), "solid_fills": ("equivariant", _ANY),
    "colour_matrix": ("equivariant", _ANY), "mixers_f32": ("equivariant", _DIAG), "mix_cross_f16": ("equivariant", _DIAG),
    "chain": ("equivariant", _ANY), "chain_batches": ("equivariant", _DIAG), "chroma_key": ("equivariant", _ANY),
    "matte": ("equivariant", _ANY), "blur_and_unsharp": ("equivariant", _ANY), "blur_over": ("equivariant", _ANY),
    "blur_over_forms": ("equivariant", _DIAG), "display_bytes": ("equivariant", _ANY), "workspace_stack": ("equivariant", _DIAG),
    # the weave reproduces the reference's row address, which counts the second field's columns from x = 0 and not from the
    # window's first column (kernels/frame_ops.hip k_weave16): what it computes depends on the absolute x, so only y moves
    "weave_fields": ("equivariant", dict(_EVEN, zero_dx=True)), "field_conversions": ("equivariant", _EVEN),
    # positions formed in float (the reference's v2f interface; plan_lanczos: (float)t / factor): equivariant where every
    # position is exact -- factors 0.5 and 2.0 inside +-RESAMPLE_MAX_COORD -- and modelled at the other factors (below)
    "scale_bilinear": ("equivariant", _FLOAT), "lanczos_resample": ("equivariant", dict(_FLOAT, source_scale=2)),
    "blur_lanczos": ("equivariant", dict(_FLOAT, source_scale=2)), "config3_pipeline": ("equivariant", dict(_FLOAT, source_scale=2)),
    "transform": ("modelled", dict(_ANY, limit=_lib.TRANSFORM_MAX_COORD)),
    "dv": ("anchored", None), "mpeg2": ("anchored", None),
    "flat_arrays": ("unwindowed", None),
}
# Cases of the resampler groups whose factors are no power of two: tap positions q + smin round differently at q + (smin + D),
# so the bits are the oracle's at the far arguments, not the origin's.  The bilinear scaler at 0.5 as well: video_scale.c:257-277
# derives the intermediate frame's window with (int)(sp - d * fac), which truncates towards zero -- a half-integer rounds up
# below zero and down above it, so the window reported changes with the sign of the coordinates.
# (group prefix, text in the case's name, the factors of a resampler that takes no points -- its far source must be lined up
# with its far target, lined_up() -- or None for the scaler, whose points move with the frames)
MODELLED_CASES = [("scale_bilinear", "x(0.5, 0.5)", None), ("scale_bilinear", "x(1.5, 1.5)", None), ("scale_bilinear", "x(0.75, 1.5)", None),
                  ("scale_bilinear", "x(0.4, 0.35)", None),
                  ("lanczos_resample", "-> (52, 14)", (0.4, 0.35)), ("lanczos_resample", "-> (128, 30)", (2.0, 1.5)),
                  ("blur_lanczos", "-> (52, 14)", (0.4, 0.35)),
                  ("config3_pipeline", "-> (128, 54)", (2.0, 1.5)), ("config3_pipeline", "-> (20, 40)", (0.1, 1.0))]
# Every modelled case is run far (tests/test_far_windows_gpu.py; the expectations at the same offsets without a GPU:
# tests/test_far_windows_cpu.py): the transform against tests/transform_model.py, these resampler cases in every form -- f32
# and f16, single and batch -- against the oracle, and the field conversions and the weave, equivariant under an even dy, once
# more at an odd dy (odd_dy_offsets), which swaps the fields, against tests/fields_model.py and the oracle.


def _modelled(gid, what):
    prefix = gid.split("[")[0]
    return [m for m in MODELLED_CASES if m[0] == prefix and m[1] in what]


def far_class(gid, what):
    """(class, rule) of case `what` of group `gid`."""
    prefix = gid.split("[")[0]
    cls, rule = FAR_CLASSES[prefix]
    if _modelled(gid, what):
        return "modelled", rule
    return cls, rule


def far_offsets(rule, boxes):
    """[(name, target offset, source offset)] for a case whose operands' full windows at the origin are `boxes`, one
    (is_output, (x0, y0, x1, y1)) per frame: across the 16-bit lines, past a float's integers, and onto the two corners of
    the rule's bound.  An input moves by source_scale times the target's offset."""
    k, lim, even = rule["source_scale"], rule["limit"], rule["even_dy"]
    named = [("across +2^15", (2 ** 15 + 1, -2 ** 15)), ("across -2^16", (-2 ** 16 - 1, 2 ** 16))]
    if lim > 2 ** 25:
        named.append(("past 2^24", (2 ** 24 + 1, -2 ** 24 - 2)))
    if not even:
        named.append(("odd dy", (-2 ** 16 - 2, 2 ** 15 + 1)))
    scale = lambda is_out: 1 if is_out else k
    top = [min((lim - b[2 + a]) // scale(o) for o, b in boxes) for a in (0, 1)]
    bottom = [max(-((lim + b[a]) // scale(o)) for o, b in boxes) for a in (0, 1)]
    if even:
        top[1] -= top[1] & 1
        bottom[1] += bottom[1] & 1
    named += [("top corner", tuple(top)), ("bottom corner", tuple(bottom))]
    if rule["zero_dx"]:
        named = [(name, (0, d[1])) for name, d in named]
    if rule["diagonal"]:              # on a corner: the axis that reaches the bound first
        named = [(name, (min(d, key=abs),) * 2 if "corner" in name else (d[0], d[0])) for name, d in named]
    out = []
    for name, d in named:
        s = (d[0] * k, d[1] * k)
        ok = all(-lim <= v <= lim for o, b in boxes for v in move_box(b, d if o else s))
        if ok:
            out.append((name, d, s))
    return out


def lined_up(fx, fy, boxes, lim):
    """Offsets at which a resampler without points finds its source: with 1 / f = p / q the target moves by q n and the
    source by p n, across the 16-bit lines and as far as the bound lets the larger of the two go."""
    from fractions import Fraction
    rx, ry = Fraction(1.0 / fx).limit_denominator(64), Fraction(1.0 / fy).limit_denominator(64)
    out = []
    for name, n in (("across +2^15", 2 ** 15 + 1), ("across -2^16", -2 ** 16 - 1), ("far", 2 ** 18 + 1), ("far, negative", -2 ** 18 - 3)):
        d, s = (rx.denominator * n, -ry.denominator * n), (rx.numerator * n, -ry.numerator * n)
        if all(-lim <= v <= lim for o, b in boxes for v in move_box(b, d if o else s)):
            out.append((name, d, s))
    return out


def far_offsets_for(gid, what, boxes):
    """The far offsets of case `what` of group `gid`, whatever its class: what both far-window modules run it at."""
    cls, rule = far_class(gid, what)
    hit = _modelled(gid, what)
    if hit and hit[0][2] is not None:
        return lined_up(hit[0][2][0], hit[0][2][1], boxes, rule["limit"])
    if hit:                                # the scaler: target, source and both points by the same offset
        return far_offsets(dict(rule, source_scale=1), boxes)
    return far_offsets(rule, boxes)


def odd_dy_offsets(rule, boxes):
    """Every offset of an even-dy rule one row further (one row back on the top corner): the fields swap."""
    return [(name + ", dy odd", (d[0], d[1] + (-1 if "top" in name else 1)), (s[0], s[1] + (-1 if "top" in name else 1)))
            for name, d, s in far_offsets(rule, boxes)]
