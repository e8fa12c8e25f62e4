"""A pull evaluator for graphs of fluggo.media.process nodes, composed of the per-node models the suite already holds to be
ground truth, and a seeded generator of such graphs.

A graph is a tree of the plain objects below, one class per node kind, holding the parameters the `process` node takes.

    build(process, bt, graph)         the real node tree
    pull(graph, index, full, fmt)     (pixels over `full`, current window or None), on the CPU, by recursion

What is restated here, per node kind, is what the node's code and DESIGN.md 4.7-4.11 say and no entry model does: the window the
node asks of its source, which format it asks it in (the route rule, `pull` itself), and what the compositing nodes do with their
children's windows.  The pixels are the entry models' (`expected` of key_model, matte_model, unsharp_model, transform_model, the
one-input form of fields_model, gain_offset_model) and the oracle's in the flavour in force (blur, scaler, over, crossfade).

A pull promises nothing outside its current window; `pull` returns zeros there, so two pulls compare as arrays.  Frames the
models are fed keep whatever the child's pull put outside its window (zeros): an `expected` that read them would show."""
import ctypes as C
import math

import numpy as np

import oracle
from canvas_amd import synth
from canvas_amd.abi import HostFrame, v2f
from tests import fields_model as fm
from tests import key_model as km
from tests import matte_model as mm
from tests import transform_model as tm
from tests import unsharp_model as um
from tests.models import f2h_rz_model, gain_offset_model

F16, F32 = "f16", "f32"
RASTER = (0, -2, 45, 28)                    # tests/test_fields_gpu.py RASTER: 46 x 31
WIDE = (-6, -3, 293, 37)                    # 300 x 41: past the blur's 256-column pair condition, several matte and transform tiles
TAPS = {
    "gauss3": synth.gaussian_taps(3, 0.8), "gauss5": synth.gaussian_taps(5, 1.0), "gauss9": synth.gaussian_taps(9, 1.5),
    "gauss13": synth.gaussian_taps(13, 2.0), "asym7": np.array([0.05, -0.15, 0.3, 0.5, 0.2, 0.15, -0.05], np.float32),
    "even4": np.array([0.1, 0.4, 0.3, 0.2], np.float32), "gauss15": synth.gaussian_taps(15, 2.5),
}
FUSED_TAPS = ("gauss3", "gauss5", "gauss9", "gauss13", "asym7")      # the unsharp mask's fused kernel has an instance for these
GENERAL_TAPS = ("even4", "gauss15")
FEATHERS = {None: None, "taps3": (0.25, 0.5, 0.25), "taps5": (0.0625, 0.25, 0.375, 0.25, 0.0625),
            "gauss9": tuple(float(t) for t in synth.gaussian_taps(9, 1.5))}
TAPE_KEY = (0.25, 0.5, 0.03)


def _f(v):
    """a number as a node reads it: through a double into an f32"""
    return float(np.float32(v))


def _box(full):
    return (full[3] - full[1] + 1, full[2] - full[0] + 1)


def _grow(full, x, y=None):
    y = x if y is None else y
    return (full[0] - x, full[1] - y, full[2] + x, full[3] + y)


class Lerp:
    """process.LerpFunc(start, end, length): frame * (end - start) / length + start, the difference in f32, the rest in double"""

    def __init__(self, start, end, length):
        self.start, self.end, self.length = tuple(start), tuple(end), float(length)

    def at(self, index):
        return tuple(float(index) * float(np.float32(np.float32(e) - np.float32(s))) / self.length + float(np.float32(s))
                     for s, e in zip(self.start, self.end))


def value(param, index):
    """A parameter at a frame, as a tuple of doubles (a constant is a number or a tuple)."""
    if isinstance(param, Lerp):
        return param.at(index)
    return tuple(float(v) for v in param) if isinstance(param, tuple) else (float(param),)


def scalar(param, index):
    return _f(value(param, index)[0])


def _real(process, bt, param):
    if isinstance(param, Lerp):
        return process.LerpFunc(param.start, param.end, param.length)
    return param


# ---------------------------------------------------------------- node kinds

class Node:
    sources = ()
    half_native = False         # fills the f16 slot only: its f32 pull is its f16 pull widened
    any_format = False          # renders in whichever format is asked for
    filter = False              # a filter with the route rule: the half entry when its source is half-native


class Tape(Node):
    """A foreign half-native source: frame i is a seeded picture over `raster`, colours uniform in 0..1, alpha with zeros and ones."""
    half_native = True

    def __init__(self, raster=RASTER, seed=0, pictures=None):
        """pictures: index -> codes over `raster`, in place of the seeded ones"""
        self.raster, self.seed, self._pictures = tuple(raster), seed, {}
        if pictures is not None:
            self.fresh_picture = pictures

    def picture(self, index):
        if index not in self._pictures:
            self._pictures[index] = self.fresh_picture(index)
        return self._pictures[index]

    def fresh_picture(self, index):
        rng = np.random.default_rng([self.seed, index + 100000])
        h, w = _box(self.raster)
        pixels = rng.uniform(0.0, 1.0, (h, w, 4)).astype(np.float32)
        kind = rng.uniform(size=(h, w))
        pixels[..., 3][kind < 0.15] = 0.0
        pixels[..., 3][kind > 0.7] = 1.0
        return f2h_rz_model(pixels)

    def render(self, index, full, fmt):
        win = um.intersect(full, self.raster)
        out = np.zeros(_box(full) + (4,), np.uint16)
        if win is not None:
            um.crop(out, full, win)[...] = um.crop(self.picture(index), self.raster, win)
        return out, win


class Solid(Node):
    any_format = True

    def __init__(self, color, window=None):
        self.color, self.window = color, window

    def render(self, index, full, fmt):
        c = value(self.color, index)
        color = np.array([_f(c[0]), _f(c[1]), _f(c[2]), min(max(_f(c[3]), 0.0), 1.0)], np.float32)
        win = full if self.window is None else um.intersect(full, self.window)
        out = np.zeros(_box(full) + (4,), np.uint16 if fmt == F16 else np.float32)
        if win is not None:
            um.crop(out, full, win)[...] = f2h_rz_model(color) if fmt == F16 else color
        return out, win


class Gain(Node):
    half_native = True

    def __init__(self, source, gain=1.0, offset=0.0):
        self.sources, self.gain, self.offset = (source,), gain, offset

    def render(self, index, full, fmt):
        src, win = pull(self.sources[0], index, full, F16)
        out = np.zeros_like(src)
        if win is not None:
            um.crop(out, full, win)[...] = gain_offset_model(um.crop(src, full, win), scalar(self.gain, index), scalar(self.offset, index))
        return out, win


class Key(Node):
    """VideoChromaKeyFilter: pulls its source over the window asked for, into the frame itself, and keys it in place"""
    filter = True

    def __init__(self, source, key=TAPE_KEY, tolerance=0.08, softness=0.25, spill=0.0, spill_range=0.0, show_matte=False):
        self.sources, self.key, self.tolerance, self.softness = (source,), key, tolerance, softness
        self.spill, self.spill_range, self.show_matte = spill, spill_range, show_matte

    def params(self, index):
        return dict(key=tuple(_f(v) for v in value(self.key, index)[:3]), tolerance=scalar(self.tolerance, index), softness=scalar(self.softness, index),
                    spill=scalar(self.spill, index), spill_range=scalar(self.spill_range, index), show_matte=self.show_matte)

    def render(self, index, full, fmt):
        src, scur = pull(self.sources[0], index, full, fmt)
        return km.expected(np.zeros_like(src), full, src, full, scur, **self.params(index))


def _oracle_blur(s32, sfull, scur, win, taps):
    src = HostFrame(sfull, np.float32, s32, scur)
    out = HostFrame(win, np.float32)
    t = np.ascontiguousarray(taps, np.float32)
    oracle.lib().orc_fir_blur_f32(out.ref(), src.ref(), t.ctypes.data_as(C.POINTER(C.c_float)), len(t))
    assert out.current_window.tuple() == tuple(win)
    return out.array


class Blur(Node):
    """VideoBlurFilter: asks for the window grown by ntaps / 2 on every side"""
    filter = True

    def __init__(self, source, taps):
        self.sources, self.taps = (source,), taps

    def request(self, full):
        return _grow(full, len(TAPS[self.taps]) // 2)

    def blurred(self, index, full, fmt):
        grown = self.request(full)
        src, scur = pull(self.sources[0], index, grown, fmt)
        win = None if scur is None else um.intersect(scur, full)
        if win is None:
            return src, grown, scur, None, None
        s32 = um.widen(src) if fmt == F16 else src
        return src, grown, scur, win, _oracle_blur(s32, grown, scur, win, TAPS[self.taps])

    def render(self, index, full, fmt):
        src, grown, scur, win, blurred = self.blurred(index, full, fmt)
        out = np.zeros(_box(full) + (4,), src.dtype)
        if win is not None:
            um.crop(out, full, win)[...] = f2h_rz_model(blurred) if fmt == F16 else blurred
        return out, win


class Unsharp(Blur):
    def __init__(self, source, taps, amount=1.0, threshold=0.0):
        Blur.__init__(self, source, taps)
        self.amount, self.threshold = amount, threshold

    def render(self, index, full, fmt):
        src, grown, scur, win, blurred = self.blurred(index, full, fmt)
        return um.expected(np.zeros(_box(full) + (4,), src.dtype), full, src, grown, scur, lambda *a: blurred,
                           scalar(self.amount, index), scalar(self.threshold, index))


class Matte(Node):
    """VideoMatteFilter: asks for the window grown by |choke| + ntaps / 2 on every side"""
    filter = True

    def __init__(self, source, choke=0, feather=None, black=0.0, white=1.0, show_matte=False):
        self.sources, self.choke, self.feather, self.black, self.white, self.show_matte = (source,), choke, feather, black, white, show_matte

    def params(self, index):
        choke = value(self.choke, index)[0]
        return dict(choke=int(math.floor(abs(choke) + 0.5)) * (1 if choke >= 0 else -1), feather=FEATHERS[self.feather],       # lround
                    black=scalar(self.black, index), white=scalar(self.white, index), show_matte=self.show_matte)

    def render(self, index, full, fmt):
        p = self.params(index)
        grown = _grow(full, abs(p["choke"]) + (len(p["feather"]) // 2 if p["feather"] else 0))
        src, scur = pull(self.sources[0], index, grown, fmt)
        return mm.expected(np.zeros(_box(full) + (4,), src.dtype), full, src, grown, scur, **p)


class Transform(Node):
    """VideoTransformFilter: asks for source_window(m, window) clipped to source_rect; reports where source_rect lands in the window"""
    filter = True

    def __init__(self, source, source_rect, anchor=(0.0, 0.0), scale=(1.0, 1.0), rotation=0.0, position=(0.0, 0.0), filter="bilinear"):
        self.sources, self.source_rect, self.anchor, self.scale, self.rotation, self.position, self.filter_name = \
            (source,), tuple(source_rect), anchor, scale, rotation, position, filter

    def coefficients(self, index):
        pair = lambda p: tuple(_f(v) for v in value(p, index)[:2])          # noqa: E731
        return tm.from_parts(pair(self.anchor), pair(self.scale), scalar(self.rotation, index), pair(self.position))

    def render(self, index, full, fmt):
        dtype = np.uint16 if fmt == F16 else np.float32
        before = np.zeros(_box(full) + (4,), dtype)
        m = self.coefficients(index)
        if m is None:
            return before, None
        filt = tm.BILINEAR if self.filter_name == "bilinear" else tm.NEAREST
        need = um.intersect(tm.source_window(m, full), self.source_rect)
        win = None
        if need is not None:
            src, scur = pull(self.sources[0], index, need, fmt)
            before, win = tm.expected(before, full, src, need, scur, m, filt)
        # the window reported is where source_rect lands in `full`, transparent where the entry wrote nothing
        return before, fm.bounding(win, tm.target_window(m, filt, self.source_rect, full))


class Scaler(Node):
    """VideoScaler: asks for the reference's rectangle (video_scale.c:288-319), the mapped window +- 1 clipped to source_rect"""
    filter = True

    def __init__(self, source, target_point, source_point, scale_factors, source_rect):
        self.sources, self.target_point, self.source_point, self.scale_factors, self.source_rect = \
            (source,), target_point, source_point, scale_factors, tuple(source_rect)

    def render(self, index, full, fmt):
        f = np.float32
        tp, sp, fac = ([f(v) for v in value(p, index)[:2]] for p in (self.target_point, self.source_point, self.scale_factors))
        dtype = np.uint16 if fmt == F16 else np.float32
        if fac[0] == 0 or fac[1] == 0:
            return np.zeros(_box(full) + (4,), dtype), None
        if fac[0] == 1 and fac[1] == 1 and tp[0] == sp[0] and tp[1] == sp[1]:
            return pull(self.sources[0], index, full, fmt)
        need = (int(f(sp[0] - f(f(tp[0] - f(full[0])) / fac[0]))) - 1, int(f(sp[1] - f(f(tp[1] - f(full[1])) / fac[1]))) - 1,
                int(f(sp[0] + f(f(f(full[2]) - tp[0]) / fac[0]))) + 1, int(f(sp[1] + f(f(f(full[3]) - tp[1]) / fac[1]))) + 1)
        need = um.intersect(need, self.source_rect)
        if need is None:
            return np.zeros(_box(full) + (4,), dtype), None
        src, scur = pull(self.sources[0], index, need, fmt)
        source = HostFrame(need, np.float32, um.widen(src) if fmt == F16 else src, (0, 0, -1, -1) if scur is None else scur)
        target = HostFrame(full, np.float32)
        oracle.lib().orc_scale_bilinear_f32(target.ref(), v2f(*tp), source.ref(), v2f(*sp), v2f(*fac))
        win = None if target.current_window.is_empty() else target.current_window.tuple()
        out, _ = _canvas(target.array, full, win)
        return (f2h_rz_model(out) if fmt == F16 else out), win


class _Field(Node):
    """The filtering field conversions: ask for the window grown by one row above and below, as f16"""
    half_native = True

    def __init__(self, source, arg=0):
        self.sources, self.arg = (source,), arg

    def render(self, index, full, fmt):
        grown = _grow(full, 0, 1)
        frame, field = self.source_frame(index)
        src, scur = pull(self.sources[0], frame, grown, F16)
        op = (lambda cur, y0: fm.soften(cur, f2h_rz_model)) if field is None else (lambda cur, y0: fm.field_to_frame(cur, y0, field, f2h_rz_model))
        return fm.expected_one_input(np.zeros(_box(full) + (4,), np.uint16), full, (src, grown, scur), op)


class Deinterlace(_Field):
    def source_frame(self, index):
        return index, self.arg


class BobDeinterlace(_Field):
    def source_frame(self, index):
        return index >> 1, self.arg ^ (index & 1)


class Weave(_Field):
    def source_frame(self, index):
        return index, None


class Undefined(Exception):
    """The graph's answer depends on pixels outside a frame's current window, which nothing defines."""


def _poisoned(pixels, full, win):
    """An f32 frame for the oracle's two-input mixers with NaN wherever the pull defined nothing.  The reference's region walk
    picks its `left` frame by comparing one window's min.x with the other's min.y (video_mix.c:137,265): where that picks the
    wrong one it copies pixels from outside that frame's window, uninitialised memory in the reference and whatever the pool
    block held before on the device.  No model can state those pixels; _defined refuses a graph whose answer holds any."""
    out = np.full(_box(full) + (4,), np.nan, np.float32)
    if win is not None:
        um.crop(out, full, win)[...] = um.crop(pixels, full, win)
    return HostFrame(full, np.float32, out, (0, 0, -1, -1) if win is None else win)


def _defined(frame, full, what):
    win = None if frame.current_window.is_empty() else frame.current_window.tuple()
    if win is not None and np.isnan(um.crop(frame.array, full, win)).any():
        raise Undefined("the %s of windows like these reads outside one of them (the reference's `left` selector)" % what)
    return _canvas(frame.array, full, win)


class Mix(Node):
    """VideoMixFilter (crossfade): the ends of the fade are single pulls; in between both sources over the window asked for"""

    def __init__(self, a, b, mix_b):
        self.sources, self.mix_b = (a, b), mix_b

    def render(self, index, full, fmt):
        mix = min(max(scalar(self.mix_b, index), 0.0), 1.0)
        if mix == 0.0 or mix == 1.0:
            return pull(self.sources[int(mix)], index, full, fmt)
        frames = []
        for s in self.sources:
            px, win = pull(s, index, full, fmt)
            frames.append(_poisoned(um.widen(px) if fmt == F16 else px, full, win))
        oracle.lib().orc_mix_cross_f32(frames[0].ref(), frames[0].ref(), frames[1].ref(), C.c_float(mix))
        out, win = _defined(frames[0], full, "crossfade")
        return (f2h_rz_model(out) if fmt == F16 else out), win


class Workspace(Node):
    """VideoWorkspace: the items live at the frame, by z then by the order they were added, each pulled as f32 over the window
    asked for and blended over what is below at mix 1.0 (the oracle's over, `left` quirk and all)"""

    def __init__(self, items):
        self.items = [dict(x=0, length=10, z=k, offset=0, **it) for k, it in enumerate(items)]
        self.sources = tuple(it["source"] for it in self.items)

    def render(self, index, full, fmt):
        live = [(it["z"], k, it) for k, it in enumerate(self.items) if it["x"] <= index < it["x"] + it["length"]]
        acc = None
        for _, _, it in sorted(live, key=lambda t: t[:2]):
            px, win = pull(it["source"], index - it["x"] + it["offset"], full, F32)
            frame = _poisoned(px, full, win)
            if acc is None:
                acc = frame
            else:
                oracle.lib().orc_mix_over_f32(acc.ref(), frame.ref(), C.c_float(1.0))
                below, win = _defined(acc, full, "over")
                acc = _poisoned(below, full, win)
        if acc is None:
            return np.zeros(_box(full) + (4,), np.float32), None
        return _defined(acc, full, "over")


class PassThrough(Node):
    any_format = True

    def __init__(self, source, offset=0, start_frame=None, end_frame=None):
        self.sources, self.offset, self.start_frame, self.end_frame = (source,), offset, start_frame, end_frame

    def render(self, index, full, fmt):
        if (self.start_frame is not None and index < self.start_frame) or (self.end_frame is not None and index >= self.end_frame):
            return np.zeros(_box(full) + (4,), np.uint16 if fmt == F16 else np.float32), None
        return pull(self.sources[0], index + self.offset, full, fmt)


class Sequence(Node):
    """VideoSequence of (source, offset, length): the element covering the frame, pulled in the caller's format"""
    any_format = True

    def __init__(self, elements):
        self.elements = list(elements)
        self.sources = tuple(e[0] for e in self.elements)

    def render(self, index, full, fmt):
        at = 0
        for source, offset, length in self.elements:
            if index >= 0 and at <= index < at + length:
                return pull(source, index - at + offset, full, fmt)
            at += length
        return np.zeros(_box(full) + (4,), np.uint16 if fmt == F16 else np.float32), None


KINDS = {"tape": Tape, "solid": Solid, "gain": Gain, "key": Key, "blur": Blur, "unsharp": Unsharp, "matte": Matte, "transform": Transform,
         "scaler": Scaler, "deinterlace": Deinterlace, "bob": BobDeinterlace, "weave": Weave, "mix": Mix, "workspace": Workspace,
         "pass": PassThrough}


def kind(node):
    return {c: k for k, c in KINDS.items()}.get(type(node), type(node).__name__.lower())


# ---------------------------------------------------------------- the pull

def _canvas(pixels, full, win):
    out = np.zeros_like(pixels)
    if win is not None:
        um.crop(out, full, win)[...] = um.crop(pixels, full, win)
    return out, win


TRACE = None                    # a list: every pull appends (node, window asked, window answered)


def _direct(node):
    """f16 wanted and every source half-native: the node's half entry on its sources' f16 pulls"""
    return (node.filter or isinstance(node, Mix)) and all(s.half_native for s in node.sources)


def pull(node, index, full, fmt):
    """The route rule, in one place.  f16 pull of a filter (or crossfade) whose sources are half-native: the half entry on the
    sources' f16 pulls.  Any other f16 pull of a node with an f32 slot: its f32 pull truncated once.  f32 pull of a half-native
    node: its f16 pull widened.  Nodes without a format of their own (solid, pass-through, sequence) answer in the caller's."""
    full = tuple(int(v) for v in full)
    if node.half_native:
        pixels, win = node.render(index, full, F16)
        if fmt == F32:
            pixels = um.widen(pixels)
    elif fmt == F32 or node.any_format or _direct(node):
        pixels, win = node.render(index, full, fmt)
    else:
        pixels, win = node.render(index, full, F32)
        pixels = f2h_rz_model(pixels)
    win = None if win is None else tuple(int(v) for v in win)
    if TRACE is not None:
        TRACE.append((node, full, win))
    return _canvas(pixels, full, win)


def walk(node):
    yield node
    for s in node.sources:
        yield from walk(s)


# ---------------------------------------------------------------- the real nodes

def build(process, bt, graph, tapes=None):
    """The process node tree of `graph`.  tapes: a list that receives (model tape, real tape) pairs."""
    from tests.test_fields_gpu import Tape as RealTape

    class GraphTape(RealTape):
        def __init__(self, model):
            RealTape.__init__(self, model.raster)
            self.model = model

        def picture(self, index):
            return self.model.picture(index)

    def real(node):
        r = lambda p: _real(process, bt, p)          # noqa: E731
        if isinstance(node, Tape):
            tape = GraphTape(node)
            if tapes is not None:
                tapes.append((node, tape))
            return tape
        if isinstance(node, Solid):
            return process.SolidColorVideoSource(r(node.color)) if node.window is None else process.SolidColorVideoSource(r(node.color), bt.box2i(*node.window))
        src = [real(s) for s in node.sources]
        if isinstance(node, Gain):
            return process.VideoGainOffsetFilter(src[0], gain=r(node.gain), offset=r(node.offset))
        if isinstance(node, Key):
            key = node.key if isinstance(node.key, Lerp) else tuple(node.key[:3]) + (1.0,)
            return process.VideoChromaKeyFilter(src[0], r(key), r(node.tolerance), r(node.softness), r(node.spill), r(node.spill_range), node.show_matte)
        if isinstance(node, Unsharp):
            return process.VideoUnsharpMaskFilter(src[0], tuple(float(t) for t in TAPS[node.taps]), r(node.amount), r(node.threshold))
        if isinstance(node, Blur):
            return process.VideoBlurFilter(src[0], tuple(float(t) for t in TAPS[node.taps]))
        if isinstance(node, Matte):
            return process.VideoMatteFilter(src[0], r(node.choke), FEATHERS[node.feather], r(node.black), r(node.white), node.show_matte)
        if isinstance(node, Transform):
            return process.VideoTransformFilter(src[0], bt.box2i(*node.source_rect), r(node.anchor), r(node.scale), r(node.rotation), r(node.position), node.filter_name)
        if isinstance(node, Scaler):
            return process.VideoScaler(src[0], target_point=r(node.target_point), source_point=r(node.source_point), scale_factors=r(node.scale_factors),
                                       source_rect=bt.box2i(*node.source_rect))
        if isinstance(node, Deinterlace):
            return process.DeinterlaceFilter(src[0], node.arg)
        if isinstance(node, BobDeinterlace):
            return process.BobDeinterlaceFilter(src[0], node.arg)
        if isinstance(node, Weave):
            return process.WeaveInterlaceFilter(src[0])
        if isinstance(node, Mix):
            return process.VideoMixFilter(src[0], src[1], r(node.mix_b))
        if isinstance(node, Workspace):
            ws = process.VideoWorkspace()
            for it, s in zip(node.items, src):
                ws.add(source=s, x=it["x"], length=it["length"], z=it["z"], offset=it["offset"])
            return ws
        if isinstance(node, PassThrough):
            return process.VideoPassThroughFilter(src[0], node.offset, node.start_frame, node.end_frame)
        if isinstance(node, Sequence):
            seq = process.VideoSequence()
            for (_, offset, length), s in zip(node.elements, src):
                seq.append((s, offset, length))
            return seq
        raise TypeError(type(node).__name__)

    return real(graph)


# ---------------------------------------------------------------- the generator

SEED = 20261018
COUNT = 48
FRAMES = (0, 3)
PAIR_KINDS = ("blur", "unsharp", "matte", "transform", "scaler", "key")
SPATIAL = ("blur", "unsharp", "matte", "transform", "scaler")
PAIRS = [(upper, lower) for lower in SPATIAL for upper in PAIR_KINDS]          # upper directly over lower: 30 of them
FILLERS = ("gain", "deinterlace", "bob", "weave", "pass", "key", "blur", "unsharp", "matte", "transform", "scaler")


def _maybe_lerp(rng, a, b, chance=0.3):
    """a, or with `chance` a ramp from a to b over 4 frames (quarters: every frame's value is exact in f32 when a and b are)"""
    return Lerp(a, b, 4.0) if rng.uniform() < chance else (a if len(a) > 1 else a[0])


def _q(rng, lo, hi, step=0.125):
    """a multiple of `step` in lo..hi"""
    return float(np.round(rng.uniform(lo, hi) / step) * step)


def _filter(rng, name, source, raster):
    cx, cy = (raster[0] + raster[2]) / 2.0, (raster[1] + raster[3]) / 2.0
    w, h = raster[2] - raster[0] + 1, raster[3] - raster[1] + 1
    inner = (raster[0] + int(rng.integers(1, 5)), raster[1] + int(rng.integers(1, 4)), raster[2] - int(rng.integers(1, 5)), raster[3] - int(rng.integers(1, 4)))
    if name == "gain":
        return Gain(source, _maybe_lerp(rng, (_q(rng, 0.5, 1.5),), (_q(rng, 0.5, 1.5),)), _q(rng, -0.0625, 0.0625, 0.015625))
    if name == "key":
        spill = rng.uniform() < 0.5
        return Key(source, TAPE_KEY, _maybe_lerp(rng, (0.125,), (0.25,)), float(rng.choice([0.0, 0.25, 0.5])), 0.75 if spill else 0.0,
                   float(rng.choice([0.0, 0.5])) if spill else 0.0, bool(rng.uniform() < 0.2))
    if name == "blur":
        return Blur(source, str(rng.choice(FUSED_TAPS + GENERAL_TAPS)))
    if name == "unsharp":
        taps = str(rng.choice(GENERAL_TAPS if rng.uniform() < 0.35 else FUSED_TAPS))
        return Unsharp(source, taps, _maybe_lerp(rng, (_q(rng, 0.25, 1.5),), (_q(rng, 0.25, 1.5),)), float(rng.choice([0.0, 2.0 ** -6])))
    if name == "matte":
        black, white = [(0.0, 1.0), (0.0625, 0.9375), (0.125, 0.875)][int(rng.integers(0, 3))]
        return Matte(source, int(rng.choice([-2, -1, 1, 2, 3, 0])), [None, "taps3", "taps5", "gauss9"][int(rng.integers(0, 4))], black, white, bool(rng.uniform() < 0.2))
    if name == "transform":
        # near the raster's centre, so that the layer stays in the window: +-40 degrees, 0.6 .. 1.6, a quarter of the raster
        position = (_q(rng, cx - w / 4.0, cx + w / 4.0, 0.25), _q(rng, cy - h / 4.0, cy + h / 4.0, 0.25))
        rotation = (_q(rng, -40.0, 40.0, 0.5),)
        return Transform(source, inner if rng.uniform() < 0.4 else raster, (_q(rng, cx - 2, cx + 2, 0.5), _q(rng, cy - 2, cy + 2, 0.5)),
                         (_q(rng, 0.6, 1.6), _q(rng, 0.6, 1.6)), _maybe_lerp(rng, rotation, (_q(rng, -40.0, 40.0, 0.5),)),
                         _maybe_lerp(rng, position, (position[0] + 2.0, position[1] - 1.5)), str(rng.choice(["bilinear", "bilinear", "nearest"])))
    if name == "scaler":
        # enlarging only: the reference's +- 1 rectangle holds the taps of an enlargement, not those of a reduction
        point = [_q(rng, cx - 3, cx + 3, 0.5), _q(rng, cy - 3, cy + 3, 0.5)]
        target, factors, axis = list(point), [1.0, 1.0], int(rng.integers(0, 2))
        target[axis], factors[axis] = point[axis] + _q(rng, -3, 3, 0.5), _q(rng, 1.0, 1.6)
        return Scaler(source, tuple(target), tuple(point), tuple(factors), inner if rng.uniform() < 0.4 else raster)
    if name == "deinterlace":
        return Deinterlace(source, int(rng.integers(0, 2)))
    if name == "bob":
        return BobDeinterlace(source, int(rng.integers(0, 2)))
    if name == "weave":
        return Weave(source)
    if name == "pass":
        return PassThrough(source, int(rng.integers(-2, 3)))
    raise ValueError(name)


def _chain(rng, raster, pair=None):
    """2-4 filters over a tape; `pair` = (upper, lower) puts that pair next to each other somewhere in it"""
    length = int(rng.integers(2, 5))
    names = [str(rng.choice(FILLERS[:4] if rng.uniform() < 0.6 else FILLERS[4:])) for _ in range(length)]      # six in ten half-native
    if pair is not None:
        at = int(rng.integers(0, length - 1))
        names[at], names[at + 1] = pair[1], pair[0]
    node = Tape(raster, int(rng.integers(0, 1 << 30)))
    for name in names:                           # names[0] sits on the tape
        node = _filter(rng, name, node, raster)
    return node


def tiles(full):
    """The four tiles a window is pulled in (tests/test_unsharp_gpu.py _tiles)"""
    x0, y0, x1, y1 = full
    mx, my = (x0 + x1) // 2, (y0 + y1) // 2 + 1
    return [(x0, y0, mx, my - 1), (mx + 1, y0, x1, my - 1), (x0, my, mx, y1), (mx + 1, my, x1, y1)]


def usable(graph, raster):
    """Whether the tests can hold `graph` to the model: every pull they make of it, whole and in tiles, is defined (no mixer
    reads outside a window, see _poisoned), and every whole pull has a window of 64 pixels or more."""
    try:
        for full in windows(raster):
            for index in FRAMES:
                win = pull(graph, index, full, F32)[1]
                if win is None or (win[2] - win[0] + 1) * (win[3] - win[1] + 1) < 64:
                    return False
                for tile in tiles(full):
                    pull(graph, index, tile, F32)
    except Undefined:
        return False
    return True


def _candidate(rng, raster, pair):
    graph = _chain(rng, raster, pair)
    fate = rng.uniform()
    if fate < 0.3:
        ground = Solid(_maybe_lerp(rng, (0.875, 0.125, 0.25, 0.75), (0.125, 0.5, 0.75, 1.0)), None if rng.uniform() < 0.5 else _grow(raster, -2))
        items = [dict(source=ground), dict(source=graph)]
        if rng.uniform() < 0.5:
            box = (raster[0] + 5, raster[1] + 4, raster[0] + 24, raster[1] + 15)
            items.append(dict(source=Solid((0.25, 0.75, 0.5, 0.5), box)))
        return Workspace(items)
    if fate < 0.5:
        return Mix(graph, _chain(rng, raster), _maybe_lerp(rng, (_q(rng, 0.125, 0.875),), (1.0,), 0.4))
    return graph


def random_graph(rng, raster=RASTER, pair=None):
    """A chain of 2-4 filters over a tape; with probability about a half it then becomes the upper layer of a workspace over a
    solid (sometimes under a third, small item) or one side of a crossfade with a second chain.  Candidates are drawn until
    one is usable()."""
    for _ in range(200):
        graph = _candidate(rng, raster, pair)
        if usable(graph, raster):
            return graph
    raise RuntimeError("no usable graph in 200 draws")


def graphs(seed=SEED, count=COUNT):
    """The graphs of a seed: [(graph, raster)].  The first len(PAIRS) carry one ordered pair each; every fourth graph sits on
    the wide raster."""
    rng = np.random.default_rng(seed)
    out = []
    for n in range(count):
        raster = WIDE if n % 4 == 3 else RASTER
        out.append((random_graph(rng, raster, PAIRS[n] if n < len(PAIRS) else None), raster))
    return out


def windows(raster):
    """The windows a graph on `raster` is pulled over: RASTER from a window every side of which lies outside it, the wide
    raster whole and over a window that starts on an odd column"""
    return [(-3, -5, 50, 31)] if raster == RASTER else [WIDE, (WIDE[0] + 17, WIDE[1] + 2, WIDE[2] - 20, WIDE[3] + 3)]


def fixed_chains():
    """Chains the GPU test pulls whatever the seed, all on RASTER: {name: graph}"""
    cx, cy = 23.0, 13.0
    small = dict(anchor=(cx, cy), scale=(0.625, 0.625), rotation=25.0, position=(cx + 1.0, cy + 0.5))      # well inside the window on every side
    keyed = lambda seed: Key(Tape(RASTER, seed), TAPE_KEY, 0.125, 0.25, 0.75, 0.5)          # noqa: E731
    chains = {
        "transform(blur(matte(key(tape))))":
            Transform(Blur(Matte(keyed(11), 1, "taps5", 0.0625, 0.9375), "gauss9"), RASTER, (cx, cy), (1.25, 0.875), -30.0, (cx - 2.0, cy + 1.0)),
        # the transform leaves the rim of the window empty; the scaler enlarges along x only (see _filter)
        "unsharp(scaler(transform(tape)))":
            Unsharp(Scaler(Transform(Tape(RASTER, 12), RASTER, **small), (cx + 1.5, cy), (cx, cy), (1.375, 1.0), RASTER), "gauss5", 1.5, 2.0 ** -6),
        # |choke| + 4 = 6 pixels of reach, all of them beyond the layer's window on every side
        "matte(transform(tape), choke=-2, feather=gauss9)": Matte(Transform(Tape(RASTER, 13), RASTER, **small), -2, "gauss9"),
        # the deinterlace is half-native: pulled as f16 this is the blur's half entry on the deinterlace's codes
        "blur(deinterlace(tape))": Blur(Deinterlace(Tape(RASTER, 14), 1), "gauss13"),
        "key(weave(tape))": Key(Weave(Tape(RASTER, 15)), TAPE_KEY, 0.125, 0.5, 0.0, 0.0, True),
        # the rotated layer's window starts below row 0, the ground's left edge, so the over's `left` selector picks the ground
        "workspace(blurred ground, keyed and refined layer, rotated layer)": Workspace([
            dict(source=Blur(Tape(RASTER, 16), "asym7")), dict(source=Matte(keyed(17), -1, "taps3")),
            dict(source=Transform(Tape(RASTER, 18), _grow(RASTER, -3), (cx, cy), (0.625, 0.5), 35.0, (cx + 1.0, cy + 4.0)))]),
        # the regression case of the transform's window: a 13-tap blur over a turned layer, whose halo a tile used to lose
        "blur(transform(tape)), 13 taps over a turned layer":
            Blur(Transform(Tape(RASTER, 19), RASTER, (22.5, 11.5), (1.375, 1.0), 16.5, (16.5, 16.25)), "gauss13"),
    }
    return chains
