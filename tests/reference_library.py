"""The reference side of a catalogue case, without a GPU: a stand-in for the library that hands cvs_X_dev(..., stream) to the
CPU oracle -- the reference's pixel code in `int` -- or to the numpy models, on frames in host memory.

  ORACLE     entries whose oracle function takes the same arguments but the stream
  COMPOSED   entries composed of the oracle's pieces as tests/test_gpu_parity.py composes them: the f16 and batch forms of the
             resamplers (widen, the f32 node, truncate; a batch is its single calls), the frame conversions through
             oracle.half_to_float / float_to_half, the fills, the colour matrix with its tables, the blur between half frames
             (tests/util.py oracle_blur_over), the chain, the display bytes (orc_frame_to_bytes, orc_frame_to_rgba8_intent)
  MODELLED   entries the reference has no C for, tied to the numpy models their own GPU modules use (fields_model, key_model,
             matte_model, transform_model, unsharp_model, lut3d_model, scope_model over the oracle's display bytes, mpeg2_model,
             mpeg2_reconstruct_model)
  EXTENSIONS the entries of the extension headers, which the reference has no code for either: the adaptive deinterlacer, the
             temporal denoise, the corner pin, the 4:2:2 and 4:2:0 edges, the median, the primary and the secondaries, each
             through the model of its own GPU module
  and the workspace's device slot, which ReferenceLibrary answers with orc_workspace_get_frame_f32

tests/test_far_windows_cpu.py and tests/test_far_windows_gpu.py run the catalogue of tests/entry_cases.py through it far from
the origin, tests/test_extents_cpu.py and tests/test_extents_gpu.py the catalogue of tests/extent_cases.py at extents no picture
has.  The oracle's functions follow oracle.flavour(); the models are the same in both flavours, as their GPU modules assert."""
import ctypes as C

import numpy as np

import oracle
from canvas_amd import _lib
from canvas_amd.abi import GET_FRAME_F16, GET_FRAME_F32, HostFrame, video_frame_source_funcs, video_source
from tests import entry_cases as ec
from tests import fields_model as fm
from tests import key_model as km
from tests import matte_model as mm
from tests import transform_model as tm
from tests import unsharp_model as um

# device entry -> the oracle function with the same arguments but the stream
ORACLE = {"cvs_copy_frame_f16_dev": "orc_copy_frame_f16", "cvs_copy_frame_alpha_f32_dev": "orc_copy_frame_alpha_f32",
          "cvs_gain_offset_f16_dev": "orc_gain_offset_f16", "cvs_mix_over_f32_dev": "orc_mix_over_f32",
          "cvs_mix_cross_f32_dev": "orc_mix_cross_f32", "cvs_weave_fields_f16_dev": "orc_weave_fields_f16",
          "cvs_scale_bilinear_f32_dev": "orc_scale_bilinear_f32", "cvs_resample_lanczos_f32_dev": "orc_resample_lanczos_f32",
          "cvs_fir_blur_f32_dev": "orc_fir_blur_f32"}


class NotInTheOracle(Exception):
    pass


def _struct(ref):
    return getattr(ref, "_obj", ref)


def _pixels_of(c, dtype):
    """The numpy view of the buffer a frame struct describes."""
    h, w = c.full_window.height, c.full_window.width
    ctype = C.c_uint16 if dtype == np.uint16 else C.c_float
    return np.ctypeslib.as_array(C.cast(c.data, C.POINTER(ctype)), shape=(h, w, 4))


def _widened(c):
    """A half frame struct as the f32 HostFrame its f32 pull would deliver (tests/test_gpu_parity.py: widen, then the f32 node)."""
    return HostFrame(c.full_window.tuple(), np.float32, oracle.half_to_float(_pixels_of(c, np.uint16)), c.current_window.tuple())


def _narrow_into(c, f32, window_only):
    """... and the f32 result truncated into the half frame: the whole buffer, or (window_only, the scaler: what lies outside
    the reported window is not defined) the reported window alone."""
    codes = oracle.float_to_half(f32.array)
    w, full = f32.current_window, c.full_window
    if not window_only:
        _pixels_of(c, np.uint16)[...] = codes
    elif not w.is_empty():
        ys, xs = slice(w.min.y - full.min.y, w.max.y - full.min.y + 1), slice(w.min.x - full.min.x, w.max.x - full.min.x + 1)
        _pixels_of(c, np.uint16)[ys, xs] = codes[ys, xs]
    c.current_window = type(c.current_window).of(*w.tuple())


# The f16 and batch forms of the resamplers, composed of the oracle's f32 pieces as tests/test_gpu_parity.py composes them
# (test_scale_bilinear_f16_twin, test_lanczos_resample_between_f16_frames, _oracle_config3); a batch is its single calls.
def _lanczos_f16(out, src, fx, fy, ksize):
    o, t = _struct(out), HostFrame(_struct(out).full_window.tuple(), np.float32)
    s32 = _widened(_struct(src))
    oracle.lib().orc_resample_lanczos_f32(t.ref(), s32.ref(), fx, fy, ksize)
    _narrow_into(o, t, False)


def _scale_f16(out, tp, src, sp, fac):
    o = _struct(out)
    t, s32 = _widened(o), _widened(_struct(src))
    oracle.lib().orc_scale_bilinear_f32(t.ref(), tp, s32.ref(), sp, fac)
    _narrow_into(o, t, True)


def _scale_batch(half):
    def run(outs, tp, srcs, sp, fac, count):
        for k in range(count):
            if half:
                _scale_f16(outs[k].contents, tp, srcs[k].contents, sp, fac)
            else:
                oracle.lib().orc_scale_bilinear_f32(outs[k], tp, srcs[k], sp, fac)
    return run


def _blur_lanczos_f16(out, src, taps, ntaps, fx, fy, ksize):
    o, s32 = _struct(out), _widened(_struct(src))
    blurred = HostFrame(s32.full_window.tuple(), np.float32)
    oracle.lib().orc_fir_blur_f32(blurred.ref(), s32.ref(), taps, ntaps)
    t = HostFrame(o.full_window.tuple(), np.float32)
    oracle.lib().orc_resample_lanczos_f32(t.ref(), blurred.ref(), fx, fy, ksize)
    _narrow_into(o, t, False)


def _blur_lanczos_batch(outs, srcs, count, taps, ntaps, fx, fy, ksize):
    for k in range(count):
        _blur_lanczos_f16(outs[k].contents, srcs[k].contents, taps, ntaps, fx, fy, ksize)


COMPOSED = {"cvs_resample_lanczos_f16_dev": _lanczos_f16, "cvs_scale_bilinear_f16_dev": _scale_f16,
            "cvs_scale_bilinear_f16_batch_dev": _scale_batch(True), "cvs_scale_bilinear_f32_batch_dev": _scale_batch(False),
            "cvs_blur_lanczos_f16_dev": _blur_lanczos_f16, "cvs_blur_lanczos_f16_batch_dev": _blur_lanczos_batch}
# the entries whose oracle result is defined inside the reported window only
WINDOW_ONLY = ("cvs_scale_bilinear_f16_dev", "cvs_scale_bilinear_f16_batch_dev")


class OracleAsLibrary:
    """Stands in for the library: the entries of ORACLE run the oracle's function, those of COMPOSED the oracle's pieces; any
    other raises NotInTheOracle."""
    tables = (ORACLE, COMPOSED)

    def __getattr__(self, name):
        direct, composed = self.tables
        if name not in direct and name not in composed:
            def missing(*args):
                raise NotInTheOracle(name)
            return missing
        fn = composed[name] if name in composed else getattr(oracle.lib(), direct[name])

        def call(*args):
            fn(*args[:-1])
            return 0
        return call


class OnHost(ec.Factory):
    """Frames in host memory, each with pixels of its own."""

    def _make_frame(self, o, host):
        o.frame = HostFrame(host.full_window.tuple(), host.dtype, host.array.copy(), host.current_window.tuple())
        o.ptr = o.frame.array.ctypes.data

    def _make_buffer(self, o, data):
        raise NotInTheOracle("a flat buffer")

    def collect(self):
        return [o.frame.array.copy() for o in self.objects]


# ------------------------------------------------------------------ the wider map (tests/extent_cases.py)

def _tuple_or_none(w):
    return None if w.is_empty() else w.tuple()


def _set_window(c, win):
    c.current_window = type(c.current_window).of(*(win if win is not None else (0, 0, -1, -1)))


def _inside(c, win):
    """The view of window `win` (a tuple) of the buffer frame struct `c` describes."""
    full = c.full_window
    dtype = np.uint16 if isinstance(c, _lib.rgba_frame_f16_t) else np.float32
    return _pixels_of(c, dtype)[win[1] - full.min.y:win[3] - full.min.y + 1, win[0] - full.min.x:win[2] - full.min.x + 1]


def _convert(out, src):
    """cvs_frame_f16_to_f32_dev / cvs_frame_f32_to_f16_dev (main.c:115-139, 43-71): the rows of the source's window through
    the oracle's conversion of the flavour-independent kind; the window is the source's."""
    o, s = _struct(out), _struct(src)
    win = _tuple_or_none(s.current_window)
    _set_window(o, win)
    if win is None:
        return
    assert fm.intersect(win, o.full_window.tuple()) == win
    pixels = np.ascontiguousarray(_inside(s, win))
    _inside(o, win)[...] = oracle.half_to_float(pixels) if pixels.dtype == np.uint16 else oracle.float_to_half(pixels)


def _fill(half):
    def run(frame, window, colour):
        c = _struct(colour)
        values = np.array([c.r, c.g, c.b, c.a], np.float32)
        fn = oracle.lib().orc_solid_f16 if half else oracle.lib().orc_solid_f32
        fn(frame, window, values.ctypes.data_as(C.POINTER(C.c_float)))
    return run


def _table_or_none(which):
    return None if which == _lib.LUT_NONE else oracle.transfer_table(which)


def _colour_matrix(frame, m, pre, post):
    pre, post = _table_or_none(pre), _table_or_none(post)
    u16p = lambda t: None if t is None else t.ctypes.data_as(C.POINTER(C.c_uint16))
    oracle.lib().orc_color_matrix_f16(frame, m, u16p(pre), u16p(post))


def _colour_matrix_to(out, src, m, pre, post):
    """host/color.c: the window is the source's, clipped to the target's buffer; its pixels are the source's, converted."""
    o, s = _struct(out), _struct(src)
    win = fm.intersect(_tuple_or_none(s.current_window), o.full_window.tuple())
    _set_window(o, win)
    if win is None:
        return
    part = HostFrame(win, np.uint16, _inside(s, win).copy())
    _colour_matrix(part.ref(), m, pre, post)
    _inside(o, win)[...] = part.array


def _blur_f16(out, src, taps, ntaps):
    o, s32 = _struct(out), _widened(_struct(src))
    t = _widened(o)
    oracle.lib().orc_fir_blur_f32(t.ref(), s32.ref(), taps, ntaps)
    _narrow_into(o, t, True)


def _model_call(expected):
    """expected(before, target_full, source, source_full, source_cur, *params) -> (buffer, window) as every model has it."""
    def run(out, src, *params):
        o, s = _struct(out), _struct(src)
        dtype = np.uint16 if isinstance(o, _lib.rgba_frame_f16_t) else np.float32
        after, win = expected(_pixels_of(o, dtype), o.full_window.tuple(), _pixels_of(s, dtype), s.full_window.tuple(),
                              _tuple_or_none(s.current_window), *params)
        _pixels_of(o, dtype)[...] = after
        _set_window(o, win)
    return run


def _key(before, tfull, src, sfull, scur, params):
    p = _struct(params)
    return km.expected(before, tfull, src, sfull, scur, tuple(p.key), p.tolerance, p.softness, p.spill, p.spill_range,
                       bool(p.flags & _lib.KEY_SHOW_MATTE))


def _matte(before, tfull, src, sfull, scur, params):
    p = _struct(params)
    feather = [p.taps[k] for k in range(p.ntaps)] if p.ntaps else None
    return mm.expected(before, tfull, src, sfull, scur, p.choke, feather, p.black, p.white, bool(p.flags & _lib.MATTE_SHOW))


def _transform(before, tfull, src, sfull, scur, params):
    p = _struct(params)
    return tm.expected(before, tfull, src, sfull, scur, tuple(p.m), p.filter)


def _field(before, tfull, src, sfull, scur, field):
    return fm.expected_one_input(before, tfull, (src, sfull, scur), lambda cur, y0: field_to_frame(cur, y0, field))


def _soften(before, tfull, src, sfull, scur):
    return fm.expected_one_input(before, tfull, (src, sfull, scur), lambda cur, y0: fm.soften(cur, oracle.float_to_half))


def field_to_frame(cur, y0, field):
    """fields_model.field_to_frame, which walks the rows in Python, with the rows as array operations: the same statements
    (t = above * 0.5; u = below * 0.5; s = t + u; truncate), evaluated for every made row at once."""
    h = cur.shape[0]
    out = cur.copy()
    made = np.flatnonzero(((y0 + np.arange(h)) & 1) != field)
    both = made[(made >= 1) & (made + 1 < h)]
    if both.size:
        with np.errstate(all="ignore"):
            t = fm.widen(cur[both - 1]) * fm.F(0.5)
            u = fm.widen(cur[both + 1]) * fm.F(0.5)
            s = t + u
        out[both] = oracle.float_to_half(s)
    if h == 1 and made.size:
        out[0] = 0                                      # (no row above or below: the model's zeros)
    elif made.size:
        if made[0] == 0:
            out[0] = cur[1]
        if made[-1] == h - 1:
            out[h - 1] = cur[h - 2]
    return out


def _interlace(out, even, odd):
    o, e, d = _struct(out), _struct(even), _struct(odd)
    frame = lambda c: (_pixels_of(c, np.uint16), c.full_window.tuple(), _tuple_or_none(c.current_window))
    after, win = fm.expected_interlace(_pixels_of(o, np.uint16), o.full_window.tuple(), frame(e), frame(d))
    _pixels_of(o, np.uint16)[...] = after
    _set_window(o, win)


def _unsharp(before, tfull, src, sfull, scur, taps, ntaps, amount, threshold):
    def blur(s32, full, cur, win):
        source = HostFrame(full, np.float32, s32, cur)
        target = HostFrame(win, np.float32)
        oracle.lib().orc_fir_blur_f32(target.ref(), source.ref(), taps, ntaps)
        assert target.current_window.tuple() == tuple(win)
        return target.array
    return um.expected(before, tfull, src, sfull, scur, blur, np.float32(amount.value), np.float32(threshold.value))


def _as_host(c):
    """A half frame struct as a HostFrame over the same pixels."""
    return HostFrame(c.full_window.tuple(), np.uint16, _pixels_of(c, np.uint16), c.current_window.tuple())


def _window_into(c, result):
    """The reported window of `result` (a HostFrame over c's buffer window) into frame struct c: these forms define no more."""
    w = _tuple_or_none(result.current_window)
    _set_window(c, w)
    if w is not None:
        _inside(c, w)[...] = result.window_view()


def _cross_f16(out, a, b, mix):
    """tests/test_gpu_parity.py _oracle_cross_f16: widen (clipped to the output buffer, as a pull into it would be), the f32
    crossfade, truncate."""
    o = _struct(out)
    full = o.full_window.tuple()

    def pulled(c):
        clip = HostFrame(full, np.uint16)
        oracle.lib().orc_copy_frame_f16(clip.ref(), C.byref(c))
        return HostFrame(full, np.float32, oracle.half_to_float(clip.array), clip.current_window)
    pa, pb = pulled(_struct(a)), pulled(_struct(b))
    t = HostFrame(full, np.float32)
    oracle.lib().orc_mix_cross_f32(t.ref(), pa.ref(), pb.ref(), mix)
    _window_into(o, HostFrame(full, np.uint16, oracle.float_to_half(t.array), t.current_window))


def _chain(jobs, njobs, m, pre, post):
    """A chain call is its jobs, each the oracle's chain (tests/test_gpu_parity.py test_chain_batch_and_lut_variants)."""
    pre, post = _table_or_none(pre), _table_or_none(post)
    for j in range(njobs):
        o = jobs[j].out.contents
        layers = [_as_host(jobs[j].layers[k].contents) for k in range(jobs[j].nlayers)]
        matrix = None if m is None else np.ctypeslib.as_array(m, shape=(9,)).copy()
        _window_into(o, oracle.chain_color_over(layers, matrix, pre, post, o.full_window.tuple()))


def _blur_over(out, src, taps, ntaps, overlays, nover):
    """tests/util.py oracle_blur_over: widen, the f32 blur into the output's buffer window, every overlay widened and laid
    over at mix 1.0, truncate."""
    from tests.util import oracle_blur_over
    o = _struct(out)
    t = np.ctypeslib.as_array(taps, shape=(ntaps,)).copy()
    _window_into(o, oracle_blur_over(oracle, _as_host(_struct(src)), t, [_as_host(overlays[k].contents) for k in range(nover)], o.full_window.tuple()))


def _blur_over_batch(outs, srcs, taps, ntaps, overlays, nover, count):
    """A batch is its single calls (run with one overlay per frame: overlay k lies over frame k)."""
    assert nover == 1
    for k in range(count):
        _blur_over(outs[k].contents, srcs[k].contents, taps, ntaps, [overlays[k]], 1)


# ---- flat buffers: on this side a buffer's address is host memory

def _bytes_at(address, count, dtype=np.uint8):
    n = int(count) * np.dtype(dtype).itemsize
    return np.frombuffer((C.c_uint8 * n).from_address(int(address)), dtype) if n else np.zeros(0, dtype)


def _u16p_or_none(t):
    return None if t is None else t.ctypes.data_as(C.POINTER(C.c_uint16))


def _to_bytes(dst, frame, pre, mode):
    oracle.lib().orc_frame_to_bytes(C.cast(dst, C.POINTER(C.c_uint32)), frame, _u16p_or_none(_table_or_none(pre)), mode)


def _to_rgba8_intent(dst, frame, pre, intent):
    oracle.lib().orc_frame_to_rgba8_intent(C.cast(dst, C.POINTER(C.c_uint32)), frame, _u16p_or_none(_table_or_none(pre)), intent)


def _lut3d(out, src, lattice, params):
    from tests import lut3d_model as lm
    o, s, p = _struct(out), _struct(src), _struct(params)
    dtype = np.uint16 if isinstance(o, _lib.rgba_frame_f16_t) else np.float32
    n = p.size
    lat = np.ascontiguousarray(_bytes_at(lattice, n ** 3 * 4, np.float32).reshape(-1, 4)[:, :3]).reshape(n, n, n, 3)
    before = _pixels_of(o, dtype).copy()                       # (in place: the source is read before the target is written)
    after, win = lm.expected(before, o.full_window.tuple(), _pixels_of(s, dtype).copy(), s.full_window.tuple(), _tuple_or_none(s.current_window),
                             lat, (tuple(p.domain_min), tuple(p.domain_max)))
    _pixels_of(o, dtype)[...] = after
    _set_window(o, win)


def _scope_counts(table, frame, params):
    """The bytes the display edge gives for the frame's window (the oracle's), counted by tests/scope_model.py."""
    from tests import scope_model as sm
    f, p = _struct(frame), _struct(params)
    cur = _tuple_or_none(f.current_window)
    px = None
    if cur is not None:
        px = np.zeros((cur[3] - cur[1] + 1, cur[2] - cur[0] + 1, 4), np.uint8)
        if p.rendering_intent > 0:
            _to_rgba8_intent(px.ctypes.data, C.byref(f), p.pre_lut, C.c_float(p.rendering_intent))
        else:
            _to_bytes(px.ctypes.data, C.byref(f), p.pre_lut, _lib.DISPLAY_RGBA8)
    counts = sm.table(p.kind, px, cur, p.region.tuple(), p.columns, bool(p.flags & _lib.SCOPE_SKIP_TRANSPARENT))
    _bytes_at(table, counts.size, np.uint32)[...] = counts


def _scope_render(target, place, table, params, gain):
    from tests import scope_model as sm
    t, p, at = _struct(target), _struct(params), _struct(place).tuple()
    picture = sm.picture(p.kind, _bytes_at(table, sm.count(p.kind, p.columns), np.uint32), p.columns, gain.value)
    win = fm.intersect(at, t.full_window.tuple())
    _set_window(t, win)
    if win is not None:
        _inside(t, win)[...] = picture[win[1] - at[1]:win[3] - at[1] + 1, win[0] - at[0]:win[2] - at[0] + 1]


def _gcc_table(which):
    """The MPEG-2 filters read the separate build's transfer table in both flavours (tests/test_mpeg2_gpu.py)."""
    with oracle.flavour("gcc"):
        return oracle.transfer_table(which)


def _planes(image):
    img = _struct(image)
    return [_bytes_at(img.data[k], img.stride[k] * img.line_count[k]).reshape(img.line_count[k], img.stride[k]) for k in range(3)]


def _reconstruct_mpeg2(frame, image, width, height, flags):
    from tests import mpeg2_reconstruct_model as rm
    f = _struct(frame)
    raster = rm.reconstruct_model(_planes(image), width, height, _gcc_table(0), oracle.float_to_half,
                                  not flags & _lib.YCC_PROGRESSIVE, "709" if flags & _lib.YCC_REC709 else "601")
    after, win = rm.expected_frame(_pixels_of(f, np.uint16), f.full_window.tuple(), raster, width, height)
    _pixels_of(f, np.uint16)[...] = after
    _set_window(f, win)


def _subsample_mpeg2(image, frame, width, height):
    from tests import mpeg2_model as sm2
    f = _struct(frame)
    want = sm2.mpeg2_subsample_model(_pixels_of(f, np.uint16), f.full_window.tuple(), f.current_window.tuple(), width, height, _gcc_table(2))
    for plane, w in zip(_planes(image), want):
        plane[:w.shape[0], :w.shape[1]] = w


# ---- the extension headers' entries: no reference code, only the numpy models of their own GPU modules.  Every one of these
# models works on whole arrays (none walks the rows in Python, as fields_model.field_to_frame does), so it is the model itself,
# not a restatement, that tests/test_extents_cpu.py runs at four million rows.

def _frame_or_none(ref, dtype=np.uint16):
    """A frame argument as the models take one: (pixels over the full window, full window, current window or None); None for NULL"""
    if ref is None:
        return None
    c = _struct(ref)
    return (_pixels_of(c, dtype), c.full_window.tuple(), _tuple_or_none(c.current_window))


def _deinterlace(out, prev, cur, nxt, params):
    from tests import deinterlace_model as dm
    o, p = _struct(out), _struct(params)
    after, win, _exact, _k = dm.expected(_pixels_of(o, np.uint16), o.full_window.tuple(), _frame_or_none(cur), _frame_or_none(prev), _frame_or_none(nxt),
                                         p.field, p.threshold, p.softness, oracle.float_to_half)
    _pixels_of(o, np.uint16)[...] = after
    _set_window(o, win)


def _temporal(out, prev2, prev1, cur, next1, next2, params):
    from tests import temporal_model as tpm
    o, p = _struct(out), _struct(params)
    neighbours = [_frame_or_none(f) for f in (prev1, next1, prev2, next2)]           # the contract's order of summation
    after, win, _exact, _w = tpm.expected(_pixels_of(o, np.uint16), o.full_window.tuple(), _frame_or_none(cur), neighbours, p.threshold, p.softness,
                                          p.channels, oracle.float_to_half)
    _pixels_of(o, np.uint16)[...] = after
    _set_window(o, win)


def _perspective(before, tfull, src, sfull, scur, params):
    from tests import perspective_model as pm
    p = _struct(params)
    return pm.expected(before, tfull, src, sfull, scur, (tuple(p.h), tuple(p.target_origin), tuple(p.source_origin)), p.filter)


def _median(before, tfull, src, sfull, scur, params):
    """(the model works on bit patterns: an f32 frame as uint32)"""
    from tests import median_model as mdm
    p = _struct(params)
    bits = (lambda a: a) if before.dtype == np.uint16 else (lambda a: a.view(np.uint32))
    after, win = mdm.expected(bits(before), tfull, bits(src), sfull, scur, p.radius, p.threshold, p.channels)
    return after.view(before.dtype), win


def _primary(out, src, params, pre, post):
    """In place too: the source is read before the target is written."""
    from tests import primary_model as prm
    o, s, p = _struct(out), _struct(src), _struct(params)
    dtype = np.uint16 if isinstance(o, _lib.rgba_frame_f16_t) else np.float32

    def curves(stage, address):
        if stage.size == 0:
            return None
        table = _bytes_at(address, 3 * stage.size, np.float32).reshape(3, stage.size).T          # (planar: K of R, K of G, K of B)
        return prm.Curves(table.copy(), (tuple(stage.domain_min), tuple(stage.domain_max)))
    matrix = list(p.matrix) if p.flags & _lib.PRIMARY_MATRIX else None
    after, win = prm.expected(_pixels_of(o, dtype).copy(), o.full_window.tuple(), _pixels_of(s, dtype).copy(), s.full_window.tuple(),
                              _tuple_or_none(s.current_window), curves(p.pre, pre), matrix, curves(p.post, post))
    _pixels_of(o, dtype)[...] = after
    _set_window(o, win)


def _qualify(out, src, key, params):
    from tests import secondary_model as scm
    o, p = _struct(out), _struct(params)
    dtype = np.uint16 if isinstance(o, _lib.rgba_frame_f16_t) else np.float32
    f = p.flags
    q = scm.Qualifier(hue=(p.hue.center, p.hue.width, p.hue.softness) if f & _lib.QUAL_HUE else None,
                      saturation=(p.saturation.low, p.saturation.high, p.saturation.soft_low, p.saturation.soft_high) if f & _lib.QUAL_SATURATION else None,
                      luma=(p.luma.low, p.luma.high, p.luma.soft_low, p.luma.soft_high) if f & _lib.QUAL_LUMA else None,
                      invert=bool(f & _lib.QUAL_INVERT), show_matte=bool(f & _lib.QUAL_SHOW_MATTE))
    s, k = _frame_or_none(src, dtype), _frame_or_none(key, dtype)
    args = (s[0].copy(), s[1], s[2], q) + ((k[0].copy(), k[1], k[2]) if k is not None else ())
    after, win = scm.expected_qualify(_pixels_of(o, dtype).copy(), o.full_window.tuple(), *args)
    _pixels_of(o, dtype)[...] = after
    _set_window(o, win)


def _matte_mix(out, a, b, matte, params):
    from tests import secondary_model as scm
    o, p = _struct(out), _struct(params)
    dtype = np.uint16 if isinstance(o, _lib.rgba_frame_f16_t) else np.float32
    args = [v for f in (a, b, matte) for v in _frame_or_none(f, dtype)]
    args[0::3] = [pixels.copy() for pixels in args[0::3]]
    after, win = scm.expected_mix(_pixels_of(o, dtype).copy(), o.full_window.tuple(), *args, luma=bool(p.flags & _lib.MMIX_LUMA), invert=bool(p.flags & _lib.MMIX_INVERT))
    _pixels_of(o, dtype)[...] = after
    _set_window(o, win)


def _coded(image, nplanes):
    img = _struct(image)
    return [_bytes_at(img.data[k], img.stride[k] * img.line_count[k]).reshape(img.line_count[k], img.stride[k]) for k in range(nplanes)]


def _name_of(table, value):
    return next(name for name, v in table.items() if v == value)


def _reconstruct_422(frame, image, width, height, layout, flags):
    from tests import ycc422_model as y2
    f, name = _struct(frame), _name_of(y2.LAYOUTS, layout)
    raster = y2.reconstruct_model(name, _coded(image, y2.PLANES[name]), width, height, _gcc_table(0), oracle.float_to_half, "709" if flags & _lib.YCC_REC709 else "601")
    after, win = y2.expected_frame(_pixels_of(f, np.uint16), f.full_window.tuple(), raster, width, height)
    _pixels_of(f, np.uint16)[...] = after
    _set_window(f, win)


def _subsample_422(image, frame, width, height, layout, flags):
    """The planes the call writes: the least stride's bytes of the raster's lines; everything else keeps what it held."""
    from tests import ycc422_model as y2
    f, name = _struct(frame), _name_of(y2.LAYOUTS, layout)
    want = y2.subsample_model(name, _pixels_of(f, np.uint16), f.full_window.tuple(), f.current_window.tuple(), width, height, _gcc_table(2),
                              "709" if flags & _lib.YCC_REC709 else "601")
    for plane, w in zip(_coded(image, y2.PLANES[name]), want):
        plane[:w.shape[0], :w.shape[1]] = w


def _flags_420(flags):
    from tests import ycc420_model as y0
    pick = lambda table, mask: _name_of(table, flags & mask)
    return (pick(y0.MATRIX_FLAGS, 2 | 4), pick(y0.RANGE_FLAGS, 8), pick(y0.SITING_FLAGS, 16 | 32), pick(y0.TRANSFER_FLAGS, 64))


def _reconstruct_420(frame, image, width, height, layout, flags):
    from tests import ycc420_model as y0
    f, name = _struct(frame), _name_of(y0.LAYOUTS, layout)
    matrix, range_, siting, transfer = _flags_420(flags)
    raster = y0.reconstruct_model(name, _coded(image, y0.PLANES[name]), width, height, _gcc_table(0), oracle.float_to_half, matrix, range_, siting, transfer)
    after, win = y0.expected_frame(_pixels_of(f, np.uint16), f.full_window.tuple(), raster, width, height)
    _pixels_of(f, np.uint16)[...] = after
    _set_window(f, win)


def _subsample_420(image, frame, width, height, layout, flags):
    from tests import ycc420_model as y0
    f, name = _struct(frame), _name_of(y0.LAYOUTS, layout)
    matrix, range_, siting, transfer = _flags_420(flags)
    want = y0.subsample_model(name, _pixels_of(f, np.uint16), f.full_window.tuple(), f.current_window.tuple(), width, height, _gcc_table(2),
                              matrix, range_, siting, transfer)
    for plane, w in zip(_coded(image, y0.PLANES[name]), want):
        plane[:w.shape[0], :w.shape[1]] = w


EXTENSIONS = {"cvs_deinterlace_adaptive_f16_dev": _deinterlace, "cvs_temporal_denoise_f16_dev": _temporal,
              "cvs_perspective_f16_dev": _model_call(_perspective), "cvs_perspective_f32_dev": _model_call(_perspective),
              "cvs_reconstruct_422_dev": _reconstruct_422, "cvs_subsample_422_dev": _subsample_422,
              "cvs_reconstruct_420_dev": _reconstruct_420, "cvs_subsample_420_dev": _subsample_420,
              "cvs_median_f16_dev": _model_call(_median), "cvs_median_f32_dev": _model_call(_median),
              "cvs_primary_f16_dev": _primary, "cvs_primary_f32_dev": _primary,
              "cvs_qualify_f16_dev": _qualify, "cvs_qualify_f32_dev": _qualify, "cvs_matte_mix_f16_dev": _matte_mix, "cvs_matte_mix_f32_dev": _matte_mix}

MODELLED = {"cvs_blur_over_f16_batch_dev": _blur_over_batch, "cvs_frame_to_bytes_dev": _to_bytes, "cvs_frame_to_rgba8_intent_dev": _to_rgba8_intent,
            "cvs_lut3d_f16_dev": _lut3d, "cvs_lut3d_f32_dev": _lut3d, "cvs_scope_counts_f16_dev": _scope_counts,
            "cvs_scope_render_f16_dev": _scope_render, "cvs_reconstruct_mpeg2_dev": _reconstruct_mpeg2, "cvs_subsample_mpeg2_dev": _subsample_mpeg2,
            "cvs_mix_cross_f16_dev": _cross_f16, "cvs_chain_color_over_f16_dev": _chain, "cvs_blur_over_f16_dev": _blur_over,
            "cvs_frame_f16_to_f32_dev": _convert, "cvs_frame_f32_to_f16_dev": _convert,
            "cvs_fill_solid_f16_dev": _fill(True), "cvs_fill_solid_f32_dev": _fill(False),
            "cvs_color_matrix_f16_dev": _colour_matrix, "cvs_color_matrix_f16_to_dev": _colour_matrix_to,
            "cvs_fir_blur_f16_dev": _blur_f16,
            "cvs_chroma_key_f16_dev": _model_call(_key), "cvs_chroma_key_f32_dev": _model_call(_key),
            "cvs_matte_refine_f16_dev": _model_call(_matte), "cvs_matte_refine_f32_dev": _model_call(_matte),
            "cvs_transform_f16_dev": _model_call(_transform), "cvs_transform_f32_dev": _model_call(_transform),
            "cvs_field_to_frame_f16_dev": _model_call(_field), "cvs_soften_fields_f16_dev": _model_call(_soften),
            "cvs_interlace_fields_f16_dev": _interlace,
            "cvs_unsharp_mask_f16_dev": _model_call(_unsharp), "cvs_unsharp_mask_f32_dev": _model_call(_unsharp)}


class OnHostWithBuffers(OnHost):
    """OnHost whose flat buffers (coded planes, byte targets, lattices, count tables) are host memory too."""

    def _make_frame(self, o, host):
        OnHost._make_frame(self, o, host)
        o.frame.ptr = o.ptr                              # (what a case reads where it hands a frame's address on, as a DeviceFrame's)

    def _make_buffer(self, o, data):
        o.array = np.array(data, np.uint8)
        o.ptr = o.array.ctypes.data

    def collect(self):
        return [o.frame.array.copy() if o.frame is not None else o.array.copy() for o in self.objects]


class ReferenceLibrary(OracleAsLibrary):
    """OracleAsLibrary with the wider map: what tests/extent_cases.py is held to.  The workspace's device slot is the oracle's
    stack (orc_workspace_get_frame_f32, as tests/test_gpu_parity.py test_workspace_stack_host_and_device holds it) over
    sources whose host slots pull through the case's own device slot, which on this side works on host memory."""
    tables = (ORACLE, dict(COMPOSED, **MODELLED, **EXTENSIONS))

    def workspace_create(self):
        return []

    def workspace_add_item(self, ws, source, x, length, offset, z, _tag):
        ws.append((C.cast(source, C.POINTER(video_source)), x, length, offset, z))

    def workspace_as_video_source(self, ws, _vs):
        self._stack = ws

    def workspace_free(self, ws):
        self._stack = None

    def video_get_frame_dev(self, _vs, index, d):
        d = _struct(d)
        keep, items = [], []
        for src, x, length, offset, z in self._stack:
            slot = ec.GET_FRAME_DEV(src.contents.funcs.contents.get_frame_dev)

            def pull(fmt, slot=slot, src=src):
                def cb(_self, idx, fp):
                    f = fp.contents
                    dev = _lib.rgba_frame_dev(C.cast(f.data, C.c_void_p).value, fmt, f.full_window, f.full_window, None)
                    slot(src.contents.obj, idx, C.byref(dev))
                    f.current_window = dev.current_window
                return cb
            funcs = video_frame_source_funcs(0, GET_FRAME_F16(pull(ec.FORMAT_F16)), GET_FRAME_F32(pull(ec.FORMAT_F32)), None)
            wrapped = video_source(None, C.pointer(funcs))
            keep += [funcs, wrapped]
            items.append(oracle.ws_item(x, length, z, offset, C.pointer(wrapped)))
        want = HostFrame(d.full_window.tuple(), np.float32)
        oracle.lib().orc_workspace_get_frame_f32((oracle.ws_item * len(items))(*items), len(items), index, want.ref())
        win = _tuple_or_none(want.current_window)
        d.current_window = type(d.current_window).of(*(win or (0, 0, -1, -1)))
        if win is not None:
            half = d.format == ec.FORMAT_F16
            cls = _lib.rgba_frame_f16_t if half else _lib.rgba_frame_f32_t
            target = cls(d.data, d.full_window, d.full_window)
            _inside(target, win)[...] = oracle.float_to_half(want.window_view()) if half else want.window_view()
