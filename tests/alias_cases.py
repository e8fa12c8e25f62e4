"""The catalogue of device-entry calls on operands that SHARE A BUFFER (include/canvas_hip.h "Operands that share a buffer";
DESIGN.md "Operands that share a buffer"), in the form of tests/entry_cases.py, whose factories, pixels, tap lists, pins and
geometries it reuses.

Two frame operands share a buffer when their `data` pointers and their `full_window`s are equal.  For every pair of frame
operands of every cvs_*_dev entry of the five headers -- a frame the entry writes against one it reads, or two it reads --
ALIAS_POLICY states what the header states:

  "in place"  the entry computes, bit for bit, what the same call gives on a distinct copy of the shared input
  "refused"   the entry returns nonzero before it launches, looks up or allocates anything, cvs_last_error() names it with
              one of WORDINGS, and the target's window is empty
  "shared"    both operands are only read

and EXEMPT lists the entries that have no such pair, each with the property of the ENTRY that excludes it.  Out of scope, as
the header says (they stay the caller's error): two structs with equal `data` and different `full_window`s, buffers that
overlap at a shifted address, and two operands that are both written.  The chain and the scaler batches do detect shifted
overlap; they keep the tests they have (tests/test_gpu_parity.py test_chain_shifted_overlap_of_output_and_layer_is_not_fused,
test_scale_batch_falls_back_on_mixed_geometry_and_overlap).

A case is run(fac, form): ONE call on operands from the factory `fac`, in one of three forms --

  "distinct"     every operand a frame of its own; the second operand of the pair holds the same pixels and window as the first
                 (the expectation: tests/reference_library.py runs this form, and the GPU module runs it on a twin)
  "one struct"   one frame struct handed in for both parameters of the pair
  "two structs"  two structs with equal data, full_window and current_window (what the call does to the output's window no
                 longer disturbs the input's)

The objects of the two sharing forms are those of the distinct form without the ones named DISTINCT..., in the same order.
tests/test_alias_cases_cpu.py holds the table to the headers and the catalogue to the table without a GPU;
tests/test_aliasing_gpu.py runs it."""
import ctypes as C

import numpy as np

import oracle
from canvas_amd import _lib, synth
from canvas_amd.abi import HostFrame, v2f
from tests import deinterlace_model as dm
from tests import entry_cases as ec
from tests import lut3d_model as lm
from tests import perspective_model as pm
from tests import reference_library as rl
from tests.entry_cases import blank, px, px16, px32
from tests.util import f32p

IN_PLACE, REFUSED, SHARED = "in place", "refused", "shared"
WORDINGS = ("the target is the source's buffer: the operation is not in place", "the output cannot be one of the inputs")
FORMS = ("one struct", "two structs")
DISTINCT = "distinct copy: "

_T_S = {("target", "source"): REFUSED}
_POINTWISE = {("target", "source"): IN_PLACE}
_BATCH = {("targets", "sources"): REFUSED, ("sources", "sources"): SHARED}

# entry -> {(written operand, read operand): "in place" | "refused"} + {(read operand, read operand): "shared"}, by the
# parameter names of the headers; a table of frame pointers is named once and pairs with itself, a cvs_chain_job is its
# `out` and its `layers`
ALIAS_POLICY = {
    # one lane per element (or per vector of eight; the vector path needs BOTH pointers on the 16-byte grid): reads what it writes
    "cvs_half_lookup_dev": {("out", "in"): IN_PLACE},
    # one lane per pixel, read at the address it is written to (kernels/frame_ops.hip, color_ops.hip)
    "cvs_copy_frame_f16_dev": {("out", "in"): IN_PLACE},
    "cvs_copy_frame_alpha_f32_dev": {("out", "in"): IN_PLACE},
    "cvs_gain_offset_f16_dev": {("out", "in"): IN_PLACE},
    "cvs_color_matrix_f16_to_dev": {("out", "in"): IN_PLACE},
    # kernels/mix_ops.hip: a lane reads p and q at the linear address of the pixel it writes, the `left` quirk included
    "cvs_mix_cross_f32_dev": {("out", "a"): IN_PLACE, ("out", "b"): IN_PLACE, ("a", "b"): SHARED},
    "cvs_mix_over_f32_dev": {("out", "b"): IN_PLACE},
    # fused: a lane reads a pixel pair of every layer before it writes that pair; node by node: the output is written last
    "cvs_mix_cross_f16_dev": {("out", "a"): IN_PLACE, ("out", "b"): IN_PLACE, ("a", "b"): SHARED},
    "cvs_chain_color_over_f16_dev": {("out", "layers"): IN_PLACE, ("layers", "layers"): SHARED},
    # row streams (host/key.c, host/lut3d.c: "the target may be the source frame itself")
    "cvs_chroma_key_f16_dev": _POINTWISE, "cvs_chroma_key_f32_dev": _POINTWISE,
    "cvs_lut3d_f16_dev": _POINTWISE, "cvs_lut3d_f32_dev": _POINTWISE,
    # k_weave16 reads the second field cur.x0 pixels before the pixel it writes (the reference's row address)
    "cvs_weave_fields_f16_dev": {("frame", "other"): REFUSED},
    # every one of these gathers source pixels that other lanes and other workgroups write as target pixels
    "cvs_field_to_frame_f16_dev": {("out", "in"): REFUSED}, "cvs_soften_fields_f16_dev": {("out", "in"): REFUSED},
    "cvs_interlace_fields_f16_dev": {("out", "even"): REFUSED, ("out", "odd"): REFUSED, ("even", "odd"): SHARED},
    "cvs_matte_refine_f16_dev": _T_S, "cvs_matte_refine_f32_dev": _T_S,
    "cvs_transform_f16_dev": _T_S, "cvs_transform_f32_dev": _T_S,
    "cvs_perspective_f16_dev": _T_S, "cvs_perspective_f32_dev": _T_S,
    "cvs_deinterlace_adaptive_f16_dev": {("out", "prev"): REFUSED, ("out", "cur"): REFUSED, ("out", "next"): REFUSED,
                                         ("prev", "cur"): SHARED, ("prev", "next"): SHARED, ("cur", "next"): SHARED},
    "cvs_fir_blur_f32_dev": _T_S, "cvs_fir_blur_f16_dev": _T_S,
    "cvs_unsharp_mask_f32_dev": _T_S, "cvs_unsharp_mask_f16_dev": _T_S,
    "cvs_resample_lanczos_f32_dev": _T_S, "cvs_resample_lanczos_f16_dev": _T_S,
    "cvs_scale_bilinear_f32_dev": _T_S, "cvs_scale_bilinear_f16_dev": _T_S,
    "cvs_scale_bilinear_f32_batch_dev": _BATCH, "cvs_scale_bilinear_f16_batch_dev": _BATCH,
    "cvs_blur_lanczos_f16_dev": _T_S, "cvs_blur_lanczos_f16_batch_dev": _BATCH,
    # the blur gathers from the source; an overlay is read where, and before, the output pixel is written (blur_kernel.hpp EPI),
    # and node by node the output is written last
    "cvs_blur_over_f16_dev": {("out", "source"): REFUSED, ("out", "overlays"): IN_PLACE, ("source", "overlays"): SHARED,
                              ("overlays", "overlays"): SHARED},
    "cvs_blur_over_f16_batch_dev": {("outs", "sources"): REFUSED, ("outs", "overlays"): IN_PLACE, ("sources", "sources"): SHARED,
                                    ("sources", "overlays"): SHARED, ("overlays", "overlays"): SHARED},
}

_ONE_FRAME = "takes one frame"
_PLANES = "its other operand is coded planes of bytes, no frame"
_BYTES = "its other operand is display bytes, no frame"
_TYPES = "its two operands have different element types and cannot share a buffer of one full_window"
EXEMPT = {
    "cvs_fill_solid_f16_dev": _ONE_FRAME, "cvs_fill_solid_f32_dev": _ONE_FRAME, "cvs_color_matrix_f16_dev": _ONE_FRAME,
    "cvs_reconstruct_dv_dev": _PLANES, "cvs_subsample_dv_dev": _PLANES, "cvs_reconstruct_mpeg2_dev": _PLANES, "cvs_subsample_mpeg2_dev": _PLANES,
    "cvs_frame_to_bytes_dev": _BYTES, "cvs_frame_to_rgba8_intent_dev": _BYTES,
    "cvs_scope_counts_f16_dev": "its other operand is a table of 32-bit counts, no frame",
    "cvs_scope_render_f16_dev": "takes one frame, beside a table of 32-bit counts",
    "cvs_half_to_float_dev": _TYPES, "cvs_half_to_float_fast_dev": _TYPES, "cvs_float_to_half_dev": _TYPES, "cvs_float_to_half_fast_dev": _TYPES,
    "cvs_frame_f16_to_f32_dev": _TYPES, "cvs_frame_f32_to_f16_dev": _TYPES,
}
# "in place" cases whose result IS the input, by the entry's definition, whatever the parameters: (entry, pair, text in
# the case's name) -> why
IDENTITY = {("cvs_copy_frame_f16_dev", ("out", "in"), ""): "a copy of a window onto itself",
            ("cvs_chain_color_over_f16_dev", ("out", "layers"), "of 1 layers, whole, plain"): "a stack of one layer without a colour stage: widened and truncated again",
            ("cvs_chain_color_over_f16_dev", ("out", "layers"), "of 1 layers, inside, plain"): "a stack of one layer without a colour stage: widened and truncated again"}


# ------------------------------------------------------------------ the pair of operands

class _Struct:
    """A second struct over a frame's buffer: equal data, full_window and current_window."""

    def __init__(self, frame):
        self.c = type(frame.c)(frame.c.data, frame.c.full_window, frame.c.current_window)

    def ref(self):
        return C.byref(self.c)


def pair(fac, form, host, out, cmp="exact", name=None, other="the operand that shares its buffer"):
    """-> (first, second): the pair's first operand, a frame of `host`'s pixels from the factory (written when `out`), and
    its second, which is -- by `form` -- a frame of its own with the same pixels, the first itself, or a second struct over
    the first's buffer."""
    first = fac.frame(host, out=out, cmp=cmp, name=name, in_place=out)
    if form == "distinct":
        return first, fac.frame(host, name=DISTINCT + other)
    assert form in FORMS, form
    return first, (first if form == "one struct" else _Struct(first))


class Case:
    """One call: run(fac, form) -> the entry's return code.  `pair`: the operands that share; `pin`: the FIR path in force."""

    def __init__(self, what, entry, pair_, run, pin=None):
        self.what, self.entry, self.pair, self.run, self.pin = what, entry, pair_, run, pin
        self.policy = ALIAS_POLICY[entry][pair_]
        # an "in place" case whose result IS its input, by the entry's definition (IDENTITY): the reason, or None
        self.identity = next((why for (e, p, text), why in IDENTITY.items() if e == entry and p == pair_ and text in what), None)

    def __call__(self, fac, form):
        return self.run(fac, form)


# (name, full window, current window): the window is the whole buffer (33 x 7); it lies strictly inside a buffer of
# 131 x 41 and starts on an odd column
GEOMETRIES = [("whole", (0, 0, 32, 6), (0, 0, 32, 6)), ("inside", (0, 0, 130, 40), (3, 2, 127, 37))]
_FMT = {True: "f16", False: "f32"}


def _two_frames(entry, half, call, names=("target", "source"), pins=(None,), geometries=GEOMETRIES, seed=4000, tag=""):
    """An entry of the form (written frame, read frame, parameters): every geometry under every pin."""
    cases = []
    for pin in pins:
        for gname, full, cur in geometries:
            def run(fac, form, full=full, cur=cur):
                t, s = pair(fac, form, px(np.random.default_rng(seed), half, full, cur), True, _FMT[half], names[0], names[1])
                return call(fac, t, s)
            cases.append(Case("%s%s, %s == %s, %s%s" % (entry, tag and " " + tag, names[0], names[1], gname, "" if pin is None else ", pinned %r" % (pin,)), entry, names, run, pin))
    return cases


# ------------------------------------------------------------------ pointwise entries: in place

KEY_SETTINGS = [dict(key=(0.1, 0.8, 0.15), tolerance=0.05, softness=3.0, spill=0.8, spill_range=0.4, flags=0),     # a ramp wider than the plane
                ec.KEY_SETTINGS[1]]                                                                               # the matte shown
LUT_SIZES = [17, 33]


def pointwise(cvs):
    cases = []
    cases += _two_frames("cvs_copy_frame_f16_dev", True, lambda fac, t, s: cvs.cvs_copy_frame_f16_dev(t.ref(), s.ref(), fac.stream), ("out", "in"))
    cases += _two_frames("cvs_copy_frame_alpha_f32_dev", False, lambda fac, t, s: cvs.cvs_copy_frame_alpha_f32_dev(t.ref(), s.ref(), C.c_float(0.4), fac.stream), ("out", "in"))
    cases += _two_frames("cvs_gain_offset_f16_dev", True, lambda fac, t, s: cvs.cvs_gain_offset_f16_dev(t.ref(), s.ref(), C.c_float(1.5), C.c_float(0.0625), fac.stream), ("out", "in"))
    m = np.array(ec.REC709_RGB_TO_YPBPR, np.float32)
    for pre, post in ec.COLOUR_MATRIX_TABLES:
        cases += _two_frames("cvs_color_matrix_f16_to_dev", True,
                             lambda fac, t, s, pre=pre, post=post: cvs.cvs_color_matrix_f16_to_dev(t.ref(), s.ref(), f32p(m), pre, post, fac.stream), ("out", "in"),
                             tag="tables %d, %d" % (pre, post))
    for half in (True, False):
        for p in KEY_SETTINGS:
            params = _lib.chroma_key((C.c_float * 3)(*p["key"]), p["tolerance"], p["softness"], p["spill"], p["spill_range"], p["flags"])
            entry = "cvs_chroma_key_%s_dev" % _FMT[half]
            cases += _two_frames(entry, half, lambda fac, t, s, entry=entry, params=params: getattr(cvs, entry)(t.ref(), s.ref(), C.byref(params), fac.stream),
                                 tag="flags %d" % p["flags"])
        for size in LUT_SIZES:
            entry = "cvs_lut3d_%s_dev" % _FMT[half]

            def lut(fac, t, s, entry=entry, size=size):
                p = _lib.lut3d(size)
                lattice = fac.buffer(lm.packed(lm.distinct(size, size)), "f32", name="lattice")
                return getattr(cvs, entry)(t.ref(), s.ref(), lattice, C.byref(p), fac.stream)
            cases += _two_frames(entry, half, lut, tag="N=%d" % size)
    return cases


def half_lookup(cvs):
    """out == in, on the 16-byte grid (eight elements per lane) and off it."""
    cases = []
    for n, skip in ((4099, 0), (4099, 6), (7, 2)):
        def run(fac, form, n=n, skip=skip):
            rng = np.random.default_rng(4100)
            table = fac.buffer(rng.integers(0, 65536, 65536).astype(np.uint16), "plane", name="table")
            codes = rng.integers(0, 65536, n + skip // 2).astype(np.uint16)
            array = fac.buffer(codes, "plane", out=True, name="half array")
            src = fac.buffer(codes, "plane", name=DISTINCT + "the input") if form == "distinct" else array
            return cvs.cvs_half_lookup_dev(table, array + skip, src + skip, n, fac.stream)
        cases.append(Case("cvs_half_lookup_dev, out == in, %d elements from byte %d" % (n, skip), "cvs_half_lookup_dev", ("out", "in"), run))
    return cases


# ------------------------------------------------------------------ mixers

FULL = ec.FULL
_WINDOWS = sorted({w for p in ec.MIX_WINDOWS for w in p})


def mixers(cvs):
    """out == a, out == b and a == b of the two crossfades, out == b of the over.  The pair's operands have one window, so
    the window pairs of entry_cases.MIX_WINDOWS -- the `left` selector pair among them -- go to the shared operand and the
    other input; where both inputs are the pair, every window of those pairs is run."""
    cases = []
    for half in (True, False):
        entry = "cvs_mix_cross_%s_dev" % _FMT[half]
        fmt = _FMT[half]                                   # (the entry is looked up when the case runs: the oracle's flavour is the run's)
        for g, (pw, qw) in enumerate(ec.MIX_WINDOWS):
            def out_a(fac, form, g=g, pw=pw, qw=qw, entry=entry, half=half, fmt=fmt):
                rng = np.random.default_rng(4200 + g)
                out, a = pair(fac, form, px(rng, half, FULL, pw), True, fmt, "out", "a")
                b = fac.frame(px(rng, half, FULL, qw), name="b")
                return getattr(cvs, entry)(out.ref(), a.ref(), b.ref(), C.c_float(0.2), fac.stream)

            def out_b(fac, form, g=g, pw=pw, qw=qw, entry=entry, half=half, fmt=fmt):
                rng = np.random.default_rng(4250 + g)
                a = fac.frame(px(rng, half, FULL, pw), name="a")
                out, b = pair(fac, form, px(rng, half, FULL, qw), True, fmt, "out", "b")
                return getattr(cvs, entry)(out.ref(), a.ref(), b.ref(), C.c_float(0.2), fac.stream)
            cases += [Case("%s, out == a, windows %r" % (entry, (pw, qw)), entry, ("out", "a"), out_a),
                      Case("%s, out == b, windows %r" % (entry, (pw, qw)), entry, ("out", "b"), out_b)]
        for g, w in enumerate(_WINDOWS):
            def a_b(fac, form, g=g, w=w, entry=entry, half=half, fmt=fmt):
                a, b = pair(fac, form, px(np.random.default_rng(4300 + g), half, FULL, w), False, name="a", other="b")
                out = fac.frame(blank(half, FULL), out=True, cmp=fmt, name="out")
                return getattr(cvs, entry)(out.ref(), a.ref(), b.ref(), C.c_float(0.2), fac.stream)
            cases.append(Case("%s, a == b, window %r" % (entry, w), entry, ("a", "b"), a_b))
    for g, w in enumerate(_WINDOWS):
        def over(fac, form, g=g, w=w):
            out, b = pair(fac, form, px32(np.random.default_rng(4350 + g), FULL, w), True, "f32", "out", "b")
            return cvs.cvs_mix_over_f32_dev(out.ref(), b.ref(), C.c_float(0.35), fac.stream)
        cases.append(Case("cvs_mix_over_f32_dev, out == b, window %r" % (w,), "cvs_mix_over_f32_dev", ("out", "b"), over))
    return cases


# ------------------------------------------------------------------ the chain

CHAIN_LAYERS = [1, 2, 4, 8]
# the whole buffer (the fused kernel) and a window inside it from an odd column (node by node through pooled frames)
CHAIN_WINDOWS = [("whole", (0, 0, 63, 35)), ("inside", (3, 2, 60, 33))]


def chain(cvs):
    """out == layer k for the first, a middle and the last layer of 1, 2, 4 and 8; one layer at two positions; plain and with
    the matrix and a table."""
    full = (0, 0, 63, 35)
    cases = []
    for plain in (True, False):
        m = None if plain else np.array(ec.REC709_RGB_TO_YPBPR, np.float32)
        pre = _lib.LUT_NONE if plain else _lib.LUT_REC709_TO_LINEAR_SCENE
        for wname, win in CHAIN_WINDOWS:
            for n in CHAIN_LAYERS:
                def run(fac, form, shared, written, n=n, win=win, m=m, pre=pre):
                    """`shared`: the two layer positions of the pair, or (k,) with `written`: out is layer k"""
                    rng = np.random.default_rng(4400 + n)
                    hosts = [px16(rng, full, win) for _ in range(n)]
                    layers, out = [None] * n, None
                    for k in range(n):
                        if written and k == shared[0]:
                            out, layers[k] = pair(fac, form, hosts[k], True, "f16", "chain output", "layer %d" % k)
                        elif not written and k == shared[0]:
                            layers[k], layers[shared[1]] = pair(fac, form, hosts[k], False, name="layer %d" % k, other="layer %d" % shared[1])
                        elif layers[k] is None:
                            layers[k] = fac.frame(hosts[k], name="layer %d" % k)
                    if out is None:
                        out = fac.frame(blank(True, full), out=True, cmp="f16", name="chain output")
                    jobs = (_lib.chain_job * 1)()
                    jobs[0].out = C.pointer(out.c)
                    for k, l in enumerate(layers):
                        jobs[0].layers[k] = C.pointer(l.c)
                    jobs[0].nlayers = n
                    return cvs.cvs_chain_color_over_f16_dev(jobs, 1, None if m is None else f32p(m), pre, _lib.LUT_NONE, fac.stream)
                tail = "%d layers, %s%s" % (n, wname, ", plain" if plain else "")
                for k in sorted({0, n // 2, n - 1}):
                    cases.append(Case("chain, out == layer %d of %s" % (k, tail), "cvs_chain_color_over_f16_dev", ("out", "layers"),
                                      lambda fac, form, run=run, k=k: run(fac, form, (k,), True)))
                if n > 1:
                    cases.append(Case("chain, layer 0 == layer %d of %s" % (n - 1, tail), "cvs_chain_color_over_f16_dev", ("layers", "layers"),
                                      lambda fac, form, run=run, n=n: run(fac, form, (0, n - 1), False)))
    return cases


# ------------------------------------------------------------------ blur + over and its batch

# (name, size, source window, taps, overlay windows): the one-launch form (whole windows, an odd list) and node by node
BLUR_OVER_SHAPES = [("in one launch, 300x41, 9 taps", (300, 41), None, 9, [None] * 3),
                    ("in one launch, 64x36, 15 taps", (64, 36), None, 15, [None] * 3),
                    ("node by node, ragged overlays", (60, 34), None, 9, [(5, 3, 40, 25), (20, 2, 59, 20), (1, 1, 58, 30)]),
                    ("node by node, 4 taps", (60, 34), None, 4, [None] * 3),
                    ("node by node, a small source window", (60, 34), (5, 2, 50, 30), 9, [None] * 3)]


def blur_over(cvs, columns):
    """out == source (refused), out == the first and the last of three overlays, an overlay == the source, two overlays one
    frame: in the one-launch form and node by node (entry_cases.blur_over_forms), to be run under COLUMN_PINS[columns]."""
    entry = "cvs_blur_over_f16_dev"
    cases = []
    for sname, (w, h), scur, ntaps, wins in BLUR_OVER_SHAPES:
        full = (0, 0, w - 1, h - 1)
        taps = synth.gaussian_taps(ntaps | 1, 1.5)[:ntaps].copy()

        def run(fac, form, which, full=full, scur=scur, ntaps=ntaps, wins=wins, taps=taps):
            rng = np.random.default_rng(4500 + ntaps)
            hs = px16(rng, full, scur or full)
            ho = [px16(rng, full, win or full) for win in wins]
            src, out, ov = None, None, [None] * len(ho)
            if which == "out == source":
                out, src = pair(fac, form, hs, True, "f16", "blur output", "blur source")
            elif which == "overlay == source":
                src, ov[1] = pair(fac, form, hs, False, name="blur source", other="overlay 1")
            else:
                src = fac.frame(hs, name="blur source")
            for k in range(len(ho)):
                if which == "out == overlay %d" % k:
                    out, ov[k] = pair(fac, form, ho[k], True, "f16", "blur output", "overlay %d" % k)
                elif which == "overlay 0 == overlay 2" and k == 0:
                    ov[0], ov[2] = pair(fac, form, ho[0], False, name="overlay 0", other="overlay 2")
                elif ov[k] is None:
                    ov[k] = fac.frame(ho[k], name="overlay %d" % k)
            if out is None:
                out = fac.frame(blank(True, full), out=True, cmp="f16", name="blur output")
            table = (C.POINTER(_lib.rgba_frame_f16_t) * len(ov))(*[C.pointer(o.c) for o in ov])
            return cvs.cvs_blur_over_f16_dev(out.ref(), src.ref(), f32p(taps), ntaps, table, len(ov), fac.stream)
        for which, names in (("out == source", ("out", "source")), ("out == overlay 0", ("out", "overlays")), ("out == overlay 2", ("out", "overlays")),
                             ("overlay == source", ("source", "overlays")), ("overlay 0 == overlay 2", ("overlays", "overlays"))):
            cases.append(Case("blur over %s, %s, columns %r" % (sname, which, columns), entry, names,
                              lambda fac, form, run=run, which=which: run(fac, form, which), ec.COLUMN_PINS[columns]))
    return cases


def blur_over_batch(cvs, columns):
    """Three frames, one overlay each: target i == source i for every i (refused), output i == overlay i, one source under
    all frames, overlay i == source i, one overlay over all frames."""
    entry = "cvs_blur_over_f16_batch_dev"
    cases = []
    for (w, h), ntaps, win in (((130, 40), 9, None), ((131, 41), 4, None), ((131, 41), 9, (3, 2, 127, 37))):
        full = (0, 0, w - 1, h - 1)
        taps = ec._taps(ntaps)

        def run(fac, form, which, full=full, ntaps=ntaps, taps=taps, win=win):
            rng = np.random.default_rng(4600 + ntaps)
            hs, ho = [px16(rng, full, win) for _ in range(3)], [px16(rng, full, win) for _ in range(3)]
            srcs, ovs, outs = [None] * 3, [None] * 3, [None] * 3
            for k in range(3):
                if which == "targets == sources":
                    outs[k], srcs[k] = pair(fac, form, hs[k], True, "f16", "blur output %d" % k, "blur source %d" % k)
                elif which == "one source" and k == 0:
                    srcs[0], srcs[1] = pair(fac, form, hs[0], False, name="blur source 0", other="blur source 1")
                    srcs[2] = srcs[0] if form != "distinct" else fac.frame(hs[0], name=DISTINCT + "blur source 2")
                elif which == "overlays == sources":
                    srcs[k], ovs[k] = pair(fac, form, hs[k], False, name="blur source %d" % k, other="overlay of frame %d" % k)
                elif srcs[k] is None:
                    srcs[k] = fac.frame(hs[k], name="blur source %d" % k)
            for k in range(3):
                if which == "outputs == overlays":
                    outs[k], ovs[k] = pair(fac, form, ho[k], True, "f16", "blur output %d" % k, "overlay of frame %d" % k)
                elif which == "one overlay" and k == 0:
                    ovs[0], ovs[1] = pair(fac, form, ho[0], False, name="overlay of frame 0", other="overlay of frame 1")
                    ovs[2] = ovs[0] if form != "distinct" else fac.frame(ho[0], name=DISTINCT + "overlay of frame 2")
                elif ovs[k] is None:
                    ovs[k] = fac.frame(ho[k], name="overlay of frame %d" % k)
            for k in range(3):
                if outs[k] is None:
                    outs[k] = fac.frame(blank(True, full), out=True, cmp="f16", name="blur output %d" % k)
            tab = lambda frames: (C.POINTER(_lib.rgba_frame_f16_t) * 3)(*[C.pointer(f.c) for f in frames])
            return cvs.cvs_blur_over_f16_batch_dev(tab(outs), tab(srcs), f32p(taps), ntaps, tab(ovs), 1, 3, fac.stream)
        for which, names in (("targets == sources", ("outs", "sources")), ("outputs == overlays", ("outs", "overlays")), ("one source", ("sources", "sources")),
                             ("overlays == sources", ("sources", "overlays")), ("one overlay", ("overlays", "overlays"))):
            cases.append(Case("blur over batch %dx%d, %d taps%s, %s, columns %r" % (w, h, ntaps, ", windows inside" if win else "", which, columns), entry, names,
                              lambda fac, form, run=run, which=which: run(fac, form, which), ec.COLUMN_PINS[columns]))
    return cases


# ------------------------------------------------------------------ host/scale.c: refused under every pin, whatever kernel would take the call

SCALE_TAPS = [3, 9, 15, 4]
_SCALE_PINS = sorted({c[2] for c in ec.SCALE_CASES}, key=str)


def _batch_of(half, run_batch, entry, pins, geometries=GEOMETRIES, tag=""):
    """A batch entry (targets, sources): target i == source i for every frame (refused as a whole), and one source under
    all three frames (shared)."""
    cls = _lib.rgba_frame_f16_t if half else _lib.rgba_frame_f32_t
    tab = lambda frames: (C.POINTER(cls) * 3)(*[C.pointer(f.c) for f in frames])
    cases = []
    for pin in pins:
        for gname, full, cur in geometries:
            def refused(fac, form, full=full, cur=cur):
                rng = np.random.default_rng(4700)
                outs, srcs = zip(*[pair(fac, form, px(rng, half, full, cur), True, _FMT[half], "target %d" % k, "source %d" % k) for k in range(3)])
                return run_batch(fac, tab(outs), tab(srcs))

            def one_source(fac, form, full=full, cur=cur):
                host = px(np.random.default_rng(4701), half, full, cur)
                s0, s1 = pair(fac, form, host, False, name="source 0", other="source 1")
                s2 = s0 if form != "distinct" else fac.frame(host, name=DISTINCT + "source 2")
                outs = [fac.frame(blank(half, full), out=True, cmp=_FMT[half], name="target %d" % k) for k in range(3)]
                return run_batch(fac, tab(outs), tab([s0, s1, s2]))
            tail = "%s%s%s" % (gname, tag and ", " + tag, "" if pin is None else ", pinned %r" % (pin,))
            cases += [Case("%s, target i == source i, %s" % (entry, tail), entry, ("targets", "sources"), refused, pin),
                      Case("%s, one source under all frames, %s" % (entry, tail), entry, ("sources", "sources"), one_source, pin)]
    return cases


def scale_entries(cvs):
    cases = []
    for half in (True, False):
        fmt = _FMT[half]
        for ntaps in SCALE_TAPS:
            taps = ec._taps(ntaps)
            entry = "cvs_fir_blur_%s_dev" % fmt
            cases += _two_frames(entry, half, lambda fac, t, s, entry=entry, taps=taps, ntaps=ntaps: getattr(cvs, entry)(t.ref(), s.ref(), f32p(taps), ntaps, fac.stream),
                                 tag="%d taps" % ntaps)
            entry = "cvs_unsharp_mask_%s_dev" % fmt
            cases += _two_frames(entry, half, lambda fac, t, s, entry=entry, taps=taps, ntaps=ntaps:
                                 getattr(cvs, entry)(t.ref(), s.ref(), f32p(taps), ntaps, C.c_float(0.7), C.c_float(0.01), fac.stream), tag="%d taps" % ntaps)
        entry = "cvs_resample_lanczos_%s_dev" % fmt
        cases += _two_frames(entry, half, lambda fac, t, s, entry=entry: getattr(cvs, entry)(t.ref(), s.ref(), C.c_float(0.5), C.c_float(0.5), 3, fac.stream), pins=ec.LANCZOS_PINS)
        entry = "cvs_scale_bilinear_%s_dev" % fmt
        for factors in ((2.0, 2.0), (0.4, 0.35), (1.0, 1.0)):           # (1, 1) with equal points: the path that forwards to the copy
            cases += _two_frames(entry, half, lambda fac, t, s, entry=entry, factors=factors:
                                 getattr(cvs, entry)(t.ref(), fac.point(0, 0), s.ref(), fac.point(0, 0, source=True), v2f(*factors), fac.stream),
                                 pins=_SCALE_PINS if factors[0] == 2.0 else (None,), tag="x%r" % (factors,))
        entry = "cvs_scale_bilinear_%s_batch_dev" % fmt
        cases += _batch_of(half, lambda fac, outs, srcs, entry=entry: getattr(cvs, entry)(outs, fac.point(0, 0), srcs, fac.point(0, 0, source=True), v2f(2.0, 2.0), 3, fac.stream),
                           entry, _SCALE_PINS)
    for ntaps in ec.BLUR_LANCZOS_TAPS:
        taps = np.array([1.0], np.float32) if ntaps == 1 else ec._taps(ntaps)
        cases += _two_frames("cvs_blur_lanczos_f16_dev", True, lambda fac, t, s, taps=taps, ntaps=ntaps:
                             cvs.cvs_blur_lanczos_f16_dev(t.ref(), s.ref(), f32p(taps), ntaps, C.c_float(0.5), C.c_float(0.5), 3, fac.stream), pins=ec.BLUR_LANCZOS_PINS, tag="%d taps" % ntaps)
        cases += _batch_of(True, lambda fac, outs, srcs, taps=taps, ntaps=ntaps:
                           cvs.cvs_blur_lanczos_f16_batch_dev(outs, srcs, 3, f32p(taps), ntaps, C.c_float(0.5), C.c_float(0.5), 3, fac.stream),
                           "cvs_blur_lanczos_f16_batch_dev", ec.BLUR_LANCZOS_PINS, tag="%d taps" % ntaps)
    return cases


# ------------------------------------------------------------------ the other spatial entries: refused (the checks they had, and the weave's)

def spatial(cvs):
    cases = []
    # the second field's buffer is allocated for the frame's current window: sharing means that window is the whole buffer
    cases += _two_frames("cvs_weave_fields_f16_dev", True, lambda fac, t, s: cvs.cvs_weave_fields_f16_dev(t.ref(), s.ref(), fac.stream), ("frame", "other"),
                         geometries=[("whole", (0, 0, 32, 6), (0, 0, 32, 6)), ("whole, from an odd column", (3, 2, 29, 14), (3, 2, 29, 14))])
    for field in (0, 1):
        cases += _two_frames("cvs_field_to_frame_f16_dev", True, lambda fac, t, s, field=field: cvs.cvs_field_to_frame_f16_dev(t.ref(), s.ref(), field, fac.stream), ("out", "in"),
                             tag="field %d" % field)
    cases += _two_frames("cvs_soften_fields_f16_dev", True, lambda fac, t, s: cvs.cvs_soften_fields_f16_dev(t.ref(), s.ref(), fac.stream), ("out", "in"))
    for gname, full, cur in GEOMETRIES:
        def interlace(fac, form, which, full=full, cur=cur):
            rng = np.random.default_rng(4800)
            he, hd = px16(rng, full, cur), px16(rng, full, cur)
            if which == "even == odd":
                even, odd = pair(fac, form, he, False, name="even", other="odd")
                out = fac.frame(blank(True, full), out=True, name="out")
            elif which == "out == even":
                out, even = pair(fac, form, he, True, name="out", other="even")
                odd = fac.frame(hd, name="odd")
            else:
                even = fac.frame(he, name="even")
                out, odd = pair(fac, form, hd, True, name="out", other="odd")
            return cvs.cvs_interlace_fields_f16_dev(out.ref(), even.ref(), odd.ref(), fac.stream)
        for which, names in (("out == even", ("out", "even")), ("out == odd", ("out", "odd")), ("even == odd", ("even", "odd"))):
            cases.append(Case("cvs_interlace_fields_f16_dev, %s, %s" % (which, gname), "cvs_interlace_fields_f16_dev", names,
                              lambda fac, form, interlace=interlace, which=which: interlace(fac, form, which)))
    for half in (True, False):
        fmt = _FMT[half]
        m = _lib.matte(2, ec.ROUGH25, 0.1, 0.9)
        entry = "cvs_matte_refine_%s_dev" % fmt
        cases += _two_frames(entry, half, lambda fac, t, s, entry=entry, m=m: getattr(cvs, entry)(t.ref(), s.ref(), C.byref(m), fac.stream))
        entry = "cvs_transform_%s_dev" % fmt

        def warp(fac, t, s, entry=entry):
            p = _lib.transform(fac.matrix((1.0, 0.0, 0.5, 0.0, 1.0, 0.5)), _lib.TRANSFORM_BILINEAR)
            return getattr(cvs, entry)(t.ref(), s.ref(), C.byref(p), fac.stream)
        cases += _two_frames(entry, half, warp)
        entry = "cvs_perspective_%s_dev" % fmt

        def pin_corners(fac, t, s, entry=entry):
            rect = pm.outer((0, 0, 32, 6))
            h, to, so = pm.from_quad(rect, [(x + 0.5, y + 0.5) for x, y in pm.rect_quad(rect)])
            p = _lib.perspective(h, to, so, _lib.TRANSFORM_BILINEAR)
            return getattr(cvs, entry)(t.ref(), s.ref(), C.byref(p), fac.stream)
        cases += _two_frames(entry, half, pin_corners)
    return cases


DEINTERLACE = (0.05, 0.1)          # threshold, softness


def deinterlace(cvs):
    """out == prev, out == cur, out == next (refused: tests/test_deinterlace_gpu.py has these too); prev == next and
    prev == cur == next (shared)."""
    entry = "cvs_deinterlace_adaptive_f16_dev"
    cases = []
    for gname, full, cur_w in GEOMETRIES:
        for field in (0, 1):
            def run(fac, form, which, full=full, cur_w=cur_w, field=field):
                rng = np.random.default_rng(4900)
                hp, hc, hn = (HostFrame(full, np.uint16, codes, cur_w) for codes in dm.thirds(rng, full, *DEINTERLACE))
                prev = cur = nxt = out = None
                if which == "out == prev":
                    out, prev = pair(fac, form, hp, True, "f16", "out", "prev")
                elif which == "out == cur":
                    out, cur = pair(fac, form, hc, True, "f16", "out", "cur")
                elif which == "out == next":
                    out, nxt = pair(fac, form, hn, True, "f16", "out", "next")
                elif which == "prev == next":
                    prev, nxt = pair(fac, form, hp, False, name="prev", other="next")
                elif which == "prev == cur":
                    prev, cur = pair(fac, form, hc, False, name="prev", other="cur")
                elif which == "cur == next":
                    cur, nxt = pair(fac, form, hc, False, name="cur", other="next")
                prev = prev or fac.frame(hp, name="prev")
                cur = cur or fac.frame(hc, name="cur")
                nxt = nxt or fac.frame(hn, name="next")
                out = out or fac.frame(blank(True, full), out=True, cmp="f16", name="out")
                p = _lib.deinterlace_adaptive(field, *DEINTERLACE)
                return cvs.cvs_deinterlace_adaptive_f16_dev(out.ref(), prev.ref(), cur.ref(), nxt.ref(), C.byref(p), fac.stream)
            for which in ("out == prev", "out == cur", "out == next", "prev == next", "prev == cur", "cur == next"):
                a, b = which.split(" == ")
                cases.append(Case("%s, %s, %s, field %d" % (entry, which, gname, field), entry, (a, b),
                                  lambda fac, form, run=run, which=which: run(fac, form, which)))

        def all_three(fac, form, full=full, cur_w=cur_w):
            hc = HostFrame(full, np.uint16, dm.thirds(np.random.default_rng(4901), full, *DEINTERLACE)[1], cur_w)
            prev, cur = pair(fac, form, hc, False, name="prev", other="cur")
            nxt = prev if form != "distinct" else fac.frame(hc, name=DISTINCT + "next")
            out = fac.frame(blank(True, full), out=True, cmp="f16", name="out")
            p = _lib.deinterlace_adaptive(0, *DEINTERLACE)
            return cvs.cvs_deinterlace_adaptive_f16_dev(out.ref(), prev.ref(), cur.ref(), nxt.ref(), C.byref(p), fac.stream)
        cases.append(Case("%s, prev == cur == next, %s" % (entry, gname), entry, ("prev", "cur"), all_three))
    return cases


# ------------------------------------------------------------------ every group

def _groups():
    """(id, builder): builder(cvs) -> [Case, ...]; a case is run with cvs_fir_path_override(ec.PINS[case.pin], or the pin
    itself where it is a number) in force."""
    g = [("pointwise", pointwise), ("half_lookup", half_lookup), ("mixers", mixers), ("chain", chain)]
    g += [("blur_over[%s]" % columns, lambda cvs, columns=columns: blur_over(cvs, columns)) for columns in (None, 1, 2)]
    g += [("blur_over_batch[%s]" % columns, lambda cvs, columns=columns: blur_over_batch(cvs, columns)) for columns in (None, 1, 2)]
    g += [("scale_entries", scale_entries), ("spatial", spatial), ("deinterlace", deinterlace)]
    return g


GROUPS = _groups()


def pin_of(case):
    return case.pin if isinstance(case.pin, int) else ec.PINS[case.pin]


# ------------------------------------------------------------------ the reference side

def _deinterlace(out, prev, cur, nxt, params):
    o, p = rl._struct(out), rl._struct(params)
    frame = lambda ref: None if ref is None else (rl._pixels_of(rl._struct(ref), np.uint16), rl._struct(ref).full_window.tuple(),
                                                  rl._tuple_or_none(rl._struct(ref).current_window))
    after, win, _exact, _k = dm.expected(rl._pixels_of(o, np.uint16), o.full_window.tuple(), frame(cur), frame(prev), frame(nxt),
                                         p.field, p.threshold, p.softness, oracle.float_to_half)
    rl._pixels_of(o, np.uint16)[...] = after
    rl._set_window(o, win)


def _half_lookup(table, out, src, count):
    t = rl._bytes_at(table, 65536, np.uint16)
    rl._bytes_at(out, count, np.uint16)[...] = t[rl._bytes_at(src, count, np.uint16).copy()]


class Reference(rl.ReferenceLibrary):
    """tests/reference_library.py ReferenceLibrary with the two entries this catalogue adds to its map."""
    tables = (rl.ORACLE, dict(rl.ReferenceLibrary.tables[1], cvs_deinterlace_adaptive_f16_dev=_deinterlace, cvs_half_lookup_dev=_half_lookup))
