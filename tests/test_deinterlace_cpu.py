"""The adaptive deinterlacer without a GPU (DESIGN.md "Adaptive deinterlace"): include/canvas_deinterlace.h against the library and
its bindings; the identities of the contract on the model alone (tests/deinterlace_model.py); the condition on the test pictures
that keeps the GPU tests from re-testing cvs_field_to_frame only; every refusal of the entry, which comes before the device is
touched; the catalogue of tests/deinterlace_cases.py; the built code object."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from tests import deinterlace_model as dm
from tests import fields_model as fm
from tests.test_perspective_cpu import _declared
from tests.test_unsharp_cpu import _kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "canvas_deinterlace.h"
ENTRY = "cvs_deinterlace_adaptive_f16_dev"
FIELDS = ["field", "threshold", "softness", "flags"]
THRESHOLD, SOFTNESS = 0.05, 0.1


@pytest.fixture(scope="module")
def lib():
    from canvas_amd import _lib
    return _lib.load()


# ---------------------------------------------------------------- the header, the library, the bindings

def test_struct_mirror_has_the_c_layout():
    from canvas_amd import _lib
    assert [name for name, _ in _lib.deinterlace_params._fields_] == FIELDS
    probe = ('#include <stddef.h>\n#include <stdio.h>\n#include "%s"\nint main(void) {\n    printf("%%zu", sizeof(cvs_deinterlace_adaptive));\n' % HEADER
             + "".join('    printf(" %%zu", offsetof(cvs_deinterlace_adaptive, %s));\n' % f for f in FIELDS) + '    printf("\\n");\n    return 0;\n}\n')
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "probe.c"), os.path.join(tmp, "probe")
        with open(src, "w") as f:
            f.write(probe)
        subprocess.run(["gcc", "-std=gnu11", "-I" + os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(_lib.deinterlace_params)] + [getattr(_lib.deinterlace_params, f).offset for f in FIELDS] and got[0] == 16
    p = _lib.deinterlace_adaptive(1, -1.0, 0.5)
    assert (p.field, p.threshold, p.softness, p.flags) == (1, -1.0, 0.5, 0)
    p = _lib.deinterlace_adaptive()
    assert (p.field, p.flags) == (0, 0) and p.threshold == np.float32(0.02) and p.softness == np.float32(0.04)
    F16 = C.POINTER(_lib.rgba_frame_f16)
    assert _lib.DEINTERLACE_SIGNATURES == {ENTRY: (C.c_int, [F16, F16, F16, F16, C.POINTER(_lib.deinterlace_params), C.c_void_p])}


def test_every_symbol_of_the_header_is_exported_and_bound(lib):
    from canvas_amd import _lib
    funcs, entries = _declared(HEADER)
    assert funcs == sorted(_lib.DEINTERLACE_SIGNATURES) == [ENTRY] and entries == [ENTRY]
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert ENTRY in {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert not set(_lib.DEINTERLACE_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.SCOPE_SIGNATURES) | set(_lib.LUT3D_SIGNATURES) | set(_lib.PERSPECTIVE_SIGNATURES))
    assert getattr(lib, ENTRY).argtypes == _lib.DEINTERLACE_SIGNATURES[ENTRY][1] and getattr(lib, ENTRY).restype is C.c_int
    # one launcher, one arithmetic flavour
    symbols = subprocess.run(["nm", _lib.LIB_PATH], stdout=subprocess.PIPE, text=True).stdout
    assert re.search(r"\bcvk_deinterlace_adaptive\b", symbols) and not re.search(r"\bcvk_deinterlace_adaptive_fma\b", symbols)


def test_the_header_compiles_as_c_and_as_cpp():
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "t.c")
        with open(src, "w") as f:
            f.write('#include "%s"\nint main(void) { cvs_deinterlace_adaptive p; p.field = 1; p.flags = 0; p.threshold = 0.02f; p.softness = 0.04f; '
                    'return sizeof p == 16 && p.field == 1 && p.threshold < p.softness ? 0 : 1; }\n' % HEADER)
        for cc, std, lang in (("gcc", "-std=c99", "c"), ("g++", "-std=c++14", "c++")):
            exe = os.path.join(tmp, "t_" + cc)
            subprocess.run([cc, std, "-Wall", "-Werror", "-x", lang, src, "-I", os.path.join(ROOT, "include"), "-o", exe], check=True)
            assert subprocess.run([exe]).returncode == 0


def test_code_object_holds_the_four_instances_without_scratch():
    """One build for both arithmetic flavours; one or two pixels per lane x one or two neighbours; no private segment, no spills."""
    assert os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"), "the ROCm LLVM tools the build itself needs are missing"
    found = _kernels("deinterlace_ops.hip.o")
    assert len(found) == 4 and all("k_deinterlace_adaptive" in n for n in found), sorted(found)
    for pix in (1, 2):
        for neighbours in (1, 2):
            assert any("k_deinterlace_adaptiveILi%dELi%dEEE" % (pix, neighbours) in n for n in found), (pix, neighbours, sorted(found))
    for name, (scratch, spills) in found.items():
        assert scratch == 0 and spills == 0, (name, scratch, spills)
    assert not os.path.exists(os.path.join(ROOT, "canvas_amd", "csrc", "build", "deinterlace_ops.fma.hip.o"))


# ---------------------------------------------------------------- the model: identities of the contract

def _frames(seed, cw, specials=True):
    rng = np.random.default_rng(seed)
    return [(codes, cw, cw) for codes in dm.thirds(rng, cw, THRESHOLD, SOFTNESS, specials)]


SIZES = [(1, 1), (1, 9), (2, 2), (5, 3), (12, 9), (33, 17), (62, 36), (125, 7)]


@pytest.mark.parametrize("width,height", SIZES)
def test_model_identities(orc, width, height):
    f2h = orc.float_to_half
    for y0 in (0, -1):
        cw = (3, y0, 3 + width - 1, y0 + height - 1)
        prev, cur, nxt = _frames(width * 37 + height, cw)
        for field in (0, 1):
            yard = fm.field_to_frame(cur[0], y0, field, f2h)
            # no neighbours, and a threshold nothing stays under: cvs_field_to_frame's codes
            for p, n in ((None, None), ((prev[0], cw, None), None)):
                assert np.array_equal(dm.adaptive(cur, p, n, field, THRESHOLD, SOFTNESS, f2h)[0], yard)
            assert np.array_equal(dm.adaptive(cur, prev, nxt, field, -1.0, 0.0, f2h)[0], yard)
            assert np.array_equal(dm.adaptive(cur, prev, None, field, -1.0, SOFTNESS, f2h)[0], yard)
            # swapping prev and next changes nothing
            a, b = dm.adaptive(cur, prev, nxt, field, THRESHOLD, SOFTNESS, f2h), dm.adaptive(cur, nxt, prev, field, THRESHOLD, SOFTNESS, f2h)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])
        # a still picture comes back code for code -- of finite pixels: inf - inf is NaN, which the contract counts as motion
        still = _frames(width * 37 + height, cw, specials=False)[1]
        for field in (0, 1):
            out, k, copied = dm.adaptive(still, still, still, field, 0.0, 0.0, f2h)
            assert np.array_equal(out, still[0]) and copied.all() and not (k[~np.isnan(k)] != 0).any()


@pytest.mark.parametrize("width,height", [(12, 9), (33, 17), (125, 21)])
def test_model_tiles_equal_the_whole(orc, width, height):
    """split at an even row, an odd row and a column: out.full_window plays no part in what counts"""
    f2h = orc.float_to_half
    cw = (-2, -1, width - 3, height - 2)
    prev, cur, nxt = _frames(5 + width, cw)
    prev = (prev[0], cw, (cw[0] + 1, cw[1] + 2, cw[2], cw[3]))               # a neighbour that covers a part
    before = np.zeros((height, width, 4), np.uint16)
    for field in (0, 1):
        whole, window, _, _ = dm.expected(before, cw, cur, prev, nxt, field, THRESHOLD, SOFTNESS, f2h)
        assert window == cw
        for tiles in ([(cw[0], cw[1], cw[2], 3), (cw[0], 4, cw[2], cw[3])], [(cw[0], cw[1], cw[2], 4), (cw[0], 5, cw[2], cw[3])],
                      [(cw[0], cw[1], 4, cw[3]), (5, cw[1], cw[2], cw[3])]):
            for tile in tiles:
                part, window, _, _ = dm.expected(np.zeros(fm.crop(before, cw, tile).shape, np.uint16), tile, cur, prev, nxt, field, THRESHOLD, SOFTNESS, f2h)
                assert window == tile and np.array_equal(part, fm.crop(whole, cw, tile)), (tile, field)


def test_model_by_hand(orc):
    """three pixels worked out by hand: a kept row, a woven pixel, an interpolated pixel and one on the ramp"""
    f2h = orc.float_to_half
    h = lambda v: np.float16(v).view(np.uint16)
    cw = (0, 0, 6, 2)
    cur = np.empty((3, 7, 4), np.uint16)
    cur[0], cur[1], cur[2] = h(0.25), h(0.75), h(0.5)
    prev = cur.copy()
    prev[1, 6] = h(0.75 + 0.125)                                         # columns 5 and 6 see a difference of 0.125
    prev[0, 3] = h(0.25 + 0.0625)                                        # columns 2 .. 4 see 0.0625
    out, k, copied = dm.adaptive((cur, cw, cw), (prev, cw, cw), None, 0, 0.03125, 0.0625, f2h)
    assert np.array_equal(out[0], cur[0]) and np.array_equal(out[2], cur[2])
    assert list(k[1]) == [0.0, 0.0, 0.5, 0.5, 0.5, 1.0, 1.0]
    assert (out[1, :2] == h(0.75)).all() and (out[1, 5:] == h(0.375)).all()          # woven; the mean of 0.25 and 0.5
    assert (out[1, 2:5] == h(0.75 + 0.5 * (0.375 - 0.75))).all()
    assert copied[1, :2].all() and not copied[1, 2:].any()


# ---------------------------------------------------------------- the condition on the test pictures

def test_every_class_of_the_weight_holds_a_fifth_of_every_test_picture():
    """Random frames are "moving" everywhere: a test on them would only re-test cvs_field_to_frame.  The pictures the GPU tests
    and the catalogue use are built in thirds (dm.thirds), and by the model alone each of the classes k == 0, 0 < k < 1 and k == 1
    holds at least 20 % of the made pixels of every picture 12 or more columns wide -- with every frame's window whole; the tests
    that cut a neighbour's window do so on such a picture."""
    import oracle
    oracle.lib()
    from tests import deinterlace_cases as dc
    from tests.test_deinterlace_gpu import HEIGHTS, WIDTHS, _pictures
    assert (THRESHOLD, SOFTNESS) == (dc.THRESHOLD, dc.SOFTNESS)
    checked, smallest = 0, 1.0

    def hold(frames, what):
        nonlocal checked, smallest
        prev, cur, nxt = frames
        for field in (0, 1):
            k = dm.adaptive(cur, prev, nxt, field, THRESHOLD, SOFTNESS, oracle.float_to_half)[1]
            if np.isnan(k).all():
                continue                                                 # one row, kept
            shares = dm.classes(k)
            assert min(shares) >= 0.2, (what, field, shares)
            smallest = min(smallest, min(shares))
            checked += 1

    for width, pairs in WIDTHS:                                          # tests/test_deinterlace_gpu.py test_whole_frames
        if width < 12:
            continue
        pad = (width & 1) if pairs else 1 - (width & 1)
        for height in HEIGHTS:
            for n, (x0, y0) in enumerate([(0, 0), (1, -1), (1, 0), (0, -1)]):
                cw = (x0, y0, x0 + width - 1, y0 + height - 1)
                hold(_pictures(width * 131 + height * 7 + n, cw, pad), (width, height, x0, y0))
    for seed, cw in ((77, (2, -3, 131, 17)), (78, (1, 0, 141, 25)), (79, (0, -1, 129, 17)), (81, (0, 0, 719, 479)), (90, (-2, -1, 140, 35)),
                     (80 + 129, (0, 0, 128, 16)), (80 + 62, (0, 0, 61, 16)), (82, (0, 0, 131072, 2))):
        hold(_pictures(seed, cw), cw)
    for w in dc.WIDTHS + [12]:                                           # tests/deinterlace_cases.py
        for h in dc.HEIGHTS:
            full = (0, 0, w - 1, h - 1)
            hold([(codes, full, full) for codes in dm.thirds(np.random.default_rng(1300 + w + h), full, THRESHOLD, SOFTNESS)], (w, h))
    assert checked >= 500 and smallest >= 0.2


# ---------------------------------------------------------------- refusals of the entry

def test_entry_refuses_before_anything_is_launched(lib):
    from canvas_amd import _lib
    from canvas_amd.abi import HostFrame
    full = (0, 0, 7, 7)
    lim = _lib.MAX_COORD
    nan, inf = float("nan"), float("inf")
    entry = getattr(lib, ENTRY)
    box = _lib.box2i.of
    fresh = lambda: HostFrame(full, np.uint16, current_window=full)
    prev, cur, nxt, ok = fresh(), fresh(), fresh(), _lib.deinterlace_adaptive()

    def refused(out, a, b, c, p, word):
        lib.cvs_clear_last_error()
        assert entry(out, a, b, c, p, None) == -1, word
        assert ENTRY in _lib.last_error() and word in _lib.last_error(), (word, _lib.last_error())

    cases = [(None, "need")] + [(_lib.deinterlace_adaptive(f), "field") for f in (2, -1, 7)]
    cases += [(_lib.deinterlace_adaptive(flags=f), "unknown flags") for f in (1, 2, -1, 0x100)]
    cases += [(_lib.deinterlace_adaptive(0, t, 0.1), "threshold") for t in (nan, inf, -inf)]
    cases += [(_lib.deinterlace_adaptive(0, 0.05, s), "softness") for s in (nan, inf, -inf, -1e-30, -1.0)]
    for p, word in cases:
        out = fresh()
        refused(out.ref(), prev.ref(), cur.ref(), nxt.ref(), None if p is None else C.byref(p), word)
        assert out.current_window.is_empty(), word
    out = fresh()
    refused(out.ref(), prev.ref(), None, nxt.ref(), C.byref(ok), "need")
    assert out.current_window.is_empty()
    refused(None, prev.ref(), cur.ref(), nxt.ref(), C.byref(ok), "need")
    frame = lambda data, fullw=full, curw=full: _lib.rgba_frame_f16(data, box(*fullw), box(*curw))
    for k in range(3):
        out = fresh()
        ops = [prev.ref(), cur.ref(), nxt.ref()]
        ops[k] = C.byref(frame(out.c.data))                              # another frame over the output's buffer
        refused(out.ref(), ops[0], ops[1], ops[2], C.byref(ok), "cannot be one of the inputs")
        assert out.current_window.is_empty()
        ops[k] = C.byref(frame((prev, cur, nxt)[k].c.data, full, (0, 0, 8, 7)))
        refused(out.ref(), ops[0], ops[1], ops[2], C.byref(ok), "outside its buffer")
        for fullw, curw in (((lim - 6, 0, lim + 1, 7), (lim - 6, 0, lim, 7)), ((0, -lim - 1, 7, -lim + 6), (0, -lim, 7, -lim + 6)),
                            ((0, 0, 2 ** 31 - 1, 7), full), ((-2 ** 31, 0, 7, 7), full)):
            out = fresh()
            ops[k] = C.byref(frame((prev, cur, nxt)[k].c.data, fullw, curw))
            refused(out.ref(), ops[0], ops[1], ops[2], C.byref(ok), "beyond")
            assert out.current_window.is_empty()
    far = frame(fresh().c.data, (lim - 6, 0, lim + 1, 7))
    refused(C.byref(far), prev.ref(), cur.ref(), nxt.ref(), C.byref(ok), "beyond")
    assert far.current_window.is_empty() and cur.current_window.tuple() == full           # a refused call leaves its inputs alone
    both = fresh()
    refused(both.ref(), None, both.ref(), None, C.byref(ok), "cannot be one of the inputs")
    # a negative threshold, a zero softness and absent neighbours are legal; an empty cur is no error and launches nothing
    nothing = HostFrame(full, np.uint16, current_window=(0, 0, -1, -1))
    out = fresh()
    assert entry(out.ref(), prev.ref(), nothing.ref(), None, C.byref(_lib.deinterlace_adaptive(1, -1.0, 0.0)), None) in (0, -1)
    if lib.cvs_device_count() == 0:
        # without a device a call that nothing refuses still fails, loudly, and computes nothing on the CPU
        for a, c in ((prev, nxt), (None, None)):
            lib.cvs_clear_last_error()
            out = fresh()
            assert entry(out.ref(), a.ref() if a else None, cur.ref(), c.ref() if c else None, C.byref(_lib.deinterlace_adaptive(1, -1.0, 0.0)), None) != 0
            assert "no CPU path" in _lib.last_error(), _lib.last_error()
            assert out.current_window.is_empty()


# ---------------------------------------------------------------- the catalogue

def test_the_device_entry_of_the_header_has_its_catalogue_cases():
    """What tests/test_entry_cases_cpu.py holds tests/entry_cases.py to, for tests/deinterlace_cases.py: the entry the header
    declares is CALLED by every case, once, and handed the factory's stream; every case has an output and asks for the same
    operands every time; the Shifted factory moves every frame and changes no buffer, so the far-window harness runs the cases as
    it runs the catalogue's; the first case hands in every operand."""
    from tests import deinterlace_cases as dc
    from tests import entry_cases as ec
    from tests.test_entry_cases_cpu import Geometry, HostOnly, Recorder, _check_shifted
    _funcs, entries = _declared(HEADER)
    assert entries == sorted(dc.ENTRIES)
    seen, stream, operands = [], 0x5EED, []
    for gid, build in dc.GROUPS:
        rec = Recorder()
        for what, case in build(rec):
            before = len(rec.calls)
            fac = HostOnly(rec, stream)
            assert case(fac) == 0
            made = rec.calls[before:]
            assert made == [(ENTRY, stream)], (gid, what, made)
            seen.append(what)
            operands.append(len(fac.objects))
            assert sum(o.out for o in fac.objects) == 1 and fac.objects[-1].out and all(o.frame is not None for o in fac.objects), (gid, what)
            again = HostOnly(rec, stream)
            case(again)
            spec = lambda f: [(o.cls, o.name, o.out, o.cmp, o.nbytes, o.row_bytes, o.reads) for o in f.objects]
            assert spec(fac) == spec(again), (gid, what)
            boxes = [(o.out, o.frame.c.full_window.tuple()) for o in fac.objects]
            assert len(ec.far_offsets(dc.FAR_RULE, boxes)) >= 4, (gid, what)
    assert len(seen) == len(set(seen)) == 36 and operands[0] == 4 and sorted(set(operands)) == [2, 3, 4]
    for w in dc.WIDTHS:
        for h in dc.HEIGHTS:
            for field in (0, 1):
                for word in ("both", "none", "prev" if field == 0 else "next"):
                    assert "adaptive %dx%d field %d neighbours %s" % (w, h, field, word) in seen
    assert dc.FAR_RULE is ec._EVEN
    frames = 0
    for gid, build in dc.GROUPS:
        a, b = Geometry(), Geometry()
        for (what, near), (_, far) in zip(build(a), build(b)):
            frames += _check_shifted(gid, what, (near, far, a, b), dc.FAR_RULE["source_scale"])
    assert frames == sum(operands)


# ---------------------------------------------------------------- the nodes, as far as they go without a device

def test_the_nodes_are_in_the_module_and_fail_soft_without_a_device():
    from fluggo.media import basetypes as bt
    from fluggo.media import process
    window = bt.box2i(0, 0, 7, 7)
    solid = process.SolidColorVideoSource((0.25, 0.5, 0.75, 1.0), bt.box2i(0, 0, 9, 9))
    for T, arg in ((process.AdaptiveDeinterlaceFilter, "field"), (process.AdaptiveBobDeinterlaceFilter, "first_field")):
        assert issubclass(T, process.VideoSource)
        node = T(None)
        assert (getattr(node, arg), node.threshold, node.softness, node.source) == (0, 0.02, 0.04, None)
        assert type(node._video_frame_source_funcs).__name__ == "PyCapsule"
        # an absent source gives an empty window and never an exception, with or without a device
        assert node.get_frame_f16(0, window).current_window.empty() and node.get_frame_f32(-3, window).current_window.empty()
        node = T(solid, 1, threshold=0.5, softness=process.LinearFrameFunc(0.0, 0.25))
        assert (getattr(node, arg), node.threshold, node.source) == (1, 0.5, solid) and isinstance(node.softness, process.LinearFrameFunc)
        node.set_source(None)
        assert node.source is None
        node.source = solid
        assert node.source is solid
        for bad in (2, -1):
            with pytest.raises(ValueError):
                T(solid, bad)
        with pytest.raises(Exception):
            T(solid, threshold="x")
        with pytest.raises(Exception):
            T(object())
        with pytest.raises((AttributeError, TypeError)):
            setattr(node, arg, 0)                                        # read-only, as the field nodes'
        from canvas_amd import _lib
        if _lib.load().cvs_device_count() == 0:
            assert node.get_frame_f16(1, window).current_window.empty()     # no device: empty, no exception
