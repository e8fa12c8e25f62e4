"""The median without a GPU (DESIGN.md "Median"): the order on bit patterns; the numpy model (tests/median_model.py) against a
per-pixel loop; the condition on the test picture that keeps the threshold's two classes populated; the two selection networks
of kernels/median_net.hpp proven on every input of zeros and ones; include/canvas_median.h against the library and its
bindings; every refusal of the entries, which comes before the device is touched; the catalogue of tests/median_cases.py; the
node's attributes; the built code object."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from tests import median_model as mm
from tests.test_perspective_cpu import _declared
from tests.test_unsharp_cpu import _kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "canvas_median.h"
ENTRIES = ["cvs_median_f16_dev", "cvs_median_f32_dev"]
FIELDS = ["radius", "threshold", "channels", "flags"]


@pytest.fixture(scope="module")
def lib():
    from canvas_amd import _lib
    return _lib.load()


# ---------------------------------------------------------------- the order

def test_key_is_a_bijection_in_the_order_of_the_values():
    codes = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    keys = mm.key(codes)
    assert len(np.unique(keys)) == 65536 and np.array_equal(mm.unkey(keys), codes)
    assert np.array_equal(keys, np.array([(~h & 0xFFFF) if h & 0x8000 else h | 0x8000 for h in range(65536)], np.uint16))
    values = codes.view(np.float16).astype(np.float64)
    finite = np.isfinite(values)
    order = np.argsort(keys[finite], kind="stable")
    assert (np.diff(values[finite][order]) >= 0).all()                  # monotone on the finite values
    assert mm.key(np.uint16(0x8000)) < mm.key(np.uint16(0x0000))        # -0 < +0
    by_key = codes[np.argsort(keys)]
    assert by_key[0] == 0xFFFF and by_key[-1] == 0x7FFF                 # -NaN .. +NaN
    assert mm.key(np.uint16(0xFC01)) < mm.key(np.uint16(0xFC00)) < mm.key(np.uint16(0xFBFF)) and mm.key(np.uint16(0x7BFF)) < mm.key(np.uint16(0x7C00)) < mm.key(np.uint16(0x7C01))
    rng = np.random.default_rng(5)
    wide = np.concatenate([rng.integers(0, 2 ** 32, 100000).astype(np.uint32), mm.SPECIALS32])
    assert np.array_equal(mm.unkey(mm.key(wide)), wide)
    with np.errstate(invalid="ignore"):
        v = wide.view(np.float32).astype(np.float64)
    ok = np.isfinite(v)
    assert (np.diff(v[ok][np.argsort(mm.key(wide)[ok], kind="stable")]) >= 0).all()
    assert mm.key(np.uint32(0x80000000)) < mm.key(np.uint32(0))


# ---------------------------------------------------------------- the model

@pytest.mark.parametrize("dtype", [np.uint16, np.uint32])
@pytest.mark.parametrize("radius", [1, 2])
def test_model_against_a_loop_over_pixels(dtype, radius):
    rng = np.random.default_rng(11 + radius)
    for w, h in ((9, 7), (1, 5), (4, 1), (2, 2)):
        pixels = mm.speck_picture(rng, w, h, dtype)
        for threshold, channels in ((0.0, "rgba"), (mm.THRESHOLD, "rgba"), (mm.THRESHOLD, "a"), (0.0, "ga"), (mm.THRESHOLD, "rgb")):
            got = mm.filter_pixels(pixels, radius, threshold, channels)
            assert np.array_equal(got, mm.brute(pixels, radius, threshold, channels)), (w, h, threshold, channels)
            unselected = [c for c in range(4) if not mm.mask_of(channels) >> c & 1]
            assert np.array_equal(got[..., unselected], pixels[..., unselected])


def test_model_windows_and_tiles():
    rng = np.random.default_rng(13)
    sfull, scur = (-2, -1, 40, 20), (0, 1, 37, 18)
    pixels = rng.integers(0, 0x3C01, (22, 43, 4)).astype(np.uint16)
    mm.crop(pixels, sfull, scur)[...] = mm.speck_picture(rng, 38, 18)
    before = np.full((30, 50, 4), 0x1234, np.uint16)
    tfull = (-5, -5, 44, 24)
    whole, win = mm.expected(before, tfull, pixels, sfull, scur, 2, mm.THRESHOLD)
    assert win == scur and (mm.crop(whole, tfull, (-5, -5, 44, 0)) == 0x1234).all()
    # junk outside the current window changes nothing
    other = rng.integers(0, 0xFFFF, pixels.shape).astype(np.uint16)
    mm.crop(other, sfull, scur)[...] = mm.crop(pixels, sfull, scur)
    assert np.array_equal(mm.expected(before, tfull, other, sfull, scur, 2, mm.THRESHOLD)[0], whole)
    # a tile from the source grown by the radius equals the same tile of the whole
    tile = (10, 5, 20, 9)
    grown = (8, 3, 22, 11)
    part = mm.filter_pixels(mm.crop(pixels, sfull, grown), 2, mm.THRESHOLD)
    assert np.array_equal(mm.crop(part, grown, tile), mm.crop(whole, tfull, tile))
    assert mm.expected(before, tfull, pixels, sfull, None, 1)[1] is None and mm.expected(before, (50, 0, 60, 5), pixels, sfull, scur, 1)[1] is None
    # every output code is an input code of its neighbourhood's channel; a flat picture and one of NaNs come back as they are
    flat = np.broadcast_to(np.array([0x3800, 0x8000, 0x0001, 0x7BFF], np.uint16), (6, 7, 4)).copy()
    nans = np.full((6, 7, 4), 0x7E00, np.uint16)
    for same in (flat, nans):
        for threshold in (0.0, mm.THRESHOLD):
            assert np.array_equal(mm.filter_pixels(same, 2, threshold), same)


def test_model_of_a_tiled_picture_is_the_model_of_the_picture():
    rng = np.random.default_rng(17)
    for period, height, radius, channels in ((37, 1000, 1, "a"), (41, 167, 2, "rgba"), (5, 23, 2, "ga")):
        tile = mm.speck_picture(rng, 3, period)
        whole = np.tile(tile, (-(-height // period), 1, 1))[:height]
        assert np.array_equal(mm.filter_tiled(tile, height, radius, mm.THRESHOLD, channels), mm.filter_pixels(whole, radius, mm.THRESHOLD, channels))


def test_both_classes_hold_a_twentieth_of_every_test_picture():
    """With the threshold of the tests, kept and replaced pixels each make up at least 5 % of every picture of 200 pixels or more
    that the GPU tests and the catalogue use: neither branch of the per-pixel decision goes untested."""
    for dtype in (np.uint16, np.uint32):
        for w, h in ((31, 7), (33, 9), (65, 7), (130, 21), (130, 9), (124, 9), (60, 17), (62, 8), (249, 3)):
            for radius in (1, 2):
                for channels in ("rgba", "rgb", "a", "ga"):
                    pixels = mm.speck_picture(np.random.default_rng(2100 + w + h), w, h, dtype)
                    kept, taken = mm.classes(pixels, radius, mm.THRESHOLD, channels)
                    assert kept >= 0.05 and taken >= 0.05, (dtype, w, h, radius, channels, kept, taken)


# ---------------------------------------------------------------- the networks

def _network(name):
    text = open(os.path.join(ROOT, "canvas_amd", "csrc", "kernels", "median_net.hpp")).read()
    body = re.search(r"#define %s\(CE\)((?:.*\\\n)*.*)\n" % name, text).group(1)
    return [(int(a), int(b)) for a, b in re.findall(r"CE\((\d+),\s*(\d+)\)", body)]


def _selects_the_median(net, n):
    """The 0-1 principle: a network of compare-exchanges that leaves the majority bit in the middle on every one of the 2^n
    inputs of zeros and ones leaves the median there on every input.  All inputs at once, one bit each, 64 to a word."""
    words = max(1, (1 << n) >> 6)
    index = np.arange(words, dtype=np.uint64)
    ones = np.uint64(0xFFFFFFFFFFFFFFFF)
    v = []
    for i in range(n):
        if i < 6:
            v.append(np.full(words, sum(1 << j for j in range(64) if j >> i & 1), np.uint64))
        else:
            v.append(np.where((index >> np.uint64(i - 6)) & np.uint64(1) == 1, ones, np.uint64(0)))
    count = [np.zeros(words, np.uint64) for _ in range(5)]               # the number of ones of every input, bit-sliced
    for x in v:
        carry = x
        for k in range(5):
            count[k], carry = count[k] ^ carry, count[k] & carry
    add, carry = 32 - (n + 1) // 2, np.zeros(words, np.uint64)           # count >= (n + 1) / 2: the carry out of count + add
    for k in range(5):
        a = ones if add >> k & 1 else np.uint64(0)
        carry = (count[k] & a) | (count[k] & carry) | (a & carry)
    for a, b in net:
        v[a], v[b] = v[a] & v[b], v[a] | v[b]
    return bool((v[n // 2] == carry).all())


def test_the_selection_networks_select_the_median():
    n9, n25 = _network("MEDIAN_NET_9"), _network("MEDIAN_NET_25")
    assert len(n9) == 19 and len(n25) == 99
    assert all(0 <= a < 9 and 0 <= b < 9 and a != b for a, b in n9) and all(0 <= a < 25 and 0 <= b < 25 and a != b for a, b in n25)
    assert _selects_the_median(n9, 9) and _selects_the_median(n25, 25)
    # the proof has teeth: with any one exchange left out of the small network it fails
    assert not any(_selects_the_median(n9[:k] + n9[k + 1:], 9) for k in range(19))
    assert not _selects_the_median(n25[:-1], 25)


# ---------------------------------------------------------------- the header, the library, the bindings

def test_struct_mirror_has_the_c_layout():
    from canvas_amd import _lib
    assert [name for name, _ in _lib.median_params._fields_] == FIELDS
    probe = ('#include <stddef.h>\n#include <stdio.h>\n#include "%s"\nint main(void) {\n    printf("%%zu", sizeof(cvs_median));\n' % HEADER
             + "".join('    printf(" %%zu", offsetof(cvs_median, %s));\n' % f for f in FIELDS)
             + '    printf(" %d %d %d %d %d %d\\n", CVS_MEDIAN_R, CVS_MEDIAN_G, CVS_MEDIAN_B, CVS_MEDIAN_A, CVS_MEDIAN_COLOUR, CVS_MEDIAN_ALL);\n    return 0;\n}\n')
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "probe.c")
        with open(src, "w") as f:
            f.write(probe)
        for cc, std, lang in (("gcc", "-std=c99", "c"), ("g++", "-std=c++14", "c++")):
            exe = os.path.join(tmp, "probe_" + cc)
            subprocess.run([cc, std, "-Wall", "-Werror", "-x", lang, src, "-I", os.path.join(ROOT, "include"), "-o", exe], check=True)
            got = [int(v) for v in subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout.split()]
            assert got[:5] == [C.sizeof(_lib.median_params)] + [getattr(_lib.median_params, f).offset for f in FIELDS] and got[0] == 16
            assert got[5:] == [_lib.MEDIAN_R, _lib.MEDIAN_G, _lib.MEDIAN_B, _lib.MEDIAN_A, _lib.MEDIAN_COLOUR, _lib.MEDIAN_ALL] == [1, 2, 4, 8, 7, 15]
    p = _lib.median()
    assert (p.radius, p.threshold, p.channels, p.flags) == (1, 0.0, 15, 0)
    p = _lib.median(2, 0.0625, _lib.MEDIAN_A)
    assert (p.radius, p.threshold, p.channels, p.flags) == (2, 0.0625, 8, 0)
    F16, F32 = C.POINTER(_lib.rgba_frame_f16), C.POINTER(_lib.rgba_frame_f32)
    assert _lib.MEDIAN_SIGNATURES == {ENTRIES[0]: (C.c_int, [F16, F16, C.POINTER(_lib.median_params), C.c_void_p]),
                                      ENTRIES[1]: (C.c_int, [F32, F32, C.POINTER(_lib.median_params), C.c_void_p])}


def test_every_symbol_of_the_header_is_exported_and_bound(lib):
    from canvas_amd import _lib
    funcs, entries = _declared(HEADER)
    assert funcs == sorted(_lib.MEDIAN_SIGNATURES) == ENTRIES and entries == ENTRIES
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert set(ENTRIES) <= {line.split()[-1] for line in out.splitlines() if line.strip()}
    others = set(_lib.SIGNATURES) | set(_lib.SCOPE_SIGNATURES) | set(_lib.LUT3D_SIGNATURES) | set(_lib.PERSPECTIVE_SIGNATURES) | set(_lib.DEINTERLACE_SIGNATURES)
    assert not set(_lib.MEDIAN_SIGNATURES) & others
    for name in ENTRIES:
        assert getattr(lib, name).argtypes == _lib.MEDIAN_SIGNATURES[name][1] and getattr(lib, name).restype is C.c_int
    # the header says where the sharing policy is stated, and canvas_hip.h does not declare the entries
    assert "Operands that share a buffer" in open(os.path.join(ROOT, "include", HEADER)).read()
    assert "cvs_median" not in open(os.path.join(ROOT, "include", "canvas_hip.h")).read()
    # one launcher, one arithmetic flavour
    symbols = subprocess.run(["nm", _lib.LIB_PATH], stdout=subprocess.PIPE, text=True).stdout
    assert re.search(r"\bcvk_median\b", symbols) and not re.search(r"\bcvk_median_fma\b", symbols)


def test_code_object_holds_the_six_instances_without_scratch():
    """One build for both arithmetic flavours; f32, f16 one pixel and f16 two pixels per lane x radius 1 and 2; no private
    segment, no spills: every value of the networks stays in a register."""
    assert os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"), "the ROCm LLVM tools the build itself needs are missing"
    found = _kernels("median_ops.hip.o")
    assert len(found) == 6 and all("k_median" in n for n in found), sorted(found)
    for fmt in (0, 1, 2):
        for radius in (1, 2):
            assert any("k_medianILi%dELi%dEEE" % (fmt, radius) in n for n in found), (fmt, radius, sorted(found))
    for name, (scratch, spills) in found.items():
        assert scratch == 0 and spills == 0, (name, scratch, spills)
    assert not os.path.exists(os.path.join(ROOT, "canvas_amd", "csrc", "build", "median_ops.fma.hip.o"))


# ---------------------------------------------------------------- refusals of the entries

@pytest.mark.parametrize("half", [True, False], ids=["f16", "f32"])
def test_entries_refuse_before_anything_is_launched(lib, half):
    from canvas_amd import _lib
    from canvas_amd.abi import HostFrame
    name = ENTRIES[0 if half else 1]
    entry = getattr(lib, name)
    dtype, struct = (np.uint16, _lib.rgba_frame_f16) if half else (np.float32, _lib.rgba_frame_f32)
    full = (0, 0, 7, 7)
    lim = _lib.MAX_COORD
    nan, inf = float("nan"), float("inf")
    box = _lib.box2i.of
    fresh = lambda: HostFrame(full, dtype, current_window=full)
    src, ok = fresh(), _lib.median()

    def refused(out, s, p, word):
        lib.cvs_clear_last_error()
        assert entry(out, s, p, None) == -1, word
        assert name in _lib.last_error() and word in _lib.last_error(), (word, _lib.last_error())

    cases = [(None, "need")] + [(_lib.median(r), "radius") for r in (0, 3, -1)]
    cases += [(_lib.median(1, 0.0, c), "channels") for c in (0, 16, 31, -1, 0x100)]
    cases += [(_lib.median(flags=f), "unknown flags") for f in (1, 2, -1, 0x100)]
    cases += [(_lib.median(1, t), "threshold") for t in (nan, inf, -inf, -1e-30, -1.0)]
    for p, word in cases:
        out = fresh()
        refused(out.ref(), src.ref(), None if p is None else C.byref(p), word)
        assert out.current_window.is_empty(), word
    out = fresh()
    refused(out.ref(), None, C.byref(ok), "need")
    assert out.current_window.is_empty()
    refused(None, src.ref(), C.byref(ok), "need")
    frame = lambda data, fullw=full, curw=full: struct(data, box(*fullw), box(*curw))
    out = fresh()
    refused(out.ref(), C.byref(frame(out.c.data)), C.byref(ok), "cannot be the source")       # another frame over the target's buffer
    assert out.current_window.is_empty()
    both = fresh()
    refused(both.ref(), both.ref(), C.byref(ok), "cannot be the source")                      # one struct as both
    out = fresh()
    refused(out.ref(), C.byref(frame(src.c.data, full, (0, 0, 8, 7))), C.byref(ok), "outside its buffer")
    for fullw, curw in (((lim - 6, 0, lim + 1, 7), (lim - 6, 0, lim, 7)), ((0, -lim - 1, 7, -lim + 6), (0, -lim, 7, -lim + 6)),
                        ((0, 0, 2 ** 31 - 1, 7), full), ((-2 ** 31, 0, 7, 7), full)):
        out = fresh()
        refused(out.ref(), C.byref(frame(src.c.data, fullw, curw)), C.byref(ok), "beyond")
        assert out.current_window.is_empty()
    far = frame(fresh().c.data, (lim - 6, 0, lim + 1, 7))
    refused(C.byref(far), src.ref(), C.byref(ok), "beyond")
    assert far.current_window.is_empty() and src.current_window.tuple() == full             # a refused call leaves its input alone
    # the refusals come in the contract's order: the first that applies is named
    out = fresh()
    refused(out.ref(), C.byref(frame(out.c.data, full, (0, 0, 8, 7))), C.byref(_lib.median(3, nan, 0, 1)), "radius")
    refused(out.ref(), C.byref(frame(out.c.data, full, (0, 0, 8, 7))), C.byref(_lib.median(2, nan, 0, 1)), "channels")
    refused(out.ref(), C.byref(frame(out.c.data, full, (0, 0, 8, 7))), C.byref(_lib.median(2, nan, 1, 1)), "unknown flags")
    refused(out.ref(), C.byref(frame(out.c.data, full, (0, 0, 8, 7))), C.byref(_lib.median(2, nan, 1)), "threshold")
    refused(out.ref(), C.byref(frame(out.c.data, full, (0, 0, 8, 7))), C.byref(ok), "cannot be the source")
    # an empty source is no error and launches nothing
    nothing = HostFrame(full, dtype, current_window=(0, 0, -1, -1))
    out = fresh()
    assert entry(out.ref(), nothing.ref(), C.byref(ok), None) in (0, -1) and out.current_window.is_empty()
    if lib.cvs_device_count() == 0:
        # without a device a call that nothing refuses still fails, loudly, and computes nothing on the CPU
        lib.cvs_clear_last_error()
        out = fresh()
        assert entry(out.ref(), src.ref(), C.byref(ok), None) != 0
        assert "no CPU path" in _lib.last_error(), _lib.last_error()
        assert out.current_window.is_empty()


# ---------------------------------------------------------------- the catalogue

def test_the_device_entries_of_the_header_have_their_catalogue_cases():
    """What tests/test_entry_cases_cpu.py holds tests/entry_cases.py to, for tests/median_cases.py: every entry the header
    declares is CALLED by a case; every case makes one call, handed the factory's stream, has one output and asks for the same
    operands every time; the Shifted factory moves every frame and changes no buffer, so the far-window harness runs the cases
    as it runs the catalogue's."""
    from tests import entry_cases as ec
    from tests import median_cases as mc
    from tests.test_entry_cases_cpu import Geometry, HostOnly, Recorder, _check_shifted
    _funcs, entries = _declared(HEADER)
    assert entries == sorted(mc.ENTRIES)
    seen, called, stream, operands = [], set(), 0x5EED, 0
    for gid, build in mc.GROUPS:
        rec = Recorder()
        for what, case in build(rec):
            before = len(rec.calls)
            fac = HostOnly(rec, stream)
            assert case(fac) == 0
            made = rec.calls[before:]
            assert len(made) == 1 and made[0][0] in ENTRIES and made[0][1] == stream, (gid, what, made)
            called.add(made[0][0])
            seen.append(what)
            operands += len(fac.objects)
            assert len(fac.objects) == 2 and not fac.objects[0].out and fac.objects[1].out and all(o.frame is not None for o in fac.objects), (gid, what)
            again = HostOnly(rec, stream)
            case(again)
            spec = lambda f: [(o.cls, o.name, o.out, o.cmp, o.nbytes, o.row_bytes, o.reads) for o in f.objects]
            assert spec(fac) == spec(again), (gid, what)
            boxes = [(o.out, o.frame.c.full_window.tuple()) for o in fac.objects]
            assert len(ec.far_offsets(mc.FAR_RULE, boxes)) >= 4, (gid, what)
    assert called == set(ENTRIES) and len(seen) == len(set(seen)) == 16
    for fmt in ("f16", "f32"):
        for radius in (1, 2):
            for word in ("threshold 0 ", "threshold 0.0625"):
                assert any(fmt in s and "radius %d" % radius in s and word in s for s in seen), (fmt, radius, word)
    assert mc.FAR_RULE is ec._ANY
    frames = 0
    for gid, build in mc.GROUPS:
        a, b = Geometry(), Geometry()
        for (what, near), (_, far) in zip(build(a), build(b)):
            frames += _check_shifted(gid, what, (near, far, a, b), mc.FAR_RULE["source_scale"])
    assert frames == operands


# ---------------------------------------------------------------- the node, as far as it goes without a device

def test_the_node_is_in_the_module_and_fails_soft_without_a_device():
    from fluggo.media import basetypes as bt
    from fluggo.media import process
    window = bt.box2i(0, 0, 7, 7)
    solid = process.SolidColorVideoSource((0.25, 0.5, 0.75, 1.0), bt.box2i(0, 0, 9, 9))
    T = process.VideoMedianFilter
    assert issubclass(T, process.VideoSource)
    node = T(None)
    assert (node.radius, node.threshold, node.channels, node.source) == (1, 0.0, "rgba", None)
    assert type(node._video_frame_source_funcs).__name__ == "PyCapsule"
    # an absent source gives an empty window and never an exception, with or without a device
    assert node.get_frame_f16(0, window).current_window.empty() and node.get_frame_f32(-3, window).current_window.empty()
    node = T(solid, 2, threshold=process.LinearFrameFunc(0.0, 0.25), channels="ag")
    assert (node.radius, node.channels, node.source) == (2, "ga", solid) and isinstance(node.threshold, process.LinearFrameFunc)
    node = T(solid, radius=2, threshold=0.5, channels="bgr")
    assert (node.radius, node.threshold, node.channels) == (2, 0.5, "rgb")
    node.set_source(None)
    assert node.source is None
    node.source = solid
    assert node.source is solid
    # a refused value raises and keeps the old one
    for attr, bad, error in (("radius", 0, ValueError), ("radius", 3, ValueError), ("radius", 1.0, TypeError), ("radius", None, TypeError), ("radius", True, TypeError),
                             ("channels", "", ValueError), ("channels", "rr", ValueError), ("channels", "rgbx", ValueError), ("channels", "RGB", ValueError),
                             ("channels", 15, TypeError), ("channels", None, TypeError), ("threshold", None, TypeError), ("threshold", "x", Exception)):
        with pytest.raises(error):
            setattr(node, attr, bad)
        assert (node.radius, node.threshold, node.channels) == (2, 0.5, "rgb"), (attr, bad)
    node.radius, node.threshold, node.channels = 1, 0.125, "a"
    assert (node.radius, node.threshold, node.channels) == (1, 0.125, "a")
    for kw in ({"radius": 3}, {"radius": "1"}, {"channels": "q"}, {"channels": ""}, {"threshold": "x"}, {"threshold": None}):
        with pytest.raises(Exception):
            T(solid, **kw)
    with pytest.raises(Exception):
        T(object())
    from canvas_amd import _lib
    if _lib.load().cvs_device_count() == 0:
        assert node.get_frame_f16(1, window).current_window.empty()     # no device: empty, no exception
