"""The primary colour corrector without a GPU (DESIGN.md "Primary colour correction"): the numpy model (tests/primary_model.py)
against a per-pixel loop; the two exactness properties the header states; the conditions on the test picture that keep every class
of sample populated; include/canvas_primary.h against the library and its bindings; cvs_curves_bytes and cvs_curves_pack; every
refusal of the entries in the header's order, which comes before the device is touched; the catalogue of tests/primary_cases.py;
ColorCurves' and the node's attributes and refusals; the built code object."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from tests import primary_model as pm
from tests.models import f2h_rz_model
from tests.test_perspective_cpu import _declared
from tests.test_unsharp_cpu import _kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "canvas_primary.h"
ENTRIES = ["cvs_primary_f16_dev", "cvs_primary_f32_dev"]
F32 = np.float32
ONE = 0x3C00                                     # the half code of 1.0: codes 0 .. ONE are the halfs in [0, 1]
POW2_SIZES = [2 ** k + 1 for k in range(13)]     # K - 1 = 1, 2, 4, ..., 4096
MATRIX = [0.75, 0.5, -0.25, 0.0625, 0.0, -1.0, 2.0, 0.0, 0.3, 0.3, 0.3, -0.2]
# every (size, domain) of a first stage that the GPU tests and the catalogue put a test picture through, and the pictures' sizes
GPU_SIZES = [2, 3, 17, 1024, 1025, 4097]
GPU_PICTURES = [(131, 9), (131073, 3), (1, 4099)]
# the pictures of tests/test_primary_node_gpu.py (46 x 31, its RASTER) and of test_primary_gpu.py's overflowing matrix, which are on
# domains and sizes of their own: (size, domain, width, height, formats)
SHAPER_DOMAIN = ((-0.125, -0.125, -0.125), (1.5, 1.5, 1.5))
OVERFLOW_DOMAIN = ((-4.0, -4.0, -4.0), (4.0, 4.0, 4.0))
OTHER_PICTURES = [(1025, pm.SKEWED, 46, 31, (True,)), (17, pm.WIDE, 46, 31, (True,)), (5, pm.UNIT, 46, 31, (True,)), (4097, SHAPER_DOMAIN, 46, 31, (True,)),
                  (2, OVERFLOW_DOMAIN, 131, 9, (True, False))]


@pytest.fixture(scope="module")
def process():
    from fluggo.media import process
    return process


@pytest.fixture(scope="module")
def lib():
    from canvas_amd import _lib
    return _lib.load()


# ---------------------------------------------------------------- the model

def test_the_model_is_the_contract_pixel_by_pixel():
    rng = np.random.default_rng(3)
    pre, post = pm.distinct(5, pm.SKEWED, 1), pm.distinct(1024, pm.WIDE, 2)
    for half in (True, False):
        pixels = pm.picture(rng, 23, 5, half, 5, pm.SKEWED)
        s = pm.widen(pixels) if half else pixels
        for a, m, b in ((pre, None, None), (None, MATRIX, None), (None, None, post), (pre, MATRIX, None), (pre, None, post), (None, MATRIX, post), (pre, MATRIX, post)):
            got, want = pm.apply_f32(s, a, m, b), pm.brute(s, a, m, b)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (half, a is not None, m is not None, b is not None)
            assert np.array_equal(got[..., 3].view(np.uint32), s[..., 3].view(np.uint32))
        out = pm.apply_pixels(pixels, pre, MATRIX, post)
        assert out.dtype == pixels.dtype and np.ascontiguousarray(out[..., 3]).tobytes() == np.ascontiguousarray(pixels[..., 3]).tobytes()


def test_the_matrix_reads_the_three_values_before_the_stage():
    s = np.array([[[0.25, 0.5, 0.75, 1.0]]], F32)
    swap = [0, 1, 0, 0, 0, 0, 1, 0, 1, 0, 0, 0]
    assert pm.apply_f32(s, matrix=swap)[0, 0].tolist() == [0.5, 0.75, 0.25, 1.0]


def test_clamp_nan_and_inf():
    cv = pm.distinct(5, pm.SKEWED)
    s = np.array([[np.nan, -np.inf, np.inf], [-1e30, 1e30, np.nan], [-0.25, 1.5, 0.1]], F32)
    out = pm.curve(cv, s)
    assert out[0].tolist() == [cv.table[0, 0], cv.table[0, 1], cv.table[4, 2]]
    assert out[1].tolist() == [cv.table[0, 0], cv.table[4, 1], cv.table[0, 2]]
    assert out[2, 0] == cv.table[0, 0] and out[2, 1] == cv.table[4, 1]


def test_expected_windows():
    rng = np.random.default_rng(4)
    sfull, scur, tfull = (-2, -1, 20, 9), (0, 0, 18, 8), (5, -3, 30, 4)
    pixels = pm.picture(rng, 23, 11, True, 3, pm.UNIT)
    before = np.full((8, 26, 4), 0x1234, np.uint16)
    cv = pm.distinct(3)
    out, win = pm.expected(before, tfull, pixels, sfull, scur, cv)
    assert win == (5, 0, 18, 4)
    assert np.array_equal(pm.crop(out, tfull, win), pm.apply_pixels(pm.crop(pixels, sfull, win), cv)) and (pm.crop(out, tfull, (19, -3, 30, 4)) == 0x1234).all()
    assert pm.expected(before, tfull, pixels, sfull, None, cv)[1] is None and pm.expected(before, (40, 0, 50, 5), pixels, sfull, scur, cv)[1] is None


# ---------------------------------------------------------------- the two properties the header states

@pytest.mark.parametrize("size", POW2_SIZES + [1024])
def test_an_input_on_a_node_returns_the_node(size):
    """On the unit domain with K - 1 = 1, 2, 4, ..., 4096, every node of a table that is no identity; and on the first and last
    node whatever K (1024): t is exact, so the result is the node's value, the last node through f = 1 (a*0 + b)."""
    cv = pm.distinct(size, pm.UNIT, 9)
    if (size - 1) & (size - 2) == 0:
        at = (np.arange(size, dtype=np.float64) / (size - 1)).astype(F32)
        s = np.stack([at, at, at], axis=-1)
        assert np.array_equal(pm.curve(cv, s), cv.table)
    ends = np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]], F32)
    assert np.array_equal(pm.curve(cv, ends), cv.table[[0, -1]])
    i, f, _ = pm.position(ends, size, pm.UNIT)
    assert (i[1] == size - 2).all() and (f[1] == 1).all() and (i[0] == 0).all() and (f[0] == 0).all()


@pytest.mark.parametrize("size", POW2_SIZES)
def test_identity_curves_are_the_identity_on_every_half_code_in_0_1(size):
    codes = np.arange(ONE + 1, dtype=np.uint16)
    pixels = np.stack([codes, codes[::-1], codes, codes], axis=-1)[None]
    cv = pm.identity(size)
    assert np.array_equal(pm.apply_pixels(pixels, cv), pixels)
    assert np.array_equal(pm.apply_pixels(pixels, cv, None, cv), pixels)
    s = pm.widen(pixels)
    assert np.array_equal(pm.apply_f32(s, cv).view(np.uint32), s.view(np.uint32))


@pytest.mark.parametrize("size", [256, 1024, 4096])
def test_identity_is_not_promised_for_other_sizes(size):
    """The claim of the header has teeth: with K - 1 no power of two some half code in [0, 1], widened, comes back as another
    f32; at K = 1024 some come back as another half after the truncation too (at 256 and 4096 the truncation happens to hide it)."""
    codes = np.arange(ONE + 1, dtype=np.uint16)
    pixels = np.stack([codes, codes, codes, codes], axis=-1)[None]
    s = pm.widen(pixels)
    assert not np.array_equal(pm.apply_f32(s, pm.identity(size)).view(np.uint32), s.view(np.uint32))
    assert np.array_equal(pm.apply_pixels(pixels, pm.identity(size)), pixels) == (size != 1024)


def test_the_other_form_loses_the_last_node():
    """a + f*(b-a), the form the header rejects: at f = 1 it returns a + (b - a), which is not b for every pair of floats."""
    rng = np.random.default_rng(8)
    a, b = rng.uniform(-0.5, 1.5, 4096).astype(F32), rng.uniform(-0.5, 1.5, 4096).astype(F32)
    assert ((a + (b - a).astype(F32)).astype(F32) != b).any()
    assert np.array_equal(((a * F32(0)).astype(F32) + (b * F32(1)).astype(F32)).astype(F32), b)


# ---------------------------------------------------------------- the test picture

@pytest.mark.parametrize("size", GPU_SIZES)
def test_every_class_of_sample_is_in_every_test_picture(size):
    """For every K the GPU tests use, on both domain sets and in both formats: at least half of the colour samples fall strictly
    inside a cell, at least 2 % are clamped at each end, at least 1 % sit on a node; and the special codes are there, in colour
    and in alpha."""
    for domain in (pm.SKEWED, pm.WIDE):
        for half in (True, False):
            for n, (w, h) in enumerate(GPU_PICTURES):
                if w > 1000 and size != 1025 or h > 1000 and size != 4097:
                    continue
                pixels = pm.picture(np.random.default_rng(size + n), w, h, half, size, domain)
                within, below, above, node = pm.classes(pixels, size, domain)
                assert within >= 0.5 and below >= 0.02 and above >= 0.02 and node >= 0.01, (size, domain, half, w, h, within, below, above, node)
                if w * h >= 40:
                    specials = pm.SPECIALS16 if half else pm.SPECIALS32
                    raw = pixels if half else pixels.view(np.uint32)
                    for code in specials:
                        assert (raw[..., :3] == code).any() and (raw[..., 3] == code).any(), (size, half, hex(int(code)))


def _check_classes(pixels, size, domain, what):
    within, below, above, node = pm.classes(pixels, size, domain)
    assert within >= 0.5 and below >= 0.02 and above >= 0.02 and node >= 0.01, (what, within, below, above, node)


@pytest.mark.parametrize("size,domain,w,h,formats", OTHER_PICTURES)
def test_the_node_tests_and_the_overflow_tests_pictures_too(size, domain, w, h, formats):
    """The same conditions for the pictures that are made for other sizes and domains than the table above: every seed the GPU
    tests draw them with."""
    from tests import test_primary_gpu, test_primary_node_gpu
    assert test_primary_node_gpu.RASTER == (0, -2, 45, 28) and SHAPER_DOMAIN == test_primary_node_gpu.SHAPER_DOMAIN and OVERFLOW_DOMAIN == test_primary_gpu.OVERFLOW_DOMAIN
    for half in formats:
        if (w, h) == (46, 31):
            for seed in (0, 3, 5, 11):
                for index in range(5):
                    _check_classes(pm.picture(np.random.default_rng([seed, index + 1000]), w, h, half, size, domain), size, domain, (size, seed, index))
        else:
            _check_classes(pm.picture(np.random.default_rng(77), w, h, half, size, domain), size, domain, (size, half))


# ---------------------------------------------------------------- the header, the library, the bindings

def test_struct_mirror_has_the_c_layout():
    from canvas_amd import _lib
    assert [name for name, _ in _lib.curves_params._fields_] == ["size", "domain_min", "domain_max"]
    assert [name for name, _ in _lib.primary_params._fields_] == ["pre", "matrix", "post", "flags"]
    probe = ('#include <stddef.h>\n#include <stdio.h>\n#include "%s"\nint main(void) {\n' % HEADER
             + '    printf("%zu %zu %zu %zu", sizeof(cvs_curves), offsetof(cvs_curves, size), offsetof(cvs_curves, domain_min), offsetof(cvs_curves, domain_max));\n'
             + '    printf(" %zu %zu %zu %zu %zu", sizeof(cvs_primary), offsetof(cvs_primary, pre), offsetof(cvs_primary, matrix), offsetof(cvs_primary, post), offsetof(cvs_primary, flags));\n'
             + '    printf(" %d %d %d\\n", CVS_CURVES_MIN_SIZE, CVS_CURVES_MAX_SIZE, CVS_PRIMARY_MATRIX);\n    return 0;\n}\n')
    cp, pp = _lib.curves_params, _lib.primary_params
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "probe.c")
        with open(src, "w") as f:
            f.write(probe)
        for cc, std, lang in (("gcc", "-std=c99", "c"), ("g++", "-std=c++14", "c++")):
            exe = os.path.join(tmp, "probe_" + cc)
            subprocess.run([cc, std, "-Wall", "-Werror", "-x", lang, src, "-I", os.path.join(ROOT, "include"), "-o", exe], check=True)
            got = [int(v) for v in subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout.split()]
            assert got[:4] == [C.sizeof(cp), cp.size.offset, cp.domain_min.offset, cp.domain_max.offset] and got[0] == 28
            assert got[4:9] == [C.sizeof(pp), pp.pre.offset, pp.matrix.offset, pp.post.offset, pp.flags.offset] and got[4] == 108
            assert got[9:] == [_lib.CURVES_MIN_SIZE, _lib.CURVES_MAX_SIZE, _lib.PRIMARY_MATRIX] == [2, 4097, 1]
    p = _lib.primary()
    assert (p.pre.size, p.post.size, p.flags, list(p.matrix)) == (0, 0, 0, [0.0] * 12)
    p = _lib.primary(5, [[1, 2, 3, 4], [5, 6, 7, 8], [9, 10, 11, 12]], (17, (0, -1, 0.5), (1, 2, 3)))
    assert (p.pre.size, list(p.pre.domain_min), list(p.pre.domain_max)) == (5, [0, 0, 0], [1, 1, 1])
    assert (p.post.size, list(p.post.domain_min), list(p.post.domain_max), p.flags) == (17, [0, -1, 0.5], [1, 2, 3], 1)
    assert list(p.matrix) == [float(v) for v in range(1, 13)]
    F16, F32P, PP = C.POINTER(_lib.rgba_frame_f16), C.POINTER(_lib.rgba_frame_f32), C.POINTER(pp)
    fp = C.POINTER(C.c_float)
    assert _lib.PRIMARY_SIGNATURES == {"cvs_curves_bytes": (C.c_size_t, [C.c_int]), "cvs_curves_pack": (C.c_int, [fp, fp, C.c_int]),
                                       ENTRIES[0]: (C.c_int, [F16, F16, PP, C.c_void_p, C.c_void_p, C.c_void_p]),
                                       ENTRIES[1]: (C.c_int, [F32P, F32P, PP, C.c_void_p, C.c_void_p, C.c_void_p])}


def test_every_symbol_of_the_header_is_exported_and_bound(lib):
    from canvas_amd import _lib
    funcs, entries = _declared(HEADER)
    assert funcs == sorted(_lib.PRIMARY_SIGNATURES) and entries == ENTRIES
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert set(funcs) <= {line.split()[-1] for line in out.splitlines() if line.strip()}
    others = (set(_lib.SIGNATURES) | set(_lib.SCOPE_SIGNATURES) | set(_lib.LUT3D_SIGNATURES) | set(_lib.PERSPECTIVE_SIGNATURES) | set(_lib.DEINTERLACE_SIGNATURES)
              | set(_lib.MEDIAN_SIGNATURES) | set(_lib.TEMPORAL_SIGNATURES) | set(_lib.YCC422_SIGNATURES))
    assert not set(_lib.PRIMARY_SIGNATURES) & others
    for name in funcs:
        assert getattr(lib, name).argtypes == _lib.PRIMARY_SIGNATURES[name][1] and getattr(lib, name).restype is _lib.PRIMARY_SIGNATURES[name][0]
    # the header states the contract's two properties and the in-place rule, and canvas_hip.h does not declare the entries
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    assert "in place is bit for bit the out-of-place result" in text and "returns that node's value exactly" in text and "K - 1 is a power of two" in text
    assert "cvs_primary" not in open(os.path.join(ROOT, "include", "canvas_hip.h")).read()
    # one launcher, one arithmetic flavour; grade.hpp, the chain's colour stage, is another thing
    symbols = subprocess.run(["nm", _lib.LIB_PATH], stdout=subprocess.PIPE, text=True).stdout
    assert re.search(r"\bcvk_primary\b", symbols) and not re.search(r"\bcvk_primary_fma\b", symbols)


def test_bytes_and_pack(lib):
    from canvas_amd import _lib
    for size in (2, 3, 17, 1024, 4097):
        assert lib.cvs_curves_bytes(size) == 12 * size
    for size in (1, 0, -1, 4098, 2 ** 30):
        lib.cvs_clear_last_error()
        assert lib.cvs_curves_bytes(size) == 0
        assert "cvs_curves_bytes" in _lib.last_error() and "outside 2..4097" in _lib.last_error()
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    for size in (2, 5, 4097):
        cv = pm.distinct(size, pm.UNIT, 1)
        rows = np.ascontiguousarray(cv.table.reshape(-1))
        out = np.full(size * 3 + 8, 7.0, F32)
        assert lib.cvs_curves_pack(fp(out[4:]), fp(rows), size) == 0
        assert np.array_equal(out[4:-4], cv.planar()) and (out[:4] == 7).all() and (out[-4:] == 7).all()
        assert np.array_equal(out[4:4 + size], cv.table[:, 0]) and np.array_equal(out[4 + 2 * size:-4], cv.table[:, 2])
        for bad in (np.nan, np.inf, -np.inf):
            for at in (0, 3 * size - 1, 4):
                poisoned = rows.copy()
                poisoned[at] = bad
                lib.cvs_clear_last_error()
                assert lib.cvs_curves_pack(fp(out[4:]), fp(poisoned), size) == -1
                assert "cvs_curves_pack" in _lib.last_error() and "not finite" in _lib.last_error() and "value %d " % at in _lib.last_error()
    rows, out = np.zeros(24, F32), np.zeros(32, F32)
    for size in (1, 4098, -3):
        lib.cvs_clear_last_error()
        assert lib.cvs_curves_pack(fp(out), fp(rows), size) == -1 and "outside 2..4097" in _lib.last_error()
    lib.cvs_clear_last_error()
    assert lib.cvs_curves_pack(None, fp(rows), 2) == -1 and "need" in _lib.last_error()
    assert lib.cvs_curves_pack(fp(out), None, 2) == -1


def test_entries_refuse_in_the_headers_order_before_anything_is_launched(lib):
    """A call that breaks rules k and k + 1 of the header's list is refused with rule k's message; every refusal empties the
    target's window."""
    from canvas_amd import _lib
    from canvas_amd.abi import HostFrame
    full = (0, 0, 7, 7)
    lim = _lib.MAX_COORD
    nan, inf = float("nan"), float("inf")
    raw = np.zeros(64, F32)
    table = raw.ctypes.data + (-raw.ctypes.data % 16)
    box = _lib.box2i.of
    for name, dtype, frame_t in (("cvs_primary_f16_dev", np.uint16, _lib.rgba_frame_f16), ("cvs_primary_f32_dev", np.float32, _lib.rgba_frame_f32)):
        entry = getattr(lib, name)

        def fresh(cur=full):
            return HostFrame(full, dtype, current_window=cur)

        def refused(target, source, p, pre, post, word):
            lib.cvs_clear_last_error()
            assert entry(target, source, None if p is None else C.byref(p), pre, post, None) == -1, (name, word)
            assert name in _lib.last_error() and word in _lib.last_error(), (name, word, _lib.last_error())
        good = fresh()
        outside = fresh((0, 0, 8, 7))
        far = frame_t(good.c.data, box(lim - 6, 0, lim + 1, 7), box(lim - 6, 0, lim + 1, 7))
        # the ten rules, each as (p, pre, post, source, word); rule k's case also breaks rule k + 1
        rules = [
            (None, table, None, good, "need"),                                                          # 1 (and nothing else can be looked at)
            (_lib.primary(flags=2), None, None, good, "no stage"),                                      # 2, with 3
            (_lib.primary(1, flags=3), table, None, good, "unknown flags"),                             # 3, with 4
            (_lib.primary((4098, (0, 0, 0), (1, 0, 1))), table, None, good, "outside 2..4097"),         # 4, with 5
            (_lib.primary((2, (0, 0, 0), (1, 0, 1))), None, None, good, "finite and ascending"),        # 5, with 6
            (_lib.primary(2), table + 4, table, good, "16-byte"),                                       # 6, with 7
            (_lib.primary(2, [nan] * 12), table, table, good, "absent"),                                # 7, with 8
            (_lib.primary(2, [inf] * 12), table, None, outside, "not finite"),                          # 8, with 9
            (_lib.primary(2), table, None, frame_t(good.c.data, box(lim - 6, 0, lim + 1, 7), box(lim - 6, 0, lim + 2, 7)), "outside its buffer"),   # 9, with 10
            (_lib.primary(2), table, None, far, "beyond"),                                              # 10
        ]
        for p, pre, post, source, word in rules:
            out = fresh()
            refused(out.ref(), source.ref() if hasattr(source, "ref") else C.byref(source), p, pre, post, word)
            assert out.current_window.is_empty(), word
        out = fresh()
        refused(out.ref(), None, _lib.primary(2), table, None, "need")
        assert out.current_window.is_empty()
        refused(None, good.ref(), _lib.primary(2), table, None, "need")
        # more of each kind
        more = [(_lib.primary(size), table, None, "outside 2..4097") for size in (1, -5, 4098, 100000)]
        more += [(_lib.primary(None, None, size), None, table, "outside 2..4097") for size in (1, 4098)]
        more += [(_lib.primary((2, lo, hi)), table, None, "finite and ascending") for lo, hi in (
            ((0, 0, 0), (1, 1, 0)), ((0, 0.5, 0), (1, 0.5, 1)), ((2, 0, 0), (1, 1, 1)), ((nan, 0, 0), (1, 1, 1)), ((0, 0, 0), (1, nan, 1)),
            ((0, 0, -inf), (1, 1, 1)), ((0, 0, 0), (inf, 1, 1)))]
        more += [(_lib.primary(None, None, (2, (0, 0, 0), (1, 1, 0))), None, table, "finite and ascending")]
        more += [(_lib.primary(2), table + off, None, "16-byte") for off in (4, 8, 12, 1)]
        more += [(_lib.primary(2, None, 3), table, None, "need their table"), (_lib.primary(None, MATRIX), None, table, "absent"), (_lib.primary(None, MATRIX), table, None, "absent")]
        more += [(_lib.primary(2, flags=flags), table, None, "unknown flags") for flags in (2, 3, -1, 0x100)]
        more += [(_lib.primary(None, [0.0] * k + [bad] + [0.0] * (11 - k)), None, None, "not finite") for k in (0, 3, 11) for bad in (nan, inf, -inf)]
        for p, pre, post, word in more:
            out = fresh()
            refused(out.ref(), good.ref(), p, pre, post, word)
            assert out.current_window.is_empty(), word
        # an absent matrix is not looked at; an absent stage's domain neither
        quiet = _lib.primary(2, [nan] * 12, flags=0)
        quiet.post.domain_min[0] = nan
        far_target = frame_t(good.c.data, box(0, -lim - 1, 7, -lim + 6), box(0, 0, 7, 7))
        refused(C.byref(far_target), good.ref(), quiet, table, None, "beyond")
        assert far_target.current_window.is_empty() and good.current_window.tuple() == full       # a refused call leaves its source alone
        # in place: the one frame's window is emptied by a refusal
        both = fresh()
        refused(both.ref(), both.ref(), _lib.primary(9999), table, None, "outside 2..4097")
        assert both.current_window.is_empty()
        if lib.cvs_device_count() == 0:
            # without a device a call that nothing refuses still fails, loudly, and computes nothing on the CPU
            lib.cvs_clear_last_error()
            out = fresh()
            assert entry(out.ref(), good.ref(), C.byref(_lib.primary(2)), table, None, None) != 0 and "no CPU path" in _lib.last_error()
            assert out.current_window.is_empty()


def test_code_object_holds_the_21_instances_without_scratch():
    """One build for both arithmetic flavours; three pixel layouts (f32, f16 one pixel per lane, f16 pairs) x the seven stage
    combinations, each its own instance (presence is a template parameter); no private segment, no spills, and no register read
    between a load into it and the wait that retires it."""
    assert os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"), "the ROCm LLVM tools the build itself needs are missing"
    found = _kernels("primary_ops.hip.o")
    assert len(found) == 21 and all("k_primary" in n for n in found), sorted(found)
    for half in (0, 1, 2):
        for pre, mat, post in ((a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1) if a or b or c):
            assert any("k_primaryILi%dELb%dELb%dELb%dEEE" % (half, pre, mat, post) in n for n in found), (half, pre, mat, post)
    for name, (scratch, spills) in found.items():
        assert scratch == 0 and spills == 0, (name, scratch, spills)
    assert not os.path.exists(os.path.join(ROOT, "canvas_amd", "csrc", "build", "primary_ops.fma.hip.o"))
    spec = __import__("importlib.util").util.spec_from_file_location("check_asm_loads", os.path.join(ROOT, "tools", "check_asm_loads.py"))
    chk = __import__("importlib.util").util.module_from_spec(spec)
    spec.loader.exec_module(chk)
    checked, problems = chk.check_paths([os.path.join(ROOT, "canvas_amd", "csrc", "build", "primary_ops.hip.o")])
    assert checked >= 21 and not problems, problems[:5]


# ---------------------------------------------------------------- the catalogue

def test_every_device_entry_of_the_header_has_its_catalogue_cases():
    """What tests/test_entry_cases_cpu.py holds tests/entry_cases.py to, for tests/primary_cases.py: every cvs_*_dev entry the
    header declares is CALLED by a case, each call is handed the factory's stream, every case has an output and asks for the same
    operands every time, the tables are "f32" buffers of 12 * K bytes, and the Shifted factory moves every frame and changes no
    buffer, so the far-window harness runs the cases as it runs the catalogue's."""
    from tests import entry_cases as ec
    from tests import primary_cases as pc
    from tests.test_entry_cases_cpu import Geometry, HostOnly, Recorder, _check_shifted
    _funcs, entries = _declared(HEADER)
    assert entries == sorted(pc.ENTRIES)
    seen, stream, cases, combos = {}, 0x5EED, 0, set()
    for gid, build in pc.GROUPS:
        rec = Recorder()
        for what, case in build(rec):
            cases += 1
            before = len(rec.calls)
            fac = HostOnly(rec, stream)
            assert case(fac) == 0
            made = rec.calls[before:]
            assert len(made) == 1 and made[0][1] == stream, (gid, what, made)
            seen.setdefault(made[0][0], []).append(what)
            assert any(o.out for o in fac.objects), (gid, what)
            held = [o for o in fac.objects if o.frame is None]
            assert len(held) <= 2 and all(o.cls == "f32" and not o.out and o.nbytes % 12 == 0 and 2 <= o.nbytes // 12 <= 4097 for o in held)
            combos.add((any(o.name == "pre" for o in held), "%r, True, " % None in what or ", True, " in what, any(o.name == "post" for o in held)))
            again = HostOnly(rec, stream)
            case(again)
            spec = lambda f: [(o.cls, o.name, o.out, o.cmp, o.nbytes, o.row_bytes, o.reads) for o in f.objects]
            assert spec(fac) == spec(again), (gid, what)
            boxes = [(o.out, o.frame.c.full_window.tuple()) for o in fac.objects if o.frame is not None]
            assert len(ec.far_offsets(pc.FAR_RULE, boxes)) >= 4, (gid, what)
    assert sorted(seen) == entries and len(seen[ENTRIES[0]]) == len(seen[ENTRIES[1]]) + 3 and cases == sum(len(v) for v in seen.values())
    assert any("in place" in w for w in seen[ENTRIES[1]]) and any("all codes" in w for w in seen[ENTRIES[0]])
    assert len(combos) == 7, sorted(combos)
    frames = 0
    for gid, build in pc.GROUPS:
        a, b = Geometry(), Geometry()
        for (what, near), (_, far) in zip(build(a), build(b)):
            frames += _check_shifted(gid, what, (near, far, a, b), pc.FAR_RULE["source_scale"])
    assert frames == 2 * cases                                       # two frame arguments per call (in place: the one frame twice)


# ---------------------------------------------------------------- ColorCurves and the node

def test_color_curves_value(process):
    rows = [(0.0, 0.1, 0.2), (0.5, 0.25, 0.75), (1.0, 0.9, 0.8)]
    cv = process.ColorCurves(3, rows)
    assert (cv.size, cv.domain_min, cv.domain_max) == (3, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    flat = np.array(rows, F32)
    assert cv.table == flat.tobytes()
    for table in ([v for row in rows for v in row], flat, flat.reshape(-1), flat.astype(np.float64), [list(r) for r in rows], tuple(rows)):
        assert process.ColorCurves(3, table).table == flat.tobytes()
    cv = process.ColorCurves(2, [0, 0, 0, 1, 1, 1], (-0.25, 0, 0.5), domain_max=(1, 2, 0.5 + 2.0 ** -10))
    assert cv.domain_min == (-0.25, 0.0, 0.5) and cv.domain_max == (1.0, 2.0, 0.5 + 2.0 ** -10)
    # rows of whole numbers: a 2-D integer array, whose rows are sequences and (to PyNumber_Check) numbers at once
    whole = np.array([[0, 0, 0], [1, 2, 3], [4, 5, 6]], np.int64)
    assert process.ColorCurves(3, whole).table == whole.astype(F32).tobytes() == process.ColorCurves(3, whole.reshape(-1)).table
    assert process.ColorCurves(3, whole.astype(np.int16)).table == whole.astype(F32).tobytes()
    big = process.ColorCurves(4097, np.zeros((4097, 3), F32))
    assert big.size == 4097 and len(big.table) == 12 * 4097
    with pytest.raises(TypeError):
        cv.__init__(2, [0] * 6)                                         # immutable
    for attr in ("size", "table", "domain_min", "domain_max"):
        with pytest.raises(AttributeError):
            setattr(cv, attr, 1)
    for args, word in (((1, [0] * 3), "outside 2..4097"), ((4098, [0] * (3 * 4098)), "outside 2..4097"), ((2, [0] * 5), "holds 5 values"), ((2, [0] * 7), "holds 7 values"),
                       ((2, [0, 0, 0, 1, float("nan"), 1]), "not finite"), ((2, [0, 0, 0, 1, float("inf"), 1]), "not finite"), ((2, [(0, 0, 0), (1, 1)]), "three numbers"),
                       ((2, [0] * 6, (0, 0, 0), (1, 0, 1)), "ascending"), ((2, [0] * 6, (0, float("nan"), 0), (1, 1, 1)), "ascending")):
        with pytest.raises((ValueError, TypeError), match=word):
            process.ColorCurves(*args)
    with pytest.raises(TypeError):
        process.ColorCurves(2, 5)
    with pytest.raises(TypeError):
        process.ColorCurves(2, ["a"] * 6)


def test_node_arguments_and_properties(process):
    red = process.SolidColorVideoSource((1, 0, 0, 1))
    a, b = process.ColorCurves(2, [0, 0, 0, 1, 1, 1]), process.ColorCurves(3, [0] * 9)
    node = process.VideoColorCorrectFilter(red)
    assert node.source is red and node.pre is None and node.matrix is None and node.post is None
    node = process.VideoColorCorrectFilter(red, a, MATRIX, b)
    assert node.pre is a and node.post is b and node.matrix == tuple(float(F32(v)) for v in MATRIX)
    node = process.VideoColorCorrectFilter(source=red, post=a, matrix=[MATRIX[0:4], MATRIX[4:8], MATRIX[8:12]])
    assert node.pre is None and node.post is a and node.matrix == tuple(float(F32(v)) for v in MATRIX)
    node.pre, node.post = b, None
    assert node.pre is b and node.post is None
    node.matrix = None
    assert node.matrix is None
    node.matrix = range(12)
    assert node.matrix == tuple(float(v) for v in range(12))
    # a refused value raises and keeps the old one
    for attr, value, error in (("pre", 3, TypeError), ("post", "curves", TypeError), ("pre", [0, 0, 0, 1, 1, 1], TypeError), ("matrix", [1.0] * 11, ValueError), ("matrix", [[1, 0, 0], [0, 1, 0], [0, 0, 1]], (ValueError, TypeError)),
                               ("matrix", [0.0] * 11 + [float("nan")], ValueError), ("matrix", [float("inf")] + [0.0] * 11, ValueError), ("matrix", 5, TypeError), ("matrix", ["a"] * 12, TypeError)):
        with pytest.raises(error):
            setattr(node, attr, value)
        assert node.pre is b and node.post is None and node.matrix == tuple(float(v) for v in range(12)), (attr, value)
    for kwargs in (dict(pre=3), dict(post=MATRIX), dict(matrix=[1, 2, 3]), dict(matrix=[float("nan")] * 12)):
        with pytest.raises((TypeError, ValueError)):
            process.VideoColorCorrectFilter(red, **kwargs)
    with pytest.raises(TypeError):
        process.VideoColorCorrectFilter()
    node.set_source(None)
    assert node.source is None
    node.source = red
    assert node.source is red
    assert hasattr(node, "_video_frame_source_funcs") and hasattr(node, "get_frame_f16") and hasattr(node, "get_frame_f32")


def test_pull_without_a_device_gives_an_empty_window_and_says_why():
    """In a child process that sees no GPU: pulled as f16 and as f32, with and without a source."""
    script = r"""
import sys
sys.path.insert(0, %r)
from fluggo.media import process, basetypes, grade
window = basetypes.box2i(0, 0, 31, 17)
red = process.SolidColorVideoSource((1, 0, 0, 1))
curves = process.ColorCurves(3, grade.identity_curves(3))
for source in (red, None):
    node = process.VideoColorCorrectFilter(source, curves, grade.saturation_matrix(0.5))
    assert node.get_frame_f16(0, window).current_window.empty()
    assert node.get_frame_f32(0, window).current_window.empty()
    node.pre = None
    assert node.get_frame_f32(0, window).current_window.empty()
    assert process.last_error(), "no message"
print("message:", process.last_error())
""" % ROOT
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    p = subprocess.run([os.sys.executable, "-c", script], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout
    assert "message:" in p.stdout and re.search(r"device|HIP|hip", p.stdout), p.stdout


def test_the_f16_model_truncates_once():
    """(what the GPU tests hold the f16 entry to) the f16 result is the f32 result truncated, not rounded to nearest"""
    cv = pm.Curves([[0.3, 0.3, 0.3], [0.3, 0.3, 0.3]])
    pixels = np.full((1, 1, 4), 0x3800, np.uint16)
    assert pm.apply_pixels(pixels, cv)[0, 0, 0] == f2h_rz_model(np.array([0.3], F32))[0] == 0x34CC
