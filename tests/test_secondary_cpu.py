"""The secondaries without a GPU (DESIGN.md "Secondaries"): include/canvas_secondary.h against the library and its bindings; the
alias policy in the header's text against a table; properties of the numpy model (tests/secondary_model.py); every refusal of the
four entries, which comes before the device is touched; the catalogue of tests/secondary_cases.py; the two nodes' and
grade.secondary's arguments and attributes; the built code object."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from tests import secondary_model as sm
from tests.models import f2h_rz_model
from tests.test_perspective_cpu import _declared
from tests.test_unsharp_cpu import _kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "canvas_secondary.h"
ENTRIES = ["cvs_matte_mix_f16_dev", "cvs_matte_mix_f32_dev", "cvs_qualify_f16_dev", "cvs_qualify_f32_dev"]
F32 = np.float32
INF, NAN = float("inf"), float("nan")
# the header's policy for operands that share a buffer: entry -> {pair: policy}; REFUSED: none
ALIAS = {}
for _fmt in ("f16", "f32"):
    ALIAS["cvs_qualify_%s_dev" % _fmt] = {("target", "source"): "in place", ("target", "key"): "in place", ("source", "key"): "shared"}
    ALIAS["cvs_matte_mix_%s_dev" % _fmt] = {("target", "a"): "in place", ("target", "b"): "in place", ("target", "matte"): "in place",
                                           ("a", "b"): "shared", ("a", "matte"): "shared", ("b", "matte"): "shared"}


@pytest.fixture(scope="module")
def process():
    from fluggo.media import process
    return process


@pytest.fixture(scope="module")
def lib():
    from canvas_amd import _lib
    return _lib.load()


def px(*rows):
    """(1, n, 4) f32 pixels from (r, g, b[, a]) rows; alpha 1 where it is not given"""
    return np.array([[list(r) + [1.0] * (4 - len(r)) for r in rows]], F32)


# ---------------------------------------------------------------- the model's properties

def test_pure_primaries_have_whole_hues():
    p = px((1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 1, 1), (0, 0, 1), (1, 0, 1), (0.25, 0, 0), (7, 7, 0.5))
    h, c = sm.hue_of(p[..., 0], p[..., 1], p[..., 2])
    assert h[0].tolist() == [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 0.0, 1.0] and (c[0] > 0).all()


def test_greys_are_never_selected_by_hue_and_always_by_its_inverse():
    greys = px((0, 0, 0), (0.5, 0.5, 0.5), (1, 1, 1), (-0.25, -0.25, -0.25), (-0.0, 0.0, -0.0), (INF, INF, INF), (65504, 65504, 65504))
    for hue in ((0, 360, 0), (0, 360, 30), (180, 10, 0), (350, 40, 20)):
        assert (sm.matte_of(greys, sm.Qualifier(hue=hue)) == 0).all(), hue
        assert (sm.matte_of(greys, sm.Qualifier(hue=hue, invert=True)) == 1).all(), hue


def test_no_axis_returns_the_sources_codes():
    from tests import secondary_cases as sc
    for half in (True, False):
        pixels = sc.picture(np.random.default_rng(5), half, (0, 0, 130, 8)).array
        out = sm.qualify_pixels(pixels, None, sm.Qualifier())
        wide = sm.widen(pixels) if half else pixels
        raw = (lambda a: a) if half else (lambda a: np.ascontiguousarray(a).view(np.uint32))
        assert np.array_equal(raw(out)[..., :3], raw(pixels)[..., :3])
        # alpha times exactly 1: the code it was (a NaN alpha comes back quiet); a pixel with a NaN colour is not selected
        measured = ~np.isnan(wide[..., :3]).any(axis=-1)
        plain = measured & ~np.isnan(wide[..., 3])
        assert plain.sum() > 1000 and np.array_equal(raw(out)[..., 3][plain], raw(pixels)[..., 3][plain])
        assert (~measured).any() and np.isin(raw(out)[..., 3][~measured & ~np.isnan(wide[..., 3]) & np.isfinite(wide[..., 3])] & (0x7FFF if half else 0x7FFFFFFF), [0]).all()


def test_width_360_selects_every_chromatic_pixel():
    from tests import secondary_cases as sc
    pixels = sm.widen(sc.picture(np.random.default_rng(6), True, (0, 0, 130, 8)).array)
    finite = np.isfinite(pixels[..., :3]).all(axis=-1)                          # (Inf - Inf and Inf / Inf leave no hue to measure)
    _, c = sm.hue_of(pixels[..., 0], pixels[..., 1], pixels[..., 2])
    assert (finite & (c > 0)).sum() > 1000 and (finite & ~(c > 0)).sum() > 10
    for center in (0, 77, 200, 359.5, -40):
        m = sm.matte_of(pixels, sm.Qualifier(hue=(center, 360, 0)))
        assert np.array_equal((m == 1)[finite], (c > 0)[finite]) and np.isin(m, [0, 1]).all(), center


def test_a_hue_range_through_zero_selects_both_sides_alike():
    def at(deg):
        h = deg / 60.0
        return (1.0, h, 0.0) if h < 1 else (1.0, 0.0, 6.0 - h)                 # hue h in sextant 0, or in sextant 5
    p = px(at(5), at(340), at(355), at(0), at(331), at(9), at(11), at(329), at(180 + 170))
    hard = sm.matte_of(p, sm.Qualifier(hue=(350, 40, 0)))[0]
    assert hard.tolist() == [1, 1, 1, 1, 1, 1, 0, 0, 1]
    soft = sm.matte_of(p, sm.Qualifier(hue=(350, 40, 20)))[0]
    assert soft[0] == soft[1] == 1 and 0 < soft[6] < 1 and 0 < soft[7] < 1 and soft[6] == pytest.approx(soft[7], abs=1e-5)
    assert np.array_equal(sm.matte_of(p, sm.Qualifier(hue=(-10, 40, 20))), sm.matte_of(p, sm.Qualifier(hue=(350, 40, 20))))
    assert np.array_equal(sm.matte_of(p, sm.Qualifier(hue=(710, 40, 20))), sm.matte_of(p, sm.Qualifier(hue=(350, 40, 20))))


def test_the_r_max_test_comes_first():
    """r == g == mx: the hue is the red branch's, (g - b) / c = 1, not the green branch's (b - r) / c + 2 = 1 -- the same here --
    but r == b == mx is 5 by the red branch's wrap ((g - b) / c = -1, + 6) and would be 4 + (r - g) / c = 5 too; the branches
    differ where they must: g == b == mx > r is 3 by the green branch, and 5 by the blue one would be wrong."""
    p = px((1, 1, 0), (1, 0, 1), (0, 1, 1), (0.5, 0.5, 0.25))
    h, _ = sm.hue_of(p[..., 0], p[..., 1], p[..., 2])
    assert h[0].tolist() == [1.0, 5.0, 3.0, 1.0]


def test_the_edges_of_a_value_range():
    low, soft = F32(0.25), F32(0.125)
    v = np.array([low, low - soft, np.nextafter(low, F32(0)), low - soft / 2, 0.75, np.nextafter(F32(0.75), F32(1)), 0.875, 1.0, INF, NAN], F32)
    r = sm.range_of((0.25, 0.75, 0.125, 0.25), v)
    assert r[0] == 1 and r[1] == 0 and 0 < r[2] < 1 and r[3] == 0.5 and r[4] == 1 and 0 < r[5] < 1 and r[6] == 0.5 and r[7] == 0 and r[8] == 0 and r[9] == 0
    hard = sm.range_of((0.25, 0.75, 0, 0), v)
    assert hard.tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 0, 0]
    unbounded = sm.range_of((0.25, INF, 0, 0), v)
    assert unbounded.tolist() == [1, 0, 0, 0, 1, 1, 1, 1, 1, 0]
    # through the qualifier: a grey's luma is its value (the three weights sum to 1 within an ulp), its saturation 0
    greys = px((0.5, 0.5, 0.5), (0.1, 0.1, 0.1))
    assert sm.matte_of(greys, sm.Qualifier(luma=(0.25, 0.75, 0, 0)))[0].tolist() == [1, 0]
    assert sm.matte_of(greys, sm.Qualifier(saturation=(0, 0, 0, 0)))[0].tolist() == [1, 1]
    assert sm.matte_of(px((1, 0.5, 0.5)), sm.Qualifier(saturation=(0.5, 0.5, 0, 0)))[0].tolist() == [1]


def test_nan_in_the_key_selects_nothing():
    p = px((NAN, 0.5, 0.2), (0.5, NAN, 0.2), (0.5, 0.2, NAN), (NAN, NAN, NAN), (0.5, 0.2, 0.1, NAN))
    for q in (sm.Qualifier(hue=(0, 360, 0)), sm.Qualifier(saturation=(0, INF, 0, 0)), sm.Qualifier(luma=(-1, INF, 1, 0)), sm.Qualifier()):
        m = sm.matte_of(p, q)[0]
        assert m.tolist() == [0, 0, 0, 0, 1], q                                # (the key's alpha plays no part)
    source = np.full((1, 5, 4), 0x3800, np.uint16)
    out = sm.qualify_pixels(source, f2h_rz_model(np.nan_to_num(p, nan=0.0)) | np.where(np.isnan(p), 0x7E00, 0).astype(np.uint16), sm.Qualifier(hue=(0, 360, 0)))
    assert out[0, :, 3].tolist() == [0, 0, 0, 0, 0x3800] and (out[..., :3] == 0x3800).all()


def test_the_mix_selects_at_the_ends():
    specials = np.array([[INF, -INF, NAN, 0.25], [-0.0, 1e-42, 3e38, NAN]], F32)[None]
    others = np.array([[1, 2, 3, 4], [NAN, INF, -3e38, 0.5]], F32)[None]
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    for luma, field in ((False, 3), (True, slice(0, 3))):
        zero, one = np.zeros((1, 2, 4), F32), np.zeros((1, 2, 4), F32)
        one[..., field] = 1.0
        over = one * F32(7)
        under = zero - F32(1)
        for matte, invert, want in ((zero, False, specials), (one, False, others), (zero, True, others), (one, True, specials), (over, False, others), (under, False, specials)):
            if luma and matte is one:
                assert sm.weight_of(one, True)[0, 0] == 1.0                      # (the weights of 1, 1, 1 round to a luma of exactly 1)
            assert np.array_equal(bits(sm.mix_pixels(specials, others, matte, luma, invert)), bits(want)), (luma, invert)
    nan_matte = np.full((1, 2, 4), NAN, F32)
    assert np.array_equal(bits(sm.mix_pixels(specials, others, nan_matte)), bits(specials))             # sel(NaN) = 0
    a16, b16 = np.array([[[0x7C00, 0xFC00, 0x7E01, 0x0001]]], np.uint16), np.array([[[0x3C00, 0x8000, 0xFFFF, 0x7BFF]]], np.uint16)
    for code, want in ((0x0000, a16), (0x8000, a16), (0x3C00, b16), (0x7BFF, b16), (0xBC00, a16), (0x7E00, a16)):
        m16 = np.full((1, 1, 4), code, np.uint16)
        assert np.array_equal(sm.mix_pixels(a16, b16, m16), want), hex(code)
    half = sm.mix_pixels(np.full((1, 1, 4), 0x3400, np.uint16), np.full((1, 1, 4), 0x3C00, np.uint16), np.full((1, 1, 4), 0x3800, np.uint16))
    assert (half == 0x3900).all()                                              # 0.25 + 0.5 * 0.75 = 0.625


def test_the_secondary_graph_leaves_alpha_and_unselected_pixels_alone():
    """the model of grade.secondary on an opaque picture: qualify, then mix the source with a graded copy through the result"""
    from tests import primary_model as pm
    rng = np.random.default_rng(11)
    source = f2h_rz_model(rng.uniform(0, 1, (9, 33, 4)).astype(F32))
    source[..., 3] = 0x3C00
    graded = pm.apply_pixels(source, None, [0.5, 0.5, 0, 0.1, 0, 1, 0, 0, 0.2, 0, 0.8, 0], None)
    q = sm.Qualifier(hue=(120, 60, 30), saturation=(0.2, INF, 0.1, 0))
    matte = sm.qualify_pixels(source, None, q)
    out = sm.mix_pixels(source, graded, matte)
    m = sm.matte_of(sm.widen(source), q)
    assert (out[..., 3] == 0x3C00).all()
    assert (m == 0).any() and (m == 1).any() and ((m > 0) & (m < 1)).any()
    assert np.array_equal(out[m == 0], source[m == 0]) and np.array_equal(out[m == 1], graded[m == 1])
    assert (out[(m > 0) & (m < 1)] != source[(m > 0) & (m < 1)]).any()


def test_the_f16_model_truncates_once():
    source = np.array([[[0x3800, 0x3800, 0x3800, 0x3401]]], np.uint16)             # alpha 0.2501...
    key = f2h_rz_model(px((1.0, 0.3, 0.0)))                                       # hue 0.3 sextants: 18 degrees
    q = sm.Qualifier(hue=(0, 20, 40))
    m = sm.matte_of(sm.widen(key), q)[0, 0]
    assert 0 < m < 1
    a1 = F32(sm.widen(source)[0, 0, 3] * m)
    assert sm.qualify_pixels(source, key, q)[0, 0, 3] == f2h_rz_model(np.array([a1], F32))[0] != np.array([a1], F32).astype(np.float16).view(np.uint16)[0]


# ---------------------------------------------------------------- the header, the library, the bindings

def test_struct_mirrors_have_the_c_layout():
    from canvas_amd import _lib
    assert [n for n, _ in _lib.hue_range._fields_] == ["center", "width", "softness"]
    assert [n for n, _ in _lib.value_range._fields_] == ["low", "high", "soft_low", "soft_high"]
    assert [n for n, _ in _lib.qualifier_params._fields_] == ["flags", "hue", "saturation", "luma"] and [n for n, _ in _lib.matte_mix_params._fields_] == ["flags"]
    probe = ('#include <stddef.h>\n#include <stdio.h>\n#include "%s"\nint main(void) {\n' % HEADER
             + '    printf("%zu %zu %zu", sizeof(cvs_hue_range), sizeof(cvs_value_range), sizeof(cvs_matte_mix));\n'
             + '    printf(" %zu %zu %zu %zu %zu", sizeof(cvs_qualifier), offsetof(cvs_qualifier, flags), offsetof(cvs_qualifier, hue), offsetof(cvs_qualifier, saturation), offsetof(cvs_qualifier, luma));\n'
             + '    printf(" %u %u %u %u %u %u %u\\n", CVS_QUAL_HUE, CVS_QUAL_SATURATION, CVS_QUAL_LUMA, CVS_QUAL_INVERT, CVS_QUAL_SHOW_MATTE, CVS_MMIX_LUMA, CVS_MMIX_INVERT);\n    return 0;\n}\n')
    qp = _lib.qualifier_params
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "probe.c")
        with open(src, "w") as f:
            f.write(probe)
        for cc, std, lang in (("gcc", "-std=c99", "c"), ("g++", "-std=c++14", "c++")):
            exe = os.path.join(tmp, "probe_" + cc)
            subprocess.run([cc, std, "-Wall", "-Werror", "-x", lang, src, "-I", os.path.join(ROOT, "include"), "-o", exe], check=True)
            got = [int(v) for v in subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout.split()]
            assert got[:3] == [C.sizeof(_lib.hue_range), C.sizeof(_lib.value_range), C.sizeof(_lib.matte_mix_params)] == [12, 16, 4]
            assert got[3:8] == [C.sizeof(qp), qp.flags.offset, qp.hue.offset, qp.saturation.offset, qp.luma.offset] and got[3] == 48
            assert got[8:] == [_lib.QUAL_HUE, _lib.QUAL_SATURATION, _lib.QUAL_LUMA, _lib.QUAL_INVERT, _lib.QUAL_SHOW_MATTE, _lib.MMIX_LUMA, _lib.MMIX_INVERT] == [1, 2, 4, 8, 16, 1, 2]
    q = _lib.qualifier()
    assert (q.flags, q.hue.width, q.luma.high) == (0, 0.0, 0.0)
    q = _lib.qualifier(hue=(350, 40, 10), luma=(0.25, INF, 0.5, 0), invert=True)
    assert q.flags == 1 | 4 | 8 and (q.hue.center, q.hue.width, q.hue.softness) == (350.0, 40.0, 10.0) and (q.luma.low, q.luma.high, q.luma.soft_low) == (0.25, INF, 0.5)
    assert _lib.qualifier(saturation=(0, 1, 0, 0), show_matte=True).flags == 2 | 16 and _lib.qualifier(hue=(0, 1, 0), flags=64).flags == 64
    assert [_lib.matte_mix(l, i).flags for l, i in ((False, False), (True, False), (False, True), (True, True))] == [0, 1, 2, 3]
    F16, F32P = C.POINTER(_lib.rgba_frame_f16), C.POINTER(_lib.rgba_frame_f32)
    QP, MP = C.POINTER(qp), C.POINTER(_lib.matte_mix_params)
    assert _lib.SECONDARY_SIGNATURES == {"cvs_qualify_f16_dev": (C.c_int, [F16, F16, F16, QP, C.c_void_p]), "cvs_qualify_f32_dev": (C.c_int, [F32P, F32P, F32P, QP, C.c_void_p]),
                                         "cvs_matte_mix_f16_dev": (C.c_int, [F16, F16, F16, F16, MP, C.c_void_p]),
                                         "cvs_matte_mix_f32_dev": (C.c_int, [F32P, F32P, F32P, F32P, MP, C.c_void_p])}


def test_every_symbol_of_the_header_is_exported_and_bound(lib):
    from canvas_amd import _lib
    funcs, entries = _declared(HEADER)
    assert funcs == sorted(_lib.SECONDARY_SIGNATURES) == entries == ENTRIES
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert set(funcs) <= {line.split()[-1] for line in out.splitlines() if line.strip()}
    others = (set(_lib.SIGNATURES) | set(_lib.SCOPE_SIGNATURES) | set(_lib.LUT3D_SIGNATURES) | set(_lib.PERSPECTIVE_SIGNATURES) | set(_lib.DEINTERLACE_SIGNATURES)
              | set(_lib.MEDIAN_SIGNATURES) | set(_lib.TEMPORAL_SIGNATURES) | set(_lib.YCC422_SIGNATURES) | set(_lib.YCC420_SIGNATURES) | set(_lib.PRIMARY_SIGNATURES))
    assert not set(_lib.SECONDARY_SIGNATURES) & others
    for name in funcs:
        assert getattr(lib, name).argtypes == _lib.SECONDARY_SIGNATURES[name][1] and getattr(lib, name).restype is _lib.SECONDARY_SIGNATURES[name][0]
    hip = open(os.path.join(ROOT, "include", "canvas_hip.h")).read()
    assert "cvs_qualify" not in hip and "cvs_matte_mix" not in hip
    # one launcher each, one arithmetic flavour
    symbols = subprocess.run(["nm", _lib.LIB_PATH], stdout=subprocess.PIPE, text=True).stdout
    for name in ("cvk_qualify", "cvk_matte_mix"):
        assert re.search(r"\b%s\b" % name, symbols) and not re.search(r"\b%s_fma\b" % name, symbols)


def test_the_alias_policy_in_the_headers_text_is_the_table():
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    for words in ("IN PLACE: the entry computes, bit for bit, windows included, what the same call gives on a distinct copy of the input.",
                  "Every lane reads the pixels it writes before it writes them.", "REFUSED: none.", "SHARED: both operands are only read, and may be one buffer."):
        assert words in text, words
    # the same words as the block of canvas_hip.h
    hip = open(os.path.join(ROOT, "include", "canvas_hip.h")).read()
    for words in ("IN PLACE: the entry computes, bit for bit, windows included, what the same call gives on a distinct copy of the input.",
                  "SHARED: both operands are only read, and may be one buffer."):
        assert words in hip
    block = text[text.index("   in place:"):text.index("typedef struct { float center")]
    lists = re.match(r"\s*in place:(.*?)\*\s+refused:(.*?)\*\s+shared:(.*?)\*/", block, re.S)
    assert lists, block
    found = {}
    for policy, body in zip(("in place", "refused", "shared"), lists.groups()):
        for entry, pairs in re.findall(r"(cvs_\w+)((?:\s*\(\w+, \w+\))+)", body):
            for a, b in re.findall(r"\((\w+), (\w+)\)", pairs):
                assert (a, b) not in found.setdefault(entry, {}), (entry, a, b)
                found[entry][(a, b)] = policy
    assert found == ALIAS
    assert not lists.group(2).replace("*", "").strip()                         # refused: none
    # every pair of frame operands of every entry is in the table
    from canvas_amd import _lib
    decl = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for name in ENTRIES:
        params = re.search(r"%s\s*\(([^;]*?)\)\s*;" % name, decl, re.S).group(1)
        frames = [p.split()[-1].lstrip("*") for p in params.split(",") if "rgba_frame" in p]
        assert len(frames) == (3 if "qualify" in name else 4)
        assert {(a, b) for i, a in enumerate(frames) for b in frames[i + 1:]} == set(ALIAS[name]), name
        assert len(frames) == sum(1 for t in _lib.SECONDARY_SIGNATURES[name][1] if t in (C.POINTER(_lib.rgba_frame_f16), C.POINTER(_lib.rgba_frame_f32)))


# ---------------------------------------------------------------- refusals, before the device is touched

def test_entries_refuse_before_anything_is_launched(lib):
    from canvas_amd import _lib
    from canvas_amd.abi import HostFrame
    from tests.test_secondary_gpu import REFUSED_QUALIFIERS
    full = (0, 0, 7, 7)
    lim = _lib.MAX_COORD
    box = _lib.box2i.of
    for half in (True, False):
        dtype, frame_t = (np.uint16, _lib.rgba_frame_f16) if half else (np.float32, _lib.rgba_frame_f32)
        qname, mname = ("cvs_qualify_f16_dev", "cvs_matte_mix_f16_dev") if half else ("cvs_qualify_f32_dev", "cvs_matte_mix_f32_dev")
        qual, mix = getattr(lib, qname), getattr(lib, mname)
        good = HostFrame(full, dtype, current_window=full)
        outside = frame_t(good.c.data, box(*full), box(0, 0, 8, 7))
        far = frame_t(good.c.data, box(lim - 6, 0, lim + 1, 7), box(lim - 6, 0, lim + 1, 7))
        far_target = frame_t(good.c.data, box(0, -lim - 1, 7, -lim + 6), box(0, 0, 7, 7))
        ok_q, ok_m = _lib.qualifier(hue=(0, 60, 0)), _lib.matte_mix()
        g, ref = good.ref(), C.byref

        def refused(name, call, word, target=None):
            out = target or HostFrame(full, dtype, current_window=full)
            lib.cvs_clear_last_error()
            assert call(out.ref() if hasattr(out, "ref") else ref(out)) == -1, (name, word)
            assert name in _lib.last_error() and word in _lib.last_error(), (name, word, _lib.last_error())
            assert out.current_window.is_empty(), (name, word)
        assert len(REFUSED_QUALIFIERS) == 3 + 8 + 24
        for p, word in REFUSED_QUALIFIERS:
            refused(qname, lambda t, p=p: qual(t, g, None, ref(p), None), word)
            refused(qname, lambda t, p=p: qual(t, g, ref(outside), ref(p), None), word)            # the parameters are judged before the windows
        refused(qname, lambda t: qual(t, None, None, ref(ok_q), None), "need")
        refused(qname, lambda t: qual(t, g, g, None, None), "need")
        lib.cvs_clear_last_error()
        assert qual(None, g, None, ref(ok_q), None) == -1 and "need" in _lib.last_error()
        refused(qname, lambda t: qual(t, ref(outside), None, ref(ok_q), None), "outside its buffer")
        refused(qname, lambda t: qual(t, g, ref(outside), ref(ok_q), None), "outside its buffer")
        refused(qname, lambda t: qual(t, ref(far), None, ref(ok_q), None), "beyond")
        refused(qname, lambda t: qual(t, g, ref(far), ref(ok_q), None), "beyond")
        refused(qname, lambda t: qual(t, g, None, ref(ok_q), None), "beyond", target=far_target)
        # an axis whose flag is clear is not looked at: NaNs everywhere, flags for the hue alone
        quiet = _lib.qualifier(hue=(0, 60, 0), saturation=(NAN, NAN, -1, NAN), luma=(INF, -INF, NAN, -1), flags=_lib.QUAL_HUE)
        refused(qname, lambda t: qual(t, g, None, ref(quiet), None), "beyond", target=far_target)
        quiet = _lib.qualifier(hue=(NAN, -1, INF), flags=0)
        refused(qname, lambda t: qual(t, g, None, ref(quiet), None), "beyond", target=far_target)
        for k, args in enumerate(((None, g, g, ref(ok_m)), (g, None, g, ref(ok_m)), (g, g, None, ref(ok_m)), (g, g, g, None))):
            refused(mname, lambda t, args=args: mix(t, *args, None), "need")
        lib.cvs_clear_last_error()
        assert mix(None, g, g, g, ref(ok_m), None) == -1 and "need" in _lib.last_error()
        for flags in (4, 8, 0x80000000):
            bad = _lib.matte_mix(flags=flags)
            refused(mname, lambda t, bad=bad: mix(t, g, g, ref(outside), ref(bad), None), "unknown flags")
        for k in range(3):
            for odd, word in ((outside, "outside its buffer"), (far, "beyond")):
                args = [g, g, g]
                args[k] = ref(odd)
                refused(mname, lambda t, args=args: mix(t, *args, ref(ok_m), None), word)
        refused(mname, lambda t: mix(t, g, g, g, ref(ok_m), None), "beyond", target=far_target)
        # in place: the one frame's window is emptied by a refusal
        both = HostFrame(full, dtype, current_window=full)
        lib.cvs_clear_last_error()
        assert qual(both.ref(), both.ref(), both.ref(), ref(_lib.qualifier(hue=(0, -1, 0))), None) == -1 and both.current_window.is_empty()
        both = HostFrame(full, dtype, current_window=full)
        assert mix(both.ref(), both.ref(), both.ref(), both.ref(), ref(_lib.matte_mix(flags=64)), None) == -1 and both.current_window.is_empty()
        assert good.current_window.tuple() == full                               # a refused call leaves its inputs alone
        if lib.cvs_device_count() == 0:
            # without a device a call that nothing refuses still fails, loudly, and computes nothing on the CPU
            for call in (lambda t: qual(t, g, None, ref(ok_q), None), lambda t: mix(t, g, g, g, ref(ok_m), None)):
                out = HostFrame(full, dtype, current_window=full)
                lib.cvs_clear_last_error()
                assert call(out.ref()) != 0 and "no CPU path" in _lib.last_error() and out.current_window.is_empty()


# ---------------------------------------------------------------- the code object

def test_code_object_holds_the_30_instances_without_lds_or_scratch():
    """One build for both arithmetic flavours; the qualifier's three pixel layouts x key frame or not x hue alone or any axes x matte
    view, the mix's three layouts x alpha or luma; no private segment, no spills, no LDS, and no register read between a load into
    it and the wait that retires it."""
    assert os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"), "the ROCm LLVM tools the build itself needs are missing"
    found = _kernels("secondary_ops.hip.o")
    assert len(found) == 30, sorted(found)
    for half in (0, 1, 2):
        for key, any_, matte in ((a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)):
            assert any("k_qualifyILi%dELb%dELb%dELb%dEEE" % (half, key, any_, matte) in n for n in found), (half, key, any_, matte)
        for luma in (0, 1):
            assert any("k_matte_mixILi%dELb%dEEE" % (half, luma) in n for n in found), (half, luma)
    for name, (scratch, spills) in found.items():
        assert scratch == 0 and spills == 0, (name, scratch, spills)
    build = os.path.join(ROOT, "canvas_amd", "csrc", "build")
    assert not os.path.exists(os.path.join(build, "secondary_ops.fma.hip.o"))
    source = open(os.path.join(ROOT, "canvas_amd", "csrc", "kernels", "secondary_ops.hip")).read()
    assert "__shared__" not in source and "rcp" not in re.sub(r"//.*", "", source)
    spec = __import__("importlib.util").util.spec_from_file_location("check_asm_loads", os.path.join(ROOT, "tools", "check_asm_loads.py"))
    chk = __import__("importlib.util").util.module_from_spec(spec)
    spec.loader.exec_module(chk)
    checked, problems = chk.check_paths([os.path.join(build, "secondary_ops.hip.o")])
    assert checked >= 30 and not problems, problems[:5]


# ---------------------------------------------------------------- the catalogue

def test_every_device_entry_of_the_header_has_its_catalogue_cases():
    """What tests/test_entry_cases_cpu.py holds tests/entry_cases.py to, for tests/secondary_cases.py: every cvs_*_dev entry the
    header declares is CALLED by a case, each call is handed the factory's stream, every case has one output and asks for the same
    operands every time, the model has an answer to every case, and the Shifted factory moves every frame and changes no buffer,
    so the far-window harness runs the cases as it runs the catalogue's.  And the cases cover what they are there to cover."""
    from tests import entry_cases as ec
    from tests import secondary_cases as sc
    from tests.test_entry_cases_cpu import Geometry, HostOnly, Recorder, _check_shifted
    _funcs, entries = _declared(HEADER)
    assert entries == sorted(sc.ENTRIES)
    seen, stream, cases = {}, 0x5EED, 0
    for gid, build in sc.GROUPS:
        rec = Recorder()
        for what, case in build(rec):
            cases += 1
            before = len(rec.calls)
            fac = HostOnly(rec, stream)
            assert case(fac) == 0
            made = rec.calls[before:]
            assert len(made) == 1 and made[0][1] == stream, (gid, what, made)
            seen.setdefault(made[0][0], []).append(what)
            assert sum(1 for o in fac.objects if o.out) == 1 and all(o.frame is not None for o in fac.objects), (gid, what)
            again = HostOnly(rec, stream)
            case(again)
            spec = lambda f: [(o.cls, o.name, o.out, o.cmp, o.nbytes, o.row_bytes, o.reads) for o in f.objects]
            assert spec(fac) == spec(again), (gid, what)
            boxes = [(o.out, o.frame.c.full_window.tuple()) for o in fac.objects]
            assert len(ec.far_offsets(sc.FAR_RULE, boxes)) >= 4, (gid, what)
            want, win = sc.expected(what)
            out = [o for o in fac.objects if o.out][0]
            assert want.shape == ec._box(out.frame.c.full_window.tuple()) + (4,) and want.dtype == (np.uint16 if out.cls == "f16" else np.float32)
    assert sorted(seen) == entries and cases == sum(len(v) for v in seen.values()) == len(sc.CASES)
    d = list(sc.CASES.values())
    qual = [c for c in d if c["op"] == "qualify"]
    assert {c["place"] for c in qual} == {"out", "source", "key"} and {c["key"] for c in qual} == set(sc.KEYS)
    assert {c["place"] for c in d if c["op"] == "mix"} == {"out", "a", "b", "matte"}
    assert {(c["luma"], c["invert"]) for c in d if c["op"] == "mix"} == set(sc.MIXES)
    assert {id(c["q"]) for c in qual} == {id(q) for q in sc.QUALIFIERS}
    for fmt in (True, False):
        assert {(c["sfull"][2] - c["sfull"][0] + 1, c["sfull"][3] - c["sfull"][1] + 1) for c in qual if c["half"] == fmt} == {(w, h) for w in sc.WIDTHS for h in sc.HEIGHTS}
    assert any(c["kcur"] != c["scur"] for c in qual if c["key"] == "distinct") and any(len(set(c["curs"])) == 3 for c in d if c["op"] == "mix")
    assert sum(1 for c in d if c["op"] == "qualify codes") == 3 == sum(1 for c in d if c["op"] == "mix codes")
    qs = sc.QUALIFIERS
    axes = {(q.hue is not None, q.saturation is not None, q.luma is not None) for q in qs}
    assert {(True, False, False), (False, True, False), (False, False, True), (True, True, True), (False, False, False)} <= axes
    assert any(q.hue and q.hue[0] == 350.0 and q.hue[1] == 40.0 for q in qs) and any(q.hue and q.hue[1] == 360.0 for q in qs)
    assert any(q.hue and q.hue[2] == 0 for q in qs) and any(q.hue and q.hue[2] > 0 for q in qs)
    ranges = [r for q in qs for r in (q.saturation, q.luma) if r]
    assert any(r[1] == INF for r in ranges) and any(r[2] == 0 for r in ranges) and any(r[2] > 0 for r in ranges) and any(r[3] == 0 for r in ranges) and any(r[3] > 0 for r in ranges)
    assert any(q.invert for q in qs) and any(q.show_matte for q in qs)
    frames = 0
    for gid, build in sc.GROUPS:
        a, b = Geometry(), Geometry()
        for (what, near), (_, far) in zip(build(a), build(b)):
            frames += _check_shifted(gid, what, (near, far, a, b), sc.FAR_RULE["source_scale"])
    want_frames = sum((2 if c["key"] == "absent" else 3) if c["op"] == "qualify" else {"mix": 4, "qualify codes": 3, "mix codes": 4}[c["op"]] for c in d)
    assert frames == want_frames


# ---------------------------------------------------------------- the nodes and grade.secondary

def test_qualifier_arguments_and_attributes(process):
    red, blue = process.SolidColorVideoSource((1, 0, 0, 1)), process.SolidColorVideoSource((0, 0, 1, 1))
    node = process.VideoQualifierFilter(red)
    assert node.source is red and node.key_source is None and node.hue is None and node.saturation is None and node.luma is None
    assert node.invert is False and node.show_matte is False
    ramp = process.LerpFunc((0.0,), (360.0,), 10)
    node = process.VideoQualifierFilter(red, (ramp, 40, 10.5), saturation=[0.25, INF, 0.125, 0], luma=(0, 1, 0, 0), key_source=blue, invert=True, show_matte=True)
    assert node.hue == (ramp, 40, 10.5) and node.hue[0] is ramp and node.saturation == (0.25, INF, 0.125, 0) and node.luma == (0, 1, 0, 0)
    assert node.key_source is blue and node.invert is True and node.show_matte is True
    node.hue, node.key_source, node.invert, node.show_matte = None, None, False, False
    assert node.hue is None and node.key_source is None and node.invert is False and node.show_matte is False
    node.luma = (0.5, 0.5, ramp, 0)
    assert node.luma[2] is ramp
    # a refused value raises and keeps the old one
    node.hue = (350, 40, 10)
    for attr, value, error in (("hue", (1, 2), ValueError), ("hue", (1, 2, 3, 4), ValueError), ("hue", 5, TypeError), ("hue", "abc", TypeError), ("hue", (NAN, 1, 1), ValueError),
                               ("hue", (0, -1, 0), ValueError), ("hue", (0, 1, INF), ValueError), ("hue", (0, "x", 0), TypeError), ("hue", ((1, 2), 1, 1), TypeError),
                               ("hue", (True, 1, 1), TypeError), ("saturation", (0, 1, 0), ValueError), ("saturation", (0.5, 0.25, 0, 0), ValueError), ("saturation", (0, NAN, 0, 0), ValueError),
                               ("saturation", (INF, INF, 0, 0), ValueError), ("luma", (0, 1, -1, 0), ValueError), ("luma", (0, 1, 0, NAN), ValueError), ("luma", (0, 1, None, 0), TypeError),
                               ("invert", 1, TypeError), ("show_matte", None, TypeError), ("key_source", 3, Exception)):
        with pytest.raises(error):
            setattr(node, attr, value)
        assert node.hue == (350, 40, 10) and node.saturation == (0.25, INF, 0.125, 0) and node.luma[2] is ramp and node.invert is False and node.key_source is None, (attr, value)
    for kwargs in (dict(hue=(1, 2)), dict(saturation=5), dict(luma=(1, 0, 0, 0)), dict(hue=(0, -1, 0))):
        with pytest.raises((TypeError, ValueError)):
            process.VideoQualifierFilter(red, **kwargs)
    with pytest.raises(TypeError):
        process.VideoQualifierFilter()
    with pytest.raises(TypeError):
        del node.hue
    node.set_source(None)
    assert node.source is None
    node.source = red
    assert node.source is red
    assert hasattr(node, "_video_frame_source_funcs") and hasattr(node, "get_frame_f16") and hasattr(node, "get_frame_f32")


def test_matte_mix_arguments_and_attributes(process):
    red, blue, grey = (process.SolidColorVideoSource(c) for c in ((1, 0, 0, 1), (0, 0, 1, 1), (0.5, 0.5, 0.5, 0.5)))
    node = process.VideoMatteMixFilter(red, blue, grey)
    assert node.src_a is red and node.src_b is blue and node.matte is grey and node.channel == "a" and node.invert is False
    node = process.VideoMatteMixFilter(src_a=red, src_b=blue, matte=grey, channel="luma", invert=True)
    assert node.channel == "luma" and node.invert is True
    node.channel, node.invert, node.src_a, node.matte = "a", False, grey, None
    assert node.channel == "a" and node.invert is False and node.src_a is grey and node.matte is None and node.src_b is blue
    for attr, value, error in (("channel", "r", ValueError), ("channel", 3, (TypeError, ValueError)), ("channel", None, (TypeError, ValueError)), ("invert", 0, TypeError), ("src_b", 3, Exception)):
        with pytest.raises(error):
            setattr(node, attr, value)
        assert node.channel == "a" and node.invert is False and node.src_b is blue
    for args in ((red, blue), (red, blue, grey, "alpha")):
        with pytest.raises((TypeError, ValueError)):
            process.VideoMatteMixFilter(*args)
    assert hasattr(node, "_video_frame_source_funcs")


def test_grade_secondary_builds_the_graph(process):
    from fluggo.media import grade
    red, blue = process.SolidColorVideoSource((1, 0, 0, 1)), process.SolidColorVideoSource((0, 0, 1, 1))
    out = grade.secondary(red, blue, hue=(0, 60, 10))
    assert isinstance(out, process.VideoMatteMixFilter) and out.src_a is red and out.src_b is blue and out.channel == "a" and out.invert is False
    assert isinstance(out.matte, process.VideoQualifierFilter) and out.matte.source is red and out.matte.hue == (0, 60, 10) and out.matte.saturation is None
    out = grade.secondary(red, blue, saturation=(0.25, 1, 0.125, 0), luma=(0, 0.5, 0, 0.25), invert=True, choke=-2)
    assert isinstance(out.matte, process.VideoMatteFilter) and isinstance(out.matte.source, process.VideoQualifierFilter)
    q = out.matte.source
    assert q.source is red and q.hue is None and q.saturation == (0.25, 1, 0.125, 0) and q.luma == (0, 0.5, 0, 0.25) and q.invert is True and q.show_matte is False
    assert isinstance(grade.secondary(red, blue, hue=(0, 60, 10), feather=(0.25, 0.5, 0.25)).matte, process.VideoMatteFilter)
    assert isinstance(grade.secondary(red, blue, hue=(0, 60, 10), choke=0, feather=None).matte, process.VideoQualifierFilter)
    with pytest.raises((TypeError, ValueError)):
        grade.secondary(red, blue, hue=(0, -60, 10))


def test_pull_without_a_device_gives_an_empty_window_and_says_why():
    """In a child process that sees no GPU: pulled as f16 and as f32."""
    script = r"""
import sys
sys.path.insert(0, %r)
from fluggo.media import process, basetypes, grade
window = basetypes.box2i(0, 0, 31, 17)
red = process.SolidColorVideoSource((1, 0, 0, 1))
for node in (process.VideoQualifierFilter(red, hue=(0, 60, 10)), process.VideoQualifierFilter(red, luma=(0, 1, 0, 0), key_source=red),
             process.VideoMatteMixFilter(red, red, red), grade.secondary(red, red, hue=(0, 60, 10), choke=1)):
    assert node.get_frame_f16(0, window).current_window.empty()
    assert node.get_frame_f32(0, window).current_window.empty()
    assert process.last_error(), "no message"
print("message:", process.last_error())
""" % ROOT
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    p = subprocess.run([os.sys.executable, "-c", script], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout
    assert "message:" in p.stdout and re.search(r"device|HIP|hip", p.stdout), p.stdout
