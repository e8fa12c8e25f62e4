"""The 3D LUT without a GPU (DESIGN.md "3D LUT"): the numpy model the GPU tests hold the kernel to (tests/lut3d_model.py) against
a float64 evaluation of the same tetrahedron and against a pixel-by-pixel restatement in Python; what follows from the contract
(identity on every half code in [0, 1], lattice points exact, the order of ties, clamping of what lies outside the domain and of
NaN and Inf); include/canvas_lut3d.h against the library and its bindings; every refusal of the two device entries, of the packer
and of cvs_lut3d_bytes, each with its message; fluggo.media.cube; the argument errors of Lut3D and VideoLut3DFilter; the built
code object."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from tests import lut3d_model as lm
from tests.models import f2h_rz_model
from tests.test_unsharp_cpu import _kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
POW2_SIZES = (2, 3, 5, 9, 17, 33, 65)            # N - 1 a power of two: t is exact for every half in [0, 1]
ONE = 0x3C00                                     # the half code of 1.0: codes 0 .. ONE are the halfs in [0, 1]


@pytest.fixture(scope="module")
def process():
    from fluggo.media import process
    return process


@pytest.fixture(scope="module")
def lib():
    from canvas_amd import _lib
    return _lib.load()


# ---------------------------------------------------------------- the model

def _by_loops(s, lat, domain):
    """The contract pixel by pixel, with Python's stable sort for the order: independent of the model's array code."""
    n = lat.shape[0]
    out = np.array(s, F32, copy=True)
    flat = out.reshape(-1, out.shape[-1])
    scale = [F32(F32(n - 1) / F32(F32(domain[1][c]) - F32(domain[0][c]))) for c in range(3)]
    with np.errstate(all="ignore"):
        for px in flat:
            i, f = [0, 0, 0], [F32(0)] * 3
            for c in range(3):
                t = F32(F32(px[c] - F32(domain[0][c])) * scale[c])
                t = (t if t < F32(n - 1) else F32(n - 1)) if t > 0 else F32(0)
                i[c] = min(int(t), n - 2)
                f[c] = F32(t - F32(i[c]))
            order = sorted(range(3), key=lambda c: (-float(f[c]), c))
            at = list(i)
            verts = [lat[at[2], at[1], at[0]]]
            for c in order:
                at[c] += 1
                verts.append(lat[at[2], at[1], at[0]])
            f1, f2, f3 = (f[c] for c in order)
            w = [F32(F32(1) - f1), F32(f1 - f2), F32(f2 - f3), f3]
            for c in range(3):
                acc = F32(F32(verts[0][c] * w[0]) + F32(verts[1][c] * w[1]))
                acc = F32(acc + F32(verts[2][c] * w[2]))
                px[c] = F32(acc + F32(verts[3][c] * w[3]))
    return out


def _tie_frames(size, rows=3):
    """f32 frames on which the order is decided by the tie rule: greys, two equal fractions in each pairing with the third above
    and below, and colours exactly on lattice planes (fractions of 0)."""
    rng = np.random.default_rng(size)
    n = 40
    v = rng.uniform(0, 1, n).astype(F32)
    u = rng.uniform(0, 1, n).astype(F32)
    step = F32(1.0) / F32(size - 1)
    cellbase = (rng.integers(0, size - 1, (n, 3)).astype(F32) * step).astype(F32)
    frac = (v * step).astype(F32)
    frac2 = (u * step).astype(F32)
    frames = [np.stack([v, v, v], -1)]                                                      # greys
    for a, b, c in ((0, 1, 2), (0, 2, 1), (1, 2, 0)):
        px = np.zeros((n, 3), F32)
        px[:, a] = frac; px[:, b] = frac; px[:, c] = frac2                                  # the same cell: equal fractions exactly
        frames.append(px)
        frames.append((px + cellbase[:, :1]).astype(F32))
    frames.append(cellbase)                                                                 # on lattice points: all fractions 0
    onplane = cellbase.copy(); onplane[:, 1] = (onplane[:, 1] + frac).astype(F32)
    frames.append(onplane)
    rgb = np.concatenate(frames)
    out = np.ones((rows, len(rgb), 4), F32)
    out[..., :3] = rgb[None]
    out[..., 3] = rng.uniform(0, 1, (rows, len(rgb))).astype(F32)
    return out


def test_the_model_is_the_contract_pixel_by_pixel():
    rng = np.random.default_rng(1)
    for size, domain in ((2, lm.UNIT), (3, lm.UNIT), (4, ((-0.25, 0.0, 0.1), (1.5, 2.0, 0.9))), (10, lm.UNIT), (17, ((0.0, 0.0, 0.0), (1.0, 0.5, 2.0)))):
        lat = lm.distinct(size, size)
        s = rng.uniform(-0.3, 1.3, (5, 60, 4)).astype(F32)
        s[0, :6, 0] = [np.nan, np.inf, -np.inf, 0.0, 1.0, -0.0]
        for frame in (s, _tie_frames(size, 1)):
            got, want = lm.apply_f32(frame, lat, domain), _by_loops(frame, lat, domain)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (size, domain)


@pytest.mark.parametrize("size", [2, 3, 5, 17, 33])
def test_the_model_against_float64(size):
    """Half inputs on the domain [0, 1] with N - 1 a power of two: t, i and f are exact, and so are 1 - f1, f1 - f2 and f2 - f3
    to within one rounding each; the sum is then four products and three adds of values below 2: at most 11 roundings, each at
    most 2^-24 relative of a value below 2, so 16 * 2^-24 bounds the error with room."""
    rng = np.random.default_rng(size)
    codes = rng.integers(0, ONE + 1, (64, 64, 4), dtype=np.uint16)
    s = lm.widen(codes)
    lat = rng.uniform(-0.5, 1.5, (size, size, size, 3)).astype(F32)
    got = lm.apply_f32(s, lat).astype(np.float64)[..., :3]
    want = lm.apply_f64(s, lat)
    worst = float(np.abs(got - want).max())
    print("N = %d: largest error against float64 %.3g (bound %.3g)" % (size, worst, 16 * 2.0 ** -24))
    assert worst <= 16 * 2.0 ** -24


@pytest.mark.parametrize("size", POW2_SIZES)
def test_identity_lattice_is_the_identity_on_every_half_code_in_0_1(size):
    codes = np.arange(ONE + 1, dtype=np.uint16)
    rng = np.random.default_rng(size)
    px = np.stack([codes, rng.permutation(codes), rng.permutation(codes), rng.permutation(codes)], -1)[None]
    lat = lm.identity(size)
    assert np.array_equal(lm.apply_pixels(px, lat), px)
    s = lm.widen(px)
    assert np.array_equal(lm.apply_f32(s, lat).view(np.uint32), s.view(np.uint32))


def test_identity_is_not_promised_for_other_sizes():
    """N = 10 and N = 32: some triples come out one code lower in a channel (never more, never higher), which is why the docs
    promise the identity for N - 1 a power of two only."""
    px = np.random.default_rng(0).integers(0, ONE + 1, (1, 50000, 4), dtype=np.uint16)
    for size in (10, 32):
        out = lm.apply_pixels(px, lm.identity(size))
        diff = px[..., :3].astype(np.int32) - out[..., :3].astype(np.int32)
        assert diff.min() == 0 and diff.max() == 1, size


@pytest.mark.parametrize("size", [2, 3, 4, 10, 17, 65])
def test_lattice_points_are_exact(size):
    """A colour on a lattice point gives that node's value exactly: on [0, 1] where N - 1 is a power of two, and for any N on the
    domain [0, N - 1], where scale is 1."""
    lat = lm.distinct(size, 3)
    rng = np.random.default_rng(size)
    idx = rng.integers(0, size, (1, 500, 3))
    idx[0, :4] = [[0, 0, 0], [size - 1] * 3, [size - 1, 0, size - 1], [0, size - 1, 0]]
    want = lat[idx[..., 2], idx[..., 1], idx[..., 0]]
    domains = [((0.0, 0.0, 0.0), (float(size - 1),) * 3)] + ([lm.UNIT] if size in POW2_SIZES else [])
    for domain in domains:
        s = np.ones(idx.shape[:2] + (4,), F32)
        s[..., :3] = idx.astype(F32) * F32(domain[1][0] / (size - 1))
        got = lm.apply_f32(s, lat, domain)
        assert np.array_equal(got[..., :3].view(np.uint32), want.view(np.uint32)), domain


def test_ties_take_r_before_g_before_b():
    """On a lattice whose every node is distinct a wrong vertex or a wrong order shows; here against explicit statements."""
    lat = lm.distinct(3, 9)
    L = lambda ir, ig, ib: lat[ib, ig, ir].astype(F32)
    def one(r, g, b):
        return lm.apply_f32(np.array([[[r, g, b, 1.0]]], F32), lat)[0, 0, :3]
    def blend(vs, ws):
        acc = (vs[0] * F32(ws[0])).astype(F32) + (vs[1] * F32(ws[1])).astype(F32)
        acc = (acc.astype(F32) + (vs[2] * F32(ws[2])).astype(F32)).astype(F32)
        return (acc + (vs[3] * F32(ws[3])).astype(F32)).astype(F32)
    # grey 0.25: cell 0, all fractions 0.5 -> order r, g, b
    assert np.array_equal(one(0.25, 0.25, 0.25), blend([L(0, 0, 0), L(1, 0, 0), L(1, 1, 0), L(1, 1, 1)], [0.5, 0.0, 0.0, 0.5]))
    # g == b above r: g first, then b, then r
    assert np.array_equal(one(0.125, 0.375, 0.375), blend([L(0, 0, 0), L(0, 1, 0), L(0, 1, 1), L(1, 1, 1)], [0.25, 0.0, 0.5, 0.25]))
    # r == b below g: g, then r before b
    assert np.array_equal(one(0.125, 0.375, 0.125), blend([L(0, 0, 0), L(0, 1, 0), L(1, 1, 0), L(1, 1, 1)], [0.25, 0.5, 0.0, 0.25]))
    # r == g below b: b, then r before g
    assert np.array_equal(one(0.125, 0.125, 0.375), blend([L(0, 0, 0), L(0, 0, 1), L(1, 0, 1), L(1, 1, 1)], [0.25, 0.5, 0.0, 0.25]))
    # the top corner: cell N - 2 with all fractions 1
    assert np.array_equal(one(1.0, 1.0, 1.0), L(2, 2, 2))
    # the tie frames really hold ties, in every pairing
    i, f = lm.cell(_tie_frames(5), 5)
    for a, b in ((0, 1), (0, 2), (1, 2)):
        assert ((f[..., a] == f[..., b]) & (f[..., a] > 0)).any()
    assert (f == 0).all(axis=-1).any()


def test_clamp_nan_and_inf():
    lat = lm.distinct(5, 4)
    domain = ((0.0, -1.0, 0.5), (1.0, 1.0, 4.0))
    lo, hi = domain
    def one(rgb):
        return lm.apply_f32(np.array([[list(rgb) + [0.5]]], F32), lat, domain)[0, 0, :3]
    inside = [0.25, 0.5, 2.0]
    for c in range(3):
        at_lo, at_hi = list(inside), list(inside)
        at_lo[c], at_hi[c] = lo[c], hi[c]
        for bad, same in ((np.nan, at_lo), (-np.inf, at_lo), (lo[c] - 3.0, at_lo), (-3e38, at_lo), (np.inf, at_hi), (hi[c] + 7.0, at_hi), (3e38, at_hi)):
            s = list(inside)
            s[c] = bad
            assert np.array_equal(one(s), one(same)), (c, bad)
    assert np.array_equal(one([np.nan] * 3), lat[0, 0, 0]) and np.array_equal(one([np.inf] * 3), lat[4, 4, 4])
    # alpha passes code for code, NaN payloads and signalling NaNs included
    px = np.array([[[0x3800, 0x3400, 0x3000, a] for a in (0x7C01, 0xFE00, 0x7C00, 0x8000, 0x0001, 0xFBFF)]], np.uint16)
    assert np.array_equal(lm.apply_pixels(px, lat)[..., 3], px[..., 3])
    s = lm.widen(px); s.view(np.uint32)[0, 0, 3] = 0x7F800001
    assert np.array_equal(lm.apply_f32(s, lat)[..., 3].view(np.uint32), s[..., 3].view(np.uint32))
    # f16 results are truncated, not rounded
    flat = np.full((2, 2, 2, 3), 0.1, F32)
    assert lm.apply_pixels(px, flat)[0, 0, 0] == f2h_rz_model(np.array([0.1], F32))[0] == 0x2E66


def test_expected_windows():
    lat = lm.identity(3)
    src = np.zeros((4, 6, 4), np.uint16)
    before = np.full((4, 6, 4), 7, np.uint16)
    out, win = lm.expected(before, (2, 1, 7, 4), src, (0, 0, 5, 3), (1, 0, 5, 3), lat)
    assert win == (2, 1, 5, 3) and (out[:3, :4] == 0).all() and (out[3] == 7).all() and (out[:, 4:] == 7).all()
    assert lm.expected(before, (2, 1, 7, 4), src, (0, 0, 5, 3), None, lat)[1] is None
    assert lm.expected(before, (20, 1, 25, 4), src, (0, 0, 5, 3), (0, 0, 5, 3), lat)[1] is None


# ---------------------------------------------------------------- the C surface

FIELDS = ["size", "domain_min", "domain_max", "flags"]


def test_struct_mirror_has_the_c_layout():
    """sizeof, every offset and the constants, from a probe compiled against the header."""
    from canvas_amd import _lib
    assert [name for name, _ in _lib.lut3d_params._fields_] == FIELDS
    probe = ('#include <stddef.h>\n#include <stdio.h>\n#include "canvas_lut3d.h"\nint main(void) {\n    printf("%zu", sizeof(cvs_lut3d));\n'
             + "".join('    printf(" %%zu", offsetof(cvs_lut3d, %s));\n' % f for f in FIELDS)
             + '    printf(" %d %d\\n", CVS_LUT3D_MIN_SIZE, CVS_LUT3D_MAX_SIZE);\n    return 0;\n}\n')
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "probe.c"), os.path.join(tmp, "probe")
        with open(src, "w") as f:
            f.write(probe)
        subprocess.run(["gcc", "-std=gnu11", "-I" + os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout.split()]
    want = [C.sizeof(_lib.lut3d_params)] + [getattr(_lib.lut3d_params, f).offset for f in FIELDS] + [_lib.LUT3D_MIN_SIZE, _lib.LUT3D_MAX_SIZE]
    assert got == want and got[0] == 32 and got[-2:] == [2, 65]
    p = _lib.lut3d(17, (0.0, -1.0, 0.5), (1.0, 2.0, 4.0))
    assert (p.size, list(p.domain_min), list(p.domain_max), p.flags) == (17, [0.0, -1.0, 0.5], [1.0, 2.0, 4.0], 0)
    P = C.POINTER
    assert _lib.LUT3D_SIGNATURES == {
        "cvs_lut3d_bytes": (C.c_size_t, [C.c_int]),
        "cvs_lut3d_pack": (C.c_int, [P(C.c_float), P(C.c_float), C.c_int]),
        "cvs_lut3d_f16_dev": (C.c_int, [P(_lib.rgba_frame_f16), P(_lib.rgba_frame_f16), C.c_void_p, P(_lib.lut3d_params), C.c_void_p]),
        "cvs_lut3d_f32_dev": (C.c_int, [P(_lib.rgba_frame_f32), P(_lib.rgba_frame_f32), C.c_void_p, P(_lib.lut3d_params), C.c_void_p]),
    }


def _declared(header):
    """(every function include/<header> declares with CVS_EXPORT, its cvs_*_dev functions whose last parameter is a cvs_stream_t)"""
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    text = "\n".join(l for l in text.splitlines() if not l.lstrip().startswith("#"))
    funcs = sorted(set(re.findall(r"CVS_EXPORT\s+[^;(]*?\b(\w+)\s*\(", text)))
    entries = [name for name, params in re.findall(r"CVS_EXPORT\s+int\s+(cvs_\w+_dev)\s*\(([^;{]*?)\)\s*;", text, flags=re.S)
               if params.split(",")[-1].split()[0] == "cvs_stream_t"]
    return funcs, sorted(entries)


def test_every_symbol_of_the_header_is_exported_and_bound(lib):
    """What tests/test_abi_cpu.py holds canvas_hip.h to, for include/canvas_lut3d.h and its own table of bindings."""
    from canvas_amd import _lib
    funcs, entries = _declared("canvas_lut3d.h")
    assert funcs == sorted(_lib.LUT3D_SIGNATURES) and len(funcs) == 4
    assert entries == ["cvs_lut3d_f16_dev", "cvs_lut3d_f32_dev"]
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert not [f for f in funcs if f not in exported]
    assert not set(_lib.LUT3D_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.SCOPE_SIGNATURES))
    for name in funcs:
        assert getattr(lib, name).argtypes == _lib.LUT3D_SIGNATURES[name][1] and getattr(lib, name).restype is _lib.LUT3D_SIGNATURES[name][0], name
    for name in entries:
        assert _lib.LUT3D_SIGNATURES[name][1][-1] is C.c_void_p, name
    # one launcher, one arithmetic flavour
    symbols = subprocess.run(["nm", _lib.LIB_PATH], stdout=subprocess.PIPE, text=True).stdout
    assert re.search(r"\bcvk_lut3d\b", symbols) and not re.search(r"\bcvk_lut3d_fma\b", symbols)
    # the header compiles as C and as C++ on its own
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "t.c")
        with open(src, "w") as f:
            f.write('#include "canvas_lut3d.h"\nint main(void) { cvs_lut3d p; p.size = CVS_LUT3D_MAX_SIZE; p.flags = 0; return sizeof p == 32 && p.size == 65 ? 0 : 1; }\n')
        for cc, std, lang in (("gcc", "-std=c99", "c"), ("g++", "-std=c++14", "c++")):
            exe = os.path.join(tmp, "t_" + cc)
            subprocess.run([cc, std, "-Wall", "-Werror", "-x", lang, src, "-I", os.path.join(ROOT, "include"), "-o", exe], check=True)
            assert subprocess.run([exe]).returncode == 0


def test_bytes_and_pack(lib):
    from canvas_amd import _lib
    for size in (2, 3, 17, 33, 65):
        assert lib.cvs_lut3d_bytes(size) == 16 * size ** 3
    for size in (1, 0, -1, 66, 2 ** 30):
        lib.cvs_clear_last_error()
        assert lib.cvs_lut3d_bytes(size) == 0
        assert "cvs_lut3d_bytes" in _lib.last_error() and "outside 2..65" in _lib.last_error()
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    for size in (2, 5):
        lat = lm.distinct(size, 1)
        rgb = np.ascontiguousarray(lat.reshape(-1))
        out = np.full(size ** 3 * 4 + 8, 7.0, F32)
        assert lib.cvs_lut3d_pack(fp(out[4:]), fp(rgb), size) == 0
        assert np.array_equal(out[4:-4], lm.packed(lat)) and (out[:4] == 7).all() and (out[-4:] == 7).all()
        for bad in (np.nan, np.inf, -np.inf):
            for at in (0, 3 * size ** 3 - 1, 7):
                poisoned = rgb.copy()
                poisoned[at] = bad
                lib.cvs_clear_last_error()
                assert lib.cvs_lut3d_pack(fp(out[4:]), fp(poisoned), size) == -1
                assert "cvs_lut3d_pack" in _lib.last_error() and "not finite" in _lib.last_error() and "value %d " % at in _lib.last_error()
    rgb, out = np.zeros(24, F32), np.zeros(32, F32)
    for size in (1, 66, -3):
        lib.cvs_clear_last_error()
        assert lib.cvs_lut3d_pack(fp(out), fp(rgb), size) == -1 and "outside 2..65" in _lib.last_error()
    lib.cvs_clear_last_error()
    assert lib.cvs_lut3d_pack(None, fp(rgb), 2) == -1 and "need" in _lib.last_error()
    assert lib.cvs_lut3d_pack(fp(out), None, 2) == -1


def test_entries_refuse_before_anything_is_launched(lib):
    from canvas_amd import _lib
    from canvas_amd.abi import HostFrame
    full = (0, 0, 7, 7)
    lim = _lib.MAX_COORD
    nan, inf = float("nan"), float("inf")
    raw = np.zeros(8 * 4 + 8, F32)
    lattice = raw.ctypes.data + (-raw.ctypes.data % 16)
    for name, dtype, frame_t in (("cvs_lut3d_f16_dev", np.uint16, _lib.rgba_frame_f16), ("cvs_lut3d_f32_dev", np.float32, _lib.rgba_frame_f32)):
        entry = getattr(lib, name)

        def refused(target, source, lat, p, word):
            lib.cvs_clear_last_error()
            assert entry(target, source, lat, p, None) == -1, (name, word)
            assert name in _lib.last_error() and word in _lib.last_error(), (name, word, _lib.last_error())

        def fresh():
            return HostFrame(full, dtype, current_window=full)
        good, ok = fresh(), _lib.lut3d(2)
        cases = [(None, ok, "need"), (lattice, None, "need")]
        cases += [(lattice + off, ok, "16-byte") for off in (4, 8, 12, 1)]
        cases += [(lattice, _lib.lut3d(size), "outside 2..65") for size in (1, 0, -5, 66, 1000)]
        cases += [(lattice, _lib.lut3d(2, lo, hi), "finite and ascending") for lo, hi in (
            ((0, 0, 0), (1, 1, 0)), ((0, 0.5, 0), (1, 0.5, 1)), ((2, 0, 0), (1, 1, 1)), ((nan, 0, 0), (1, 1, 1)), ((0, 0, 0), (1, nan, 1)),
            ((0, 0, -inf), (1, 1, 1)), ((0, 0, 0), (inf, 1, 1)))]
        cases += [(lattice, _lib.lut3d(2, flags=flags), "unknown flags") for flags in (1, 2, -1, 0x100)]
        for lat, p, word in cases:
            out = fresh()
            refused(out.ref(), good.ref(), lat, None if p is None else C.byref(p), word)
            assert out.current_window.is_empty(), word
        out = fresh()
        refused(out.ref(), None, lattice, C.byref(ok), "need")
        assert out.current_window.is_empty()
        refused(None, good.ref(), lattice, C.byref(ok), "need")
        out, outside = fresh(), HostFrame(full, dtype, current_window=(0, 0, 8, 7))
        refused(out.ref(), outside.ref(), lattice, C.byref(ok), "outside its buffer")
        assert out.current_window.is_empty()
        # coordinates beyond the bound: frames that describe buffers nobody allocates (nothing is dereferenced)
        box = _lib.box2i.of
        far = frame_t(good.c.data, box(lim - 6, 0, lim + 1, 7), box(lim - 6, 0, lim + 1, 7))
        out = fresh()
        refused(out.ref(), C.byref(far), lattice, C.byref(ok), "beyond")
        assert out.current_window.is_empty()
        far = frame_t(good.c.data, box(0, -lim - 1, 7, -lim + 6), box(0, 0, 7, 7))
        refused(C.byref(far), good.ref(), lattice, C.byref(ok), "beyond")
        assert far.current_window.is_empty() and good.current_window.tuple() == full       # a refused call leaves its source alone
        # in place: the one frame's window is emptied by a refusal
        both = fresh()
        refused(both.ref(), both.ref(), lattice, C.byref(_lib.lut3d(99)), "outside 2..65")
        assert both.current_window.is_empty()
        if lib.cvs_device_count() == 0:
            # without a device a call that nothing refuses still fails, loudly, and computes nothing on the CPU
            lib.cvs_clear_last_error()
            out = fresh()
            assert entry(out.ref(), good.ref(), lattice, C.byref(ok), None) != 0 and "no CPU path" in _lib.last_error()
            assert out.current_window.is_empty()


def test_code_object_holds_every_instance_without_scratch():
    """One build for both arithmetic flavours; two kernels (the lattice through the caches, the lattice staged in LDS) x three
    pixel layouts (f32, f16 one pixel per lane, f16 pairs); no private segment, no spills, and no register read between a load
    into it and the wait that retires it."""
    assert os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"), "the ROCm LLVM tools the build itself needs are missing"
    found = _kernels("lut3d_ops.hip.o")
    assert len(found) == 6 and all("k_lut3d" in n for n in found), sorted(found)
    for half in (0, 1, 2):
        assert any("k_lut3dILi%dEEE" % half in n for n in found) and any("k_lut3d_ldsILi%dEEE" % half in n for n in found), half
    for name, (scratch, spills) in found.items():
        assert scratch == 0 and spills == 0, (name, scratch, spills)
    assert not os.path.exists(os.path.join(ROOT, "canvas_amd", "csrc", "build", "lut3d_ops.fma.hip.o"))
    spec = __import__("importlib.util").util.spec_from_file_location("check_asm_loads", os.path.join(ROOT, "tools", "check_asm_loads.py"))
    chk = __import__("importlib.util").util.module_from_spec(spec)
    spec.loader.exec_module(chk)
    checked, problems = chk.check_paths([os.path.join(ROOT, "canvas_amd", "csrc", "build", "lut3d_ops.hip.o")])
    assert checked >= 6 and not problems, problems[:5]


# ---------------------------------------------------------------- fluggo.media.cube

def test_read_cube_and_round_trip(tmp_path):
    from fluggo.media import cube
    rows = ["%r %r %r" % (0.125 * k, 1.0 - 0.1 * k, -0.5 + k) for k in range(8)]
    text = "# a look\nTITLE \"two by two\"\n\nLUT_3D_SIZE 2\nDOMAIN_MIN 0 -1 0\nDOMAIN_MAX 1.0 2.0 4.0\n" + "\n".join(rows) + "\n\n"
    size, table, lo, hi = cube.read_cube(text)
    assert (size, lo, hi) == (2, (0.0, -1.0, 0.0), (1.0, 2.0, 4.0))
    assert table == [v for k in range(8) for v in (0.125 * k, 1.0 - 0.1 * k, -0.5 + k)]
    assert cube.parse_cube(text)[4] == "two by two"
    path = tmp_path / "look.cube"
    path.write_text(text)
    assert cube.read_cube(str(path)) == (size, table, lo, hi) and cube.read_cube(path) == (size, table, lo, hi)
    # defaults, and a round trip through write_cube of numbers that have no short decimal form
    rng = np.random.default_rng(2)
    values = [float(v) for v in rng.uniform(-1, 2, 81).astype(np.float32)]
    again = cube.read_cube(cube.write_cube(3, values, title="t"))
    assert again == (3, values, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    again = cube.read_cube(cube.write_cube(3, values, (0.0, 0.1, 0.2), (1.0, 1.1, 1.3)))
    assert again == (3, values, (0.0, 0.1, 0.2), (1.0, 1.1, 1.3))
    assert cube.read_cube("LUT_3D_SIZE 2\n" + "0 0 0\n" * 8)[2:] == ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))


def test_read_cube_refusals_name_the_line():
    from fluggo.media import cube
    head = "TITLE \"t\"\nLUT_3D_SIZE 2\n"
    row = "0 0 0\n"
    for text, line, word in [
            ("LUT_1D_SIZE 16\n" + row * 16, 1, "LUT_1D_SIZE"),
            ("# c\n\nLUT_1D_SIZE 16\n", 3, "LUT_1D_SIZE"),
            (head + row * 7, 9, "7 rows"),
            (head + row * 9, 11, "more than"),
            (head + row * 3 + "0 nan 0\n" + row * 4, 6, "not finite"),
            (head + row * 3 + "inf 0 0\n" + row * 4, 6, "not finite"),
            (head + "DOMAIN_MAX 1 -inf 1\n" + row * 8, 3, "not finite"),
            (head + row + "0 0\n", 4, "3 numbers"),
            (head + row + "0 0 zero\n", 4, "not a number"),
            (row * 8, 1, "before LUT_3D_SIZE"),
            ("TITLE \"t\"\n", 1, "no LUT_3D_SIZE"),
            ("LUT_3D_SIZE 1\n", 1, "outside 2..65"),
            ("LUT_3D_SIZE 66\n", 1, "outside 2..65"),
            ("LUT_3D_SIZE two\n", 1, "whole number"),
            (head + "LUT_3D_SIZE 2\n", 3, "twice"),
            (head + "LUT_3D_INPUT_RANGE 0 1\n" + row * 8, 3, "unknown keyword"),
            (head + "DOMAIN_MIN 0 1 0\n" + row * 8, 11, "not below"),
    ]:
        with pytest.raises(cube.CubeError) as e:
            cube.read_cube(text)
        assert isinstance(e.value, ValueError)
        assert str(e.value).startswith("line %d:" % line) and word in str(e.value), (text[:40], str(e.value))


def test_lattices_from_functions(process):
    from fluggo.media import cube
    for size in (2, 5, 17):
        got = cube.identity_lattice(size)
        assert got[0] == size and got[2:] == ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
        assert np.array_equal(lm.lattice(got[1], size), lm.identity(size))
    # a CDL (slope, offset; power 1) and a saturation change, baked and applied: the lattice points hold the function's values
    lo, hi = (0.0, 0.0, -1.0), (1.0, 2.0, 1.0)
    fn = lambda r, g, b: (1.5 * r + 0.1, 0.5 * g - 0.25, b * b)
    size, table, dmin, dmax = cube.lattice_from_function(fn, 4, lo, hi)
    assert (size, dmin, dmax) == (4, lo, hi) and len(table) == 192
    lat = lm.lattice(table, 4)
    assert lat[3, 0, 0].tolist() == [F32(0.1), F32(-0.25), F32(1.0)] and lat[0, 3, 3].tolist() == [F32(1.6), F32(0.75), F32(1.0)]
    assert lat[1, 2, 3].tolist() == [F32(1.6), F32(0.5 * (4.0 / 3.0) - 0.25), F32((-1.0 + 2.0 / 3.0) ** 2)]
    lut = process.Lut3D(*cube.lattice_from_function(fn, 4, lo, hi))
    assert np.array_equal(np.frombuffer(lut.table, F32), lat.reshape(-1))
    for bad in (1, 66):
        with pytest.raises(ValueError):
            cube.identity_lattice(bad)
    with pytest.raises(ValueError):
        cube.lattice_from_function(lambda r, g, b: (r, g), 2)


# ---------------------------------------------------------------- the Python surface

def test_lut3d_value(process):
    cls = process.Lut3D
    table = [float(v) for v in lm.distinct(3, 2).reshape(-1)]
    lut = cls(3, table)
    assert (lut.size, lut.domain_min, lut.domain_max) == (3, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    assert np.array_equal(np.frombuffer(lut.table, F32), np.array(table, F32))
    for form in (np.array(table, F32), np.array(table, np.float64), np.array(table, F32).reshape(27, 3), tuple(table), np.array(table, F32).tobytes() and memoryview(np.array(table, F32))):
        assert cls(3, form).table == lut.table
    lut = cls(size=2, table=[0.5] * 24, domain_min=(0.0, -1.0, 0.25), domain_max=(1.0, 2.0, 4.0))
    assert (lut.domain_min, lut.domain_max) == ((0.0, -1.0, 0.25), (1.0, 2.0, 4.0))
    for name in ("size", "table", "domain_min", "domain_max"):
        with pytest.raises(AttributeError):
            setattr(lut, name, getattr(lut, name))
    with pytest.raises(TypeError):
        lut.__init__(2, [0.0] * 24)                                   # immutable
    nan, inf = float("nan"), float("inf")
    for args, kw, word in [((1, []), {}, "outside 2..65"), ((66, [0.0] * 3), {}, "outside 2..65"), ((2, [0.0] * 23), {}, "24"), ((2, [0.0] * 25), {}, "24"),
                           ((2, np.zeros(23, F32)), {}, "24"), ((2, [0.0] * 23 + [nan]), {}, "not finite"), ((2, np.full(24, inf)), {}, "not finite"),
                           ((2, [0.0] * 24), dict(domain_min=(0, 0, 1)), "ascending"), ((2, [0.0] * 24), dict(domain_max=(1, nan, 1)), "ascending"),
                           ((2, [0.0] * 24), dict(domain_min=(-inf, 0, 0)), "ascending")]:
        with pytest.raises(ValueError) as e:
            cls(*args, **kw)
        assert word in str(e.value), (args[0], kw, str(e.value))
    for args, kw in [((), {}), ((2,), {}), (("two", [0.0] * 24), {}), ((2, ["a"] * 24), {}), ((2, 5), {}), ((2, [0.0] * 24), dict(domain_min=(0, 0))),
                     ((2, [0.0] * 24), dict(domain_max="abc")), ((2, [0.0] * 24, (0, 0, 0), (1, 1, 1), 0), {})]:
        with pytest.raises(TypeError):
            cls(*args, **kw)


def test_node_arguments_and_properties(process):
    cls = process.VideoLut3DFilter
    assert issubclass(cls, process.VideoSource)
    red = process.SolidColorVideoSource((1.0, 0.0, 0.0, 1.0))
    lut, other = process.Lut3D(2, [0.0] * 24), process.Lut3D(3, [1.0] * 81)
    node = cls(red, lut)
    assert node.source is red and node.lut is lut
    node = cls(source=None, lut=lut)
    assert node.source is None
    node.lut = other
    assert node.lut is other
    node.source = red
    assert node.source is red
    for bad in (None, 3, "look", (2, [0.0] * 24), red):
        with pytest.raises(TypeError):
            node.lut = bad
        assert node.lut is other                                      # a refused value leaves the old one
        with pytest.raises(TypeError):
            cls(red, bad)
    with pytest.raises(TypeError):
        del node.lut
    for bad in (object(), 3, "source"):
        with pytest.raises(Exception):
            cls(bad, lut)
        with pytest.raises(Exception):
            node.set_source(bad)
    with pytest.raises(TypeError):
        cls(red)
    with pytest.raises(TypeError):
        cls()
    node.set_source(None)
    assert node.source is None


def test_pull_without_a_device_gives_an_empty_window_and_says_why():
    """In a child process that sees no GPU: pulled as f16 and as f32, with and without a source."""
    script = r"""
import sys
sys.path.insert(0, %r)
from fluggo.media import process, basetypes, cube
window = basetypes.box2i(0, 0, 31, 17)
red = process.SolidColorVideoSource((1, 0, 0, 1))
lut = process.Lut3D(*cube.identity_lattice(3))
for source in (red, None):
    node = process.VideoLut3DFilter(source, lut)
    assert node.get_frame_f16(0, window).current_window.empty()
    assert node.get_frame_f32(0, window).current_window.empty()
    node.lut = process.Lut3D(*cube.identity_lattice(2))
    assert process.last_error(), "no message"
print("message:", process.last_error())
""" % ROOT
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    p = subprocess.run([os.sys.executable, "-c", script], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout
    assert "message:" in p.stdout and re.search(r"device|HIP|hip", p.stdout), p.stdout


def test_every_device_entry_of_the_header_has_its_catalogue_cases():
    """What tests/test_entry_cases_cpu.py holds tests/entry_cases.py to, for tests/lut3d_cases.py: every cvs_*_dev entry the
    header declares is CALLED by a case, each call is handed the factory's stream, every case has an output and asks for the same
    operands every time, and the Shifted factory moves every frame and changes no buffer, so the far-window harness runs the
    cases as it runs the catalogue's."""
    from tests import entry_cases as ec
    from tests import lut3d_cases as lc
    from tests.test_entry_cases_cpu import Geometry, HostOnly, Recorder, _check_shifted
    _funcs, entries = _declared("canvas_lut3d.h")
    assert entries == sorted(lc.ENTRIES)
    seen, stream, cases = {}, 0x5EED, 0
    for gid, build in lc.GROUPS:
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
            lattice = [o for o in fac.objects if o.frame is None]
            assert len(lattice) == 1 and lattice[0].cls == "f32" and not lattice[0].out and lattice[0].nbytes in (16 * 4 ** 3, 16 * 5 ** 3, 16 * 17 ** 3)
            again = HostOnly(rec, stream)
            case(again)
            spec = lambda f: [(o.cls, o.name, o.out, o.cmp, o.nbytes, o.row_bytes, o.reads) for o in f.objects]
            assert spec(fac) == spec(again), (gid, what)
            boxes = [(o.out, o.frame.c.full_window.tuple()) for o in fac.objects if o.frame is not None]
            assert len(ec.far_offsets(lc.FAR_RULE, boxes)) >= 4, (gid, what)
    assert sorted(seen) == entries and len(seen["cvs_lut3d_f16_dev"]) == len(seen["cvs_lut3d_f32_dev"]) + 3 and cases == sum(len(v) for v in seen.values())
    assert any("in place" in w for w in seen["cvs_lut3d_f32_dev"]) and any("all codes" in w for w in seen["cvs_lut3d_f16_dev"])
    frames = 0
    for gid, build in lc.GROUPS:
        a, b = Geometry(), Geometry()
        for (what, near), (_, far) in zip(build(a), build(b)):
            frames += _check_shifted(gid, what, (near, far, a, b), lc.FAR_RULE["source_scale"])
    assert frames == 2 * cases                                       # two frame arguments per call (in place: the one frame twice)
