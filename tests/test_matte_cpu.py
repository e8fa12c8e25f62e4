"""VideoMatteFilter without a GPU: the two C entries are declared, exported and mirrored, the ctypes struct has the C struct's
layout; every refusal of the contract (DESIGN.md "Matte refine") comes back as -1 with a message naming the entry and an empty
window before anything is launched; the node's surface; self-checks of the numpy model the GPU tests hold the kernel to
(tests/matte_model.py); the built code object holds the three k_matte_refine instances without scratch memory and passes the
load-in-flight check; a pull without a device or without a source ends with an empty window."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from tests import matte_model as mm
from tests.models import blur_model
from tests.test_unsharp_cpu import _kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("cvs_matte_refine_f32_dev", "cvs_matte_refine_f16_dev")


@pytest.fixture(scope="module")
def process():
    from fluggo.media import process
    return process


def test_entry_points_declared_exported_and_mirrored():
    header = open(os.path.join(ROOT, "include", "canvas_hip.h")).read()
    for fmt in ("f32", "f16"):
        decl = (r"CVS_EXPORT int cvs_matte_refine_%s_dev\(rgba_frame_%s \*target, const rgba_frame_%s \*source, const cvs_matte \*m, cvs_stream_t s\);"
                % (fmt, fmt, fmt))
        assert re.search(decl, header), decl
    assert re.search(r"enum \{ CVS_MATTE_SHOW = 1 \};", header)
    assert re.search(r"enum \{ CVS_MATTE_MAX_CHOKE = 16, CVS_MATTE_MAX_TAPS = 25 \};", header)
    from canvas_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for name, frame in (("cvs_matte_refine_f32_dev", _lib.rgba_frame_f32), ("cvs_matte_refine_f16_dev", _lib.rgba_frame_f16)):
        assert hasattr(raw, name) and name in _lib.SIGNATURES, name
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is C.c_int and argtypes == [C.POINTER(frame), C.POINTER(frame), C.POINTER(_lib.matte_params), C.c_void_p]
    assert (_lib.MATTE_SHOW, _lib.MATTE_MAX_CHOKE, _lib.MATTE_MAX_TAPS) == (1, 16, 25)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], stdout=subprocess.PIPE, text=True).stdout
    assert all(name in out for name in ENTRIES)
    symbols = subprocess.run(["nm", _lib.LIB_PATH], stdout=subprocess.PIPE, text=True).stdout
    assert re.search(r"\bcvk_matte_refine\b", symbols) and not re.search(r"\bcvk_matte_refine_fma\b", symbols)


def test_struct_mirror_has_the_c_layout():
    """sizeof and every offset, from a probe compiled against the header."""
    from canvas_amd import _lib
    fields = [name for name, _ in _lib.matte_params._fields_]
    assert fields == ["black", "white", "choke", "ntaps", "taps", "flags"]
    probe = ('#include <stddef.h>\n#include <stdio.h>\n#include "canvas_hip.h"\nint main(void) {\n    printf("%zu", sizeof(cvs_matte));\n'
             + "".join('    printf(" %%zu", offsetof(cvs_matte, %s));\n' % f for f in fields)
             + '    printf(" %d %d %d\\n", CVS_MATTE_SHOW, CVS_MATTE_MAX_CHOKE, CVS_MATTE_MAX_TAPS);\n    return 0;\n}\n')
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "probe.c"), os.path.join(tmp, "probe")
        with open(src, "w") as f:
            f.write(probe)
        subprocess.run(["gcc", "-std=gnu11", "-I" + os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout.split()]
    want = ([C.sizeof(_lib.matte_params)] + [getattr(_lib.matte_params, f).offset for f in fields]
            + [_lib.MATTE_SHOW, _lib.MATTE_MAX_CHOKE, _lib.MATTE_MAX_TAPS])
    assert got == want and got[0] == 32


def test_helper_builds_the_struct():
    from canvas_amd import _lib
    m = _lib.matte()
    assert (m.black, m.white, m.choke, m.ntaps, m.flags) == (0.0, 1.0, 0, 0, 0) and not m.taps
    m = _lib.matte(-3, [0.25, 0.5, 0.25], 0.125, 0.75, True)
    assert (m.black, m.white, m.choke, m.ntaps, m.flags) == (0.125, 0.75, -3, 3, _lib.MATTE_SHOW)
    assert [m.taps[k] for k in range(3)] == [0.25, 0.5, 0.25]


def test_entries_refuse_bad_arguments_before_any_launch():
    from canvas_amd import _lib
    from canvas_amd.abi import HostFrame
    lib = _lib.load()
    full = (0, 0, 7, 7)
    nan, inf = float("nan"), float("inf")

    def raw(ntaps, taps, **kw):
        """a struct the helper would not build: a tap count that disagrees with the list, no list, stray flag bits"""
        m = _lib.matte(**kw)
        m._taps = (C.c_float * len(taps))(*taps) if taps else None
        m.ntaps, m.taps = ntaps, C.cast(m._taps, C.POINTER(C.c_float)) if taps else None
        return m

    flagged = _lib.matte()
    flagged.flags = 2
    flagged_too = _lib.matte(show_matte=True)
    flagged_too.flags = 1 | 0x100
    bad = ([("choke", _lib.matte(choke=v)) for v in (17, -17, 40, -(1 << 31))]
           + [("taps", raw(n, t)) for n, t in ((-1, [1.0]), (2, [0.5, 0.5]), (4, [0.25] * 4), (27, [0.0] * 27), (26, [0.0] * 26), (3, None), (1, None))]
           + [("tap", _lib.matte(feather=t)) for t in ([nan], [0.25, inf, 0.25], [0.25, 0.5, -inf])]
           + [("white", _lib.matte(black=b, white=w)) for b, w in ((nan, 1.0), (0.0, nan), (inf, 1.0), (0.0, inf), (-inf, 0.0), (0.5, 0.5), (0.75, 0.25), (1.0, 0.0))]
           + [("flags", flagged), ("flags", flagged_too)])
    for name, dtype in ((ENTRIES[1], np.uint16), (ENTRIES[0], np.float32)):
        entry = getattr(lib, name)

        def refused(target, source, m, what):
            lib.cvs_clear_last_error()
            assert entry(target, source, m, None) == -1, what
            assert name in _lib.last_error(), (what, _lib.last_error())
        good = HostFrame(full, dtype, current_window=full)
        for word, m in bad:
            out = HostFrame(full, dtype, current_window=full)
            refused(out.ref(), good.ref(), C.byref(m), (word, m.choke, m.ntaps, m.black, m.white, m.flags))
            assert out.current_window.is_empty(), word
            assert word in _lib.last_error(), (word, _lib.last_error())
        out, outside = HostFrame(full, dtype, current_window=full), HostFrame(full, dtype, current_window=(0, 0, 8, 7))
        refused(out.ref(), outside.ref(), C.byref(_lib.matte()), "source window outside its buffer")
        assert out.current_window.is_empty() and "outside" in _lib.last_error()
        out = HostFrame(full, dtype, current_window=full)
        refused(out.ref(), None, C.byref(_lib.matte()), "NULL source")
        assert out.current_window.is_empty()
        out = HostFrame(full, dtype, current_window=full)
        refused(out.ref(), good.ref(), None, "NULL settings")
        assert out.current_window.is_empty()
        refused(None, good.ref(), C.byref(_lib.matte()), "NULL target")
        assert good.current_window.tuple() == full                   # a refused call leaves its source alone
        # not in place: the same buffer as target and source, through one frame struct and through two
        same = HostFrame(full, dtype, current_window=full)
        refused(same.ref(), same.ref(), C.byref(_lib.matte(choke=1)), "in place")
        assert same.current_window.is_empty() and "in place" in _lib.last_error()
        twin = HostFrame(full, dtype, good.array, full)
        twin.c.data = good.c.data
        refused(twin.ref(), good.ref(), C.byref(_lib.matte()), "in place, two structs")
        assert twin.current_window.is_empty() and good.current_window.tuple() == full


def test_node_surface(process):
    red = process.SolidColorVideoSource((1, 0, 0, 1))
    cls = process.VideoMatteFilter
    assert issubclass(cls, process.VideoSource)
    node = cls(red)
    cap = node._video_frame_source_funcs
    assert type(cap).__name__ == "PyCapsule" and '"_video_frame_source_funcs"' in repr(cap)
    assert node.source is red
    assert (node.choke, node.feather, node.black, node.white, node.show_matte) == (0, None, 0.0, 1.0, False)
    taps = process.gaussian_taps(1.0)
    node = cls(red, 2, taps, 0.125, 0.75, True)
    assert (node.choke, node.feather, node.black, node.white, node.show_matte) == (2, taps, 0.125, 0.75, True)
    node = cls(source=red, show_matte=True, white=0.5, black=0.25, feather=[1], choke=-3)
    assert (node.choke, node.feather, node.black, node.white, node.show_matte) == (-3, (1.0,), 0.25, 0.5, True)
    other = process.SolidColorVideoSource((0, 1, 0, 1))
    node.set_source(other)
    assert node.source is other
    node.source = red
    assert node.source is red
    node.set_source(None)
    assert node.source is None
    ramp = process.LerpFunc((0.0,), (2.0,), 3.0)
    for name, value in (("choke", 5), ("black", 0.375), ("white", 0.625)):
        setattr(node, name, value)
        assert getattr(node, name) == value
        setattr(node, name, ramp)
        assert getattr(node, name) is ramp
        for bad in ("much", None, object()):
            with pytest.raises(Exception):
                setattr(node, name, bad)
        assert getattr(node, name) is ramp                          # a refused value leaves the old one
        setattr(node, name, 1)
        assert getattr(node, name) == 1
    node.feather = (0.25, 0.5, 0.25)
    assert node.feather == (0.25, 0.5, 0.25)
    for bad in ("wide", 3, object(), (), (0.5, 0.5), [0.0] * 27, (0.25, "x", 0.25), (float("nan"),), (0.5, float("inf"), 0.5)):
        with pytest.raises(Exception):
            node.feather = bad
        assert node.feather == (0.25, 0.5, 0.25)
    node.feather = None
    assert node.feather is None
    node.feather = [0.04] * 25
    assert len(node.feather) == 25
    node.show_matte = False
    assert node.show_matte is False
    for bad in (1, "yes", None):
        with pytest.raises(TypeError):
            node.show_matte = bad
    for bad in (object(), 3, "source"):
        with pytest.raises(Exception):
            cls(bad)
        with pytest.raises(Exception):
            node.set_source(bad)
    with pytest.raises(TypeError):
        cls()
    for kw in (dict(choke="far"), dict(choke=None), dict(feather="soft"), dict(feather=(0.5, 0.5)), dict(black="low"), dict(white=None)):
        with pytest.raises(Exception):
            cls(red, **kw)


# ---------------------------------------------------------------- the model

def _planes():
    rng = np.random.default_rng(11)
    noise = rng.uniform(0, 1, (23, 31)).astype(np.float32)
    return [("noise", noise), ("disc", mm.soft_disc(40, 27)), ("column", noise[:, :1].copy()), ("row", noise[:1].copy()), ("pixel", noise[:1, :1].copy())]


def test_model_identity_zeroes_nan_alphas_only():
    rng = np.random.default_rng(2)
    for dtype in (np.uint16, np.float32):
        if dtype == np.uint16:
            pixels = rng.integers(0, 0x3C01, (12, 17, 4), dtype=np.uint16)
            pixels[0, 0] = [0x7C01, 0xFC01, 0x8000, 0x7E00]
            pixels[3, 5, 3] = 0xFC01
            nan = (pixels[..., 3] & 0x7FFF) > 0x7C00
        else:
            pixels = rng.uniform(-0.5, 1.5, (12, 17, 4)).astype(np.float32)
            pixels[2, 3, 3] = np.nan
            pixels[4, 4, 3] = np.inf
            pixels[5, 5, 0] = np.nan
            nan = np.isnan(pixels[..., 3])
        assert nan.any()
        out = mm.refine_pixels(pixels)
        view = (lambda a: a) if dtype == np.uint16 else (lambda a: np.ascontiguousarray(a).view(np.uint32))
        assert np.array_equal(view(out[..., :3]), view(pixels[..., :3]))
        assert np.array_equal(view(out[..., 3])[~nan], view(pixels[..., 3])[~nan]) and (out[..., 3][nan] == 0).all()
        shown = mm.refine_pixels(pixels, show_matte=True)
        for ch in range(3):
            assert np.array_equal(view(shown[..., ch]), view(out[..., 3]))
        assert (shown[..., 3] == (0x3C00 if dtype == np.uint16 else 1.0)).all()


def test_model_opening_never_raises_and_closing_never_lowers():
    for name, a in _planes():
        for r in (1, 2, 5, 16):
            opened = mm.choke_plane(mm.choke_plane(a, r), -r)
            closed = mm.choke_plane(mm.choke_plane(a, -r), r)
            assert (opened <= a).all() and (closed >= a).all(), (name, r)
            assert (mm.choke_plane(a, r) <= a).all() and (mm.choke_plane(a, -r) >= a).all()
    a = _planes()[0][1]
    assert (mm.choke_plane(a, 1) < a).any() and (mm.choke_plane(a, -1) > a).any()
    one = np.zeros((9, 9), np.float32)
    one[4, 4] = 1
    assert mm.choke_plane(one, -2).sum() == 25 and mm.choke_plane(1 - one, 2).sum() == 81 - 25


def test_model_constant_matte_stays_constant_under_choke():
    """The neighbourhood is clipped to S: nothing erodes in from the border, in windows smaller than 2r + 1 too."""
    for h, w in ((1, 1), (3, 5), (2, 40), (33, 33), (40, 7)):
        flat = np.full((h, w), 0.625, np.float32)
        for r in range(0, 17):
            for choke in (r, -r):
                assert (mm.choke_plane(flat, choke) == np.float32(0.625)).all(), (h, w, choke)
                assert (mm.refine_alpha(flat, choke) == np.float32(0.625)).all()


def test_model_feather_is_the_blur_models_alpha_plane():
    rng = np.random.default_rng(3)
    lists = [[1.0], [0.25, 0.5, 0.25], list(np.float32(rng.uniform(-0.2, 0.4, 9))), list(np.float32(rng.uniform(-0.1, 0.2, 25)))]
    for name, a in _planes():
        src = np.zeros(a.shape + (4,), np.float32)
        src[..., 3] = a
        for taps in lists:
            want = blur_model(src, [np.float32(t) for t in taps])[..., 3]
            assert np.array_equal(mm.feather_plane(a, taps).view(np.uint32), want.view(np.uint32)), (name, len(taps))
    a = _planes()[0][1]
    assert np.array_equal(mm.feather_plane(a, None), a) and np.array_equal(mm.feather_plane(a, [1.0]), a)


def test_model_levels_and_windows():
    a = np.array([[-1.0, 0.0, 0.1, 0.5, 0.9, 1.0, 2.0, np.inf, -np.inf, np.nan]], np.float32)
    got = mm.refine_alpha(a, black=0.1, white=0.9)[0]
    assert got[[0, 1, 2]].tolist() == [0, 0, 0] and got[[5, 6, 7]].tolist() == [1, 1, 1] and got[8] == 0 and got[9] == 0
    assert got[3] == np.float32(np.float32(np.float32(0.5) - np.float32(0.1)) * np.float32(np.float32(1.0) / np.float32(np.float32(0.9) - np.float32(0.1))))
    hard = mm.refine_alpha(a, black=0.5, white=0.500001)[0]
    assert set(hard.tolist()) == {0.0, 1.0} and hard[3] == 0 and hard[4] == 1
    # a target smaller than the source sees the neighbours outside its window
    rng = np.random.default_rng(4)
    src = rng.uniform(0, 1, (20, 30, 4)).astype(np.float32)
    sfull, tfull = (0, 0, 29, 19), (10, 5, 19, 12)
    before = np.full((8, 10, 4), 7.0, np.float32)
    out, win = mm.expected(before, tfull, src, sfull, sfull, choke=2, feather=[0.25, 0.5, 0.25])
    whole = mm.refine_pixels(src, 2, [0.25, 0.5, 0.25])
    assert win == tfull and np.array_equal(out, mm.crop(whole, sfull, tfull))
    alone = mm.refine_pixels(mm.crop(src, sfull, tfull), 2, [0.25, 0.5, 0.25])
    assert not np.array_equal(out, alone)
    assert mm.expected(before, tfull, src, sfull, None)[1] is None and mm.expected(before, (40, 0, 49, 7), src, sfull, sfull)[1] is None


# ---------------------------------------------------------------- the code object

def test_code_object_holds_every_instance_without_scratch():
    """One build for both arithmetic flavours; three pixel layouts (f32, f16 one pixel per lane, f16 pairs)."""
    assert os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"), "the ROCm LLVM tools the build itself needs are missing"
    found = _kernels("matte_ops.hip.o")
    names = [n for n in found if "k_matte_refine" in n]
    assert len(names) == 3 and len(found) == 3, sorted(found)
    for half in (0, 1, 2):
        assert any("k_matte_refineILi%dEEE" % half in n for n in names), half
    for name, (scratch, spills) in found.items():
        assert scratch == 0 and spills == 0, (name, scratch, spills)
    assert not os.path.exists(os.path.join(ROOT, "canvas_amd", "csrc", "build", "matte_ops.fma.hip.o"))
    spec = __import__("importlib.util").util.spec_from_file_location("check_asm_loads", os.path.join(ROOT, "tools", "check_asm_loads.py"))
    chk = __import__("importlib.util").util.module_from_spec(spec)
    spec.loader.exec_module(chk)
    checked, problems = chk.check_paths([os.path.join(ROOT, "canvas_amd", "csrc", "build", "matte_ops.hip.o")])
    assert checked >= 3 and not problems, problems[:5]


# ---------------------------------------------------------------- without a device

def test_pull_without_a_device_or_a_source_gives_an_empty_window():
    """In a child process that sees no GPU: pulled as f16 and as f32, with and without a source, legal and refused settings."""
    script = r"""
import sys
sys.path.insert(0, %r)
from fluggo.media import process, basetypes
window = basetypes.box2i(0, 0, 31, 17)
red = process.SolidColorVideoSource((1, 0, 0, 1))
for source in (red, None):
    for choke in (1, 40):
        node = process.VideoMatteFilter(source, choke, process.gaussian_taps(1.0), 0.1, 0.9, choke == 1)
        assert node.get_frame_f16(0, window).current_window.empty()
        assert node.get_frame_f32(0, window).current_window.empty()
        assert process.last_error(), "no message"
print("message:", process.last_error())
""" % ROOT
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    p = subprocess.run([os.sys.executable, "-c", script], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout
    assert "message:" in p.stdout and re.search(r"device|HIP|hip", p.stdout), p.stdout
