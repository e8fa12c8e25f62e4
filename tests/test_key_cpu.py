"""VideoChromaKeyFilter without a GPU: the two C entries are declared, exported and mirrored, the ctypes struct has the C
struct's layout; every refusal of the contract (DESIGN.md "Chroma key") comes back as -1 with a message and an empty window
before anything is launched; the node's surface; self-checks of the numpy model the GPU tests hold the kernel to
(tests/key_model.py); the built code object holds every k_chroma_key instance without scratch memory and passes the
load-in-flight check; the new sources name none of the scalar-memory-write instructions; a pull without a device ends with an
empty window and a message."""
import ctypes as C
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from tests import key_model as km
from tests.models import f2h_rz_model
from tests.test_unsharp_cpu import _kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SOURCES = ["canvas_amd/csrc/kernels/key_ops.hip", "canvas_amd/csrc/kernels/stream_common.hpp", "canvas_amd/csrc/host/key.c",
               "canvas_amd/pyext/pykey.c", "tools/time_key.py", "tests/key_model.py", "tests/test_key_gpu.py"]
# the shot's parameters: the ones the GPU tests and tools/time_key.py use on km.green_screen
SHOT = dict(key=km.GREEN, tolerance=0.08, softness=0.25, spill=0.8, spill_range=0.4)


@pytest.fixture(scope="module")
def process():
    from fluggo.media import process
    return process


def test_entry_points_declared_exported_and_mirrored():
    header = open(os.path.join(ROOT, "include", "canvas_hip.h")).read()
    for fmt in ("f32", "f16"):
        decl = (r"CVS_EXPORT int cvs_chroma_key_%s_dev\(rgba_frame_%s \*target, const rgba_frame_%s \*source, const cvs_chroma_key \*key, cvs_stream_t s\);"
                % (fmt, fmt, fmt))
        assert re.search(decl, header), decl
    assert re.search(r"enum \{ CVS_KEY_SHOW_MATTE = 1 \};", header)
    from canvas_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for name, frame in (("cvs_chroma_key_f32_dev", _lib.rgba_frame_f32), ("cvs_chroma_key_f16_dev", _lib.rgba_frame_f16)):
        assert hasattr(raw, name) and name in _lib.SIGNATURES, name
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is C.c_int and argtypes == [C.POINTER(frame), C.POINTER(frame), C.POINTER(_lib.chroma_key), C.c_void_p]
    assert _lib.KEY_SHOW_MATTE == 1


def test_struct_mirror_has_the_c_layout():
    """sizeof and every offset, from a probe compiled against the header."""
    from canvas_amd import _lib
    fields = [name for name, _ in _lib.chroma_key._fields_]
    assert fields == ["key", "tolerance", "softness", "spill", "spill_range", "flags"]
    probe = ('#include <stddef.h>\n#include <stdio.h>\n#include "canvas_hip.h"\nint main(void) {\n    printf("%zu", sizeof(cvs_chroma_key));\n'
             + "".join('    printf(" %%zu", offsetof(cvs_chroma_key, %s));\n' % f for f in fields) + '    printf(" %d\\n", CVS_KEY_SHOW_MATTE);\n    return 0;\n}\n')
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "probe.c"), os.path.join(tmp, "probe")
        with open(src, "w") as f:
            f.write(probe)
        subprocess.run(["gcc", "-std=gnu11", "-I" + os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout.split()]
    want = [C.sizeof(_lib.chroma_key)] + [getattr(_lib.chroma_key, f).offset for f in fields] + [_lib.KEY_SHOW_MATTE]
    assert got == want and got[0] == 32


def _key(**kw):
    from canvas_amd import _lib
    v = dict(key=(0.0, 1.0, 0.0), tolerance=0.1, softness=0.1, spill=0.0, spill_range=0.0, flags=0)
    v.update(kw)
    return _lib.chroma_key((C.c_float * 3)(*v["key"]), v["tolerance"], v["softness"], v["spill"], v["spill_range"], v["flags"])


def test_entries_refuse_bad_arguments_before_any_launch():
    from canvas_amd import _lib
    from canvas_amd.abi import HostFrame
    lib = _lib.load()
    full = (0, 0, 7, 7)
    nan, inf = float("nan"), float("inf")
    bad_keys = ([dict(key=k) for k in ((nan, 1, 0), (0, inf, 0), (0, 1, -inf))]
                + [{name: v} for name in ("tolerance", "softness", "spill_range") for v in (-0.5, nan, inf, -inf)])
    for entry, dtype in ((lib.cvs_chroma_key_f16_dev, np.uint16), (lib.cvs_chroma_key_f32_dev, np.float32)):
        def refused(target, source, key, what):
            lib.cvs_clear_last_error()
            assert entry(target, source, key, None) == -1, what
            assert _lib.last_error(), what
        good = HostFrame(full, dtype, current_window=full)
        for kw in bad_keys:
            out = HostFrame(full, dtype, current_window=full)
            refused(out.ref(), good.ref(), C.byref(_key(**kw)), kw)
            assert out.current_window.is_empty(), kw
            assert re.search("finite", _lib.last_error()), _lib.last_error()
        out, outside = HostFrame(full, dtype, current_window=full), HostFrame(full, dtype, current_window=(0, 0, 8, 7))
        refused(out.ref(), outside.ref(), C.byref(_key()), "source window outside its buffer")
        assert out.current_window.is_empty() and "outside" in _lib.last_error()
        out = HostFrame(full, dtype, current_window=full)
        refused(out.ref(), None, C.byref(_key()), "NULL source")
        assert out.current_window.is_empty()
        out = HostFrame(full, dtype, current_window=full)
        refused(out.ref(), good.ref(), None, "NULL key")
        assert out.current_window.is_empty()
        refused(None, good.ref(), C.byref(_key()), "NULL target")
        assert good.current_window.tuple() == full                   # a refused call leaves its source alone


def test_node_surface(process):
    red = process.SolidColorVideoSource((1, 0, 0, 1))
    cls = process.VideoChromaKeyFilter
    assert issubclass(cls, process.VideoSource)
    node = cls(red, (0.0, 1.0, 0.0, 1.0))
    cap = node._video_frame_source_funcs
    assert type(cap).__name__ == "PyCapsule" and '"_video_frame_source_funcs"' in repr(cap)
    assert node.source is red and tuple(node.key)[:3] == (0.0, 1.0, 0.0)
    assert (node.tolerance, node.softness, node.spill, node.spill_range, node.show_matte) == (0.1, 0.1, 0.0, 0.0, False)
    node = cls(red, (0.25, 0.5, 0.75), 0.2, 0.3, 0.5, 0.125, True)
    assert tuple(node.key)[:3] == (0.25, 0.5, 0.75)
    assert (node.tolerance, node.softness, node.spill, node.spill_range, node.show_matte) == (0.2, 0.3, 0.5, 0.125, True)
    node = cls(source=red, key=(0.0, 1.0, 0.0, 1.0), show_matte=True, spill_range=0.5, spill=1.5, softness=0.0, tolerance=0.25)
    assert (node.tolerance, node.softness, node.spill, node.spill_range, node.show_matte) == (0.25, 0.0, 1.5, 0.5, True)
    other = process.SolidColorVideoSource((0, 1, 0, 1))
    node.set_source(other)
    assert node.source is other
    node.source = red
    assert node.source is red
    node.set_source(None)
    assert node.source is None
    ramp = process.LerpFunc((0.0,), (2.0,), 3.0)
    for name in ("tolerance", "softness", "spill", "spill_range"):
        setattr(node, name, 0.375)
        assert getattr(node, name) == 0.375
        setattr(node, name, ramp)
        assert getattr(node, name) is ramp
        for bad in ("much", None, object()):
            with pytest.raises(Exception):
                setattr(node, name, bad)
        assert getattr(node, name) is ramp                          # a refused value leaves the old one
        setattr(node, name, 2)
        assert getattr(node, name) == 2.0
    colour = process.LerpFunc((0.0, 1.0, 0.0, 1.0), (0.0, 0.0, 1.0, 1.0), 4.0)
    node.key = colour
    assert node.key is colour
    node.key = (0.5, 0.25, 0.125, 1.0)
    assert tuple(node.key) == (0.5, 0.25, 0.125, 1.0)
    for bad in ("green", None, object(), (1, 2, 3, 4, 5), ()):
        with pytest.raises(Exception):
            node.key = bad
    assert tuple(node.key) == (0.5, 0.25, 0.125, 1.0)
    node.show_matte = False
    assert node.show_matte is False
    for bad in (1, "yes", None):
        with pytest.raises(TypeError):
            node.show_matte = bad
    for bad in (object(), 3, "source"):
        with pytest.raises(Exception):
            cls(bad, (0, 1, 0, 1))
        with pytest.raises(Exception):
            node.set_source(bad)
    with pytest.raises(TypeError):
        cls(red)                                                     # the key has no default
    with pytest.raises(Exception):
        cls(red, "green")
    with pytest.raises(TypeError):
        cls(red, None)
    with pytest.raises(Exception):
        cls(red, (0, 1, 0, 1), tolerance="wide")


# ---------------------------------------------------------------- the model

def _px(*rgba):
    return np.array([[rgba]], np.float32)


def test_model_key_colour_is_removed_and_far_colours_are_kept():
    key = (0.1, 0.8, 0.2)
    assert km.matte(_px(0.1, 0.8, 0.2, 1.0), key, 0.1, 0.1)[0, 0] == 0
    assert km.matte(_px(0.1, 0.8, 0.2, 1.0), key, 0.0, 0.0)[0, 0] == 0            # d == tolerance == 0: the hard edge removes it
    assert km.key_f32(_px(0.1, 0.8, 0.2, 0.75), key, 0.1, 0.1)[0, 0].tolist() == [np.float32(0.1), np.float32(0.8), np.float32(0.2), 0.0]
    rng = np.random.default_rng(5)
    s = rng.uniform(0, 1, (64, 64, 4)).astype(np.float32)
    d = km.distance(s, key)
    far = d >= np.float32(0.1) + np.float32(0.25)
    assert far.sum() > 100
    for spill in (0.0, 0.7):
        out = km.key_f32(s, key, 0.1, 0.25, spill, 0.1)
        assert np.array_equal(out[..., 3][far].view(np.uint32), s[..., 3][far].view(np.uint32))      # the alpha code is kept


def test_model_matte_does_not_decrease_with_distance():
    """A sweep from the key colour towards magenta: d grows, m must not fall, for a soft and for a hard edge."""
    key = np.array([0.0, 1.0, 0.0], np.float32)
    t = np.linspace(0.0, 1.0, 4001, dtype=np.float32)[:, None]
    s = np.ones((4001, 1, 4), np.float32)
    s[:, 0, :3] = key * (1 - t) + np.array([1.0, 0.0, 1.0], np.float32) * t
    d = km.distance(s, key)[:, 0]
    assert (np.diff(d) >= 0).all() and d[0] == 0 and d[-1] > 0.5
    for softness in (0.3, 0.0):
        m = km.matte(s, key, 0.15, softness)[:, 0]
        assert (np.diff(m) >= 0).all() and m[0] == 0 and m[-1] == 1
        assert ((m > 0) & (m < 1)).any() == (softness > 0)
    ws = km.spill_weight(s, key, 0.15, 0.5, 0.3)[:, 0]
    assert (np.diff(ws) <= 0).all() and ws[0] == 0.5 and ws[-1] == 0


def test_model_spill_zero_returns_the_colour_codes_and_matte_view_is_opaque():
    rng = np.random.default_rng(6)
    codes = rng.integers(0, 0x3C01, (32, 32, 4), dtype=np.uint16)
    codes[0, 0] = [0x7C01, 0xFC01, 0x8000, 0x3C00]                                  # signalling NaNs and -0 are codes too
    s = km.widen(codes)
    for spill in (0.0, -1.0, float("nan")):
        out = km.key_f32(s, km.GREEN, 0.1, 0.2, spill, 0.3)
        assert np.array_equal(out[..., :3].view(np.uint32), s[..., :3].view(np.uint32))
        assert np.array_equal(km.key_pixels(codes, km.GREEN, 0.1, 0.2, spill, 0.3)[..., :3], codes[..., :3])
    assert km.clamp_spill(1.5) == 1 and km.clamp_spill(0.5) == 0.5 and km.clamp_spill(-2) == 0
    assert np.array_equal(km.key_f32(s, km.GREEN, 0.1, 0.2, 1.5, 0.3).view(np.uint32), km.key_f32(s, km.GREEN, 0.1, 0.2, 1.0, 0.3).view(np.uint32))
    view = km.key_f32(s, km.GREEN, 0.1, 0.2, 0.5, 0.3, show_matte=True)
    assert (view[..., 3] == 1.0).all()
    alpha = km.key_f32(s, km.GREEN, 0.1, 0.2, 0.0, 0.0)[..., 3]
    for c in range(3):
        assert np.array_equal(view[..., c].view(np.uint32), alpha.view(np.uint32))
    assert (km.key_pixels(codes, km.GREEN, 0.1, 0.2, show_matte=True)[..., 3] == 0x3C00).all()


def test_model_statement_on_known_values():
    # key black: kpb = kpr = 0; a pixel (0, 0, 1): pb = 0.5, pr = -0.045847 -> d = sqrt(0.25 + 0.045847^2)
    d = km.distance(_px(0.0, 0.0, 1.0, 1.0), (0, 0, 0))[0, 0]
    pr = np.float32(-0.045847)
    assert d == np.sqrt(np.float32(np.float32(0.25) + np.float32(pr * pr)))
    assert abs(float(d) - math.hypot(0.5, 0.045847)) < 1e-7
    # hard edges: at d == tolerance the pixel is removed, one code beyond it is kept
    beyond = np.nextafter(d, np.float32(-1))
    assert km.matte(_px(0, 0, 1, 1), (0, 0, 0), d, 0.0)[0, 0] == 0 and km.matte(_px(0, 0, 1, 1), (0, 0, 0), beyond, 0.0)[0, 0] == 1
    assert km.spill_weight(_px(0, 0, 1, 1), (0, 0, 0), d, 0.75, 0.0)[0, 0] == 0.75
    assert km.spill_weight(_px(0, 0, 1, 1), (0, 0, 0), beyond, 0.75, 0.0)[0, 0] == 0
    # soft edge: halfway up the ramp halves alpha
    half = km.key_f32(_px(0, 0, 1, 0.5), (0, 0, 0), d - np.float32(0.125), 0.25)[0, 0]
    assert abs(float(half[3]) - 0.25) < 1e-6 and half[:3].tolist() == [0, 0, 1]
    # full despill pulls every colour onto the luma
    grey = km.key_f32(_px(0, 0, 1, 1), (0, 0, 1), 0.1, 0.0, 1.0, 0.0)[0, 0]
    assert grey[3] == 0 and grey[0] == np.float32(0.0722) and grey[1] == np.float32(0.0722) and abs(float(grey[2]) - 0.0722) < 1e-7
    # ramp: the three branches and NaN
    assert km.ramp(np.array([-1, -0.0, 0.0, 0.25, 1, 7, np.nan, np.inf, -np.inf], np.float32)).tolist() == [0, 0, 0, 0.25, 1, 1, 1, 1, 0]


def test_model_keeps_a_nan_pixel():
    """A pixel whose distance is NaN keeps its alpha and gets no spill suppression, soft edge or hard."""
    for bad in (np.nan, np.inf, -np.inf):
        s = _px(bad, 0.5, 0.25, 0.75)
        assert np.isnan(km.distance(s, km.GREEN)[0, 0]) or np.isinf(km.distance(s, km.GREEN)[0, 0])
    s = _px(np.nan, 0.5, 0.25, 0.75)
    for softness, spill_range in ((0.2, 0.3), (0.0, 0.0)):
        assert km.matte(s, km.GREEN, 0.1, softness)[0, 0] == 1
        assert km.spill_weight(s, km.GREEN, 0.1, 0.8, spill_range)[0, 0] == 0
        out = km.key_f32(s, km.GREEN, 0.1, softness, 0.8, spill_range)[0, 0]
        assert out[3] == np.float32(0.75) and np.isnan(out[0])
    inf = _px(np.inf, 0.0, 0.0, 0.5)                                 # pb = -Inf, pr = +Inf: d = +Inf, kept
    assert km.matte(inf, km.GREEN, 0.1, 0.2)[0, 0] == 1
    assert f2h_rz_model(km.key_f32(inf, km.GREEN, 0.1, 0.2))[0, 0].tolist() == [0x7C00, 0, 0, 0x3800]


def test_synthetic_shot_exercises_the_ramps():
    """The picture the GPU tests and the timing tool key: with their parameters at least a tenth of its pixels lie on the
    matte's ramp and at least a tenth get some spill suppression; the ground goes and most of the subject's middle stays."""
    for width, height, seed in ((320, 180, 0), (97, 61, 3)):
        shot = km.green_screen(width, height, seed)
        assert shot.shape == (height, width, 4) and shot.dtype == np.float32 and (shot[..., 3] == 1).all()
        assert np.array_equal(shot, km.green_screen(width, height, seed))
        m = km.matte(shot, SHOT["key"], SHOT["tolerance"], SHOT["softness"])
        ws = km.spill_weight(shot, SHOT["key"], SHOT["tolerance"], SHOT["spill"], SHOT["spill_range"])
        assert ((m > 0) & (m < 1)).mean() >= 0.10, ((m > 0) & (m < 1)).mean()
        assert (ws > 0).mean() >= 0.10, (ws > 0).mean()
        assert (m == 0).mean() >= 0.10 and (m == 1).mean() >= 0.10
        inner = m[height // 3:2 * height // 3, width // 3:2 * width // 3]
        assert m[0, 0] == 0 and inner.mean() > 0.5 and (inner == 1).any()


# ---------------------------------------------------------------- the code object and the sources

def test_code_object_holds_every_instance_without_scratch():
    """One build for both arithmetic flavours: three pixel layouts (f32, f16 one pixel per lane, f16 pairs) x (plain, despill,
    matte view)."""
    assert os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"), "the ROCm LLVM tools the build itself needs are missing"
    found = _kernels("key_ops.hip.o")
    names = [n for n in found if "k_chroma_key" in n]
    assert len(names) == 9 and len(found) == 9, sorted(found)
    for half in (0, 1, 2):
        for spill, matte in ((0, 0), (1, 0), (0, 1)):
            assert any("k_chroma_keyILi%dELb%dELb%dEEE" % (half, spill, matte) in n for n in names), (half, spill, matte)
    for name, (scratch, spills) in found.items():
        assert scratch == 0 and spills == 0, (name, scratch, spills)
    assert not os.path.exists(os.path.join(ROOT, "canvas_amd", "csrc", "build", "key_ops.fma.hip.o"))
    spec = __import__("importlib.util").util.spec_from_file_location("check_asm_loads", os.path.join(ROOT, "tools", "check_asm_loads.py"))
    chk = __import__("importlib.util").util.module_from_spec(spec)
    spec.loader.exec_module(chk)
    checked, problems = chk.check_paths([os.path.join(ROOT, "canvas_amd", "csrc", "build", "key_ops.hip.o")])
    assert checked >= 9 and not problems, problems[:5]


def test_library_links_the_launcher_once():
    from canvas_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], stdout=subprocess.PIPE, text=True).stdout
    assert "cvs_chroma_key_f16_dev" in out and "cvs_chroma_key_f32_dev" in out
    symbols = subprocess.run(["nm", _lib.LIB_PATH], stdout=subprocess.PIPE, text=True).stdout
    assert re.search(r"\bcvk_chroma_key\b", symbols) and not re.search(r"\bcvk_chroma_key_fma\b", symbols)


def test_new_sources_name_no_scalar_memory_write():
    """Neither in code nor in a comment: scalar stores, scalar buffer and scratch stores, scalar atomics, scalar cache
    write-back and discard.  (The words are put together here so that this file does not hold them either.)"""
    words = ["s_" + w for w in ("store_", "buffer_" + "store_", "scratch_" + "store_", "atomic_", "buffer_" + "atomic_", "dcache_" + "wb", "dcache_" + "discard")]
    for rel in NEW_SOURCES + ["tests/test_key_cpu.py"]:
        text = open(os.path.join(ROOT, rel)).read().lower()
        for word in words:
            assert word not in text, (rel, word)


# ---------------------------------------------------------------- without a device

def test_pull_without_a_device_gives_an_empty_window_and_says_why():
    """In a child process that sees no GPU: pulled as f16 and as f32, with and without a source."""
    script = r"""
import sys
sys.path.insert(0, %r)
from fluggo.media import process, basetypes
window = basetypes.box2i(0, 0, 31, 17)
red = process.SolidColorVideoSource((1, 0, 0, 1))
for source in (red, None):
    for matte in (False, True):
        node = process.VideoChromaKeyFilter(source, (0, 1, 0, 1), 0.1, 0.2, 0.5, 0.3, matte)
        assert node.get_frame_f16(0, window).current_window.empty()
        assert node.get_frame_f32(0, window).current_window.empty()
        assert process.last_error(), "no message"
print("message:", process.last_error())
""" % ROOT
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    p = subprocess.run([os.sys.executable, "-c", script], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout
    assert "message:" in p.stdout and re.search(r"device|HIP|hip", p.stdout), p.stdout
