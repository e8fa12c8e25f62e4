"""VideoBlurFilter / VideoUnsharpMaskFilter without a GPU: the two C entries are declared, exported and mirrored; the nodes'
surface; gaussian_taps against canvas_amd.synth; self-checks of the numpy model of the contract (tests/unsharp_model.py,
DESIGN.md "Unsharp mask"); the built code objects hold the new kernels in both arithmetic flavours, without scratch memory, and
pass the load-in-flight check; pulls without a device end with an empty window and a message."""
import ctypes as C
import glob
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from tests import unsharp_model as um
from tests.models import blur_model, f2h_rz_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODES = ["VideoBlurFilter", "VideoUnsharpMaskFilter"]
TAPS = (0.25, 0.5, 0.25)


@pytest.fixture(scope="module")
def process():
    from fluggo.media import process
    return process


def test_entry_points_declared_exported_and_mirrored():
    header = open(os.path.join(ROOT, "include", "canvas_hip.h")).read()
    for fmt in ("f32", "f16"):
        decl = (r"CVS_EXPORT int cvs_unsharp_mask_%s_dev\(rgba_frame_%s \*target, const rgba_frame_%s \*source, const float \*taps, int ntaps, "
                r"float amount, float threshold, cvs_stream_t s\);" % (fmt, fmt, fmt))
        assert re.search(decl, header), decl
    assert re.search(r"CVS_FIR_KERNEL_UNSHARP = 13\b", header)
    from canvas_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("cvs_unsharp_mask_f32_dev", "cvs_unsharp_mask_f16_dev"):
        assert hasattr(raw, name) and name in _lib.SIGNATURES, name
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is C.c_int and len(argtypes) == 7 and argtypes[4] is C.c_float and argtypes[5] is C.c_float
    assert _lib.FIR_KERNEL_UNSHARP == 13


def test_entries_refuse_bad_arguments_before_any_launch():
    from canvas_amd import _lib
    from canvas_amd.abi import HostFrame
    lib = _lib.load()
    taps = np.array(TAPS, np.float32)
    tp = taps.ctypes.data_as(C.POINTER(C.c_float))
    full = (0, 0, 7, 7)
    for entry, dtype in ((lib.cvs_unsharp_mask_f16_dev, np.uint16), (lib.cvs_unsharp_mask_f32_dev, np.float32)):
        out, outside = HostFrame(full, dtype), HostFrame(full, dtype, current_window=(0, 0, 8, 7))
        lib.cvs_clear_last_error()
        assert entry(out.ref(), outside.ref(), tp, 3, 1.0, 0.0, None) == -1 and _lib.last_error()
        assert out.current_window.is_empty()


@pytest.mark.parametrize("name", NODES)
def test_node_surface(process, name):
    red = process.SolidColorVideoSource((1, 0, 0, 1))
    cls = getattr(process, name)
    assert issubclass(cls, process.VideoSource)
    node = cls(red, TAPS)
    cap = node._video_frame_source_funcs
    assert type(cap).__name__ == "PyCapsule" and '"_video_frame_source_funcs"' in repr(cap)
    assert node.source is red and node.taps == TAPS
    assert cls(source=red, taps=list(TAPS)).taps == TAPS
    other = process.SolidColorVideoSource((0, 1, 0, 1))
    node.set_source(other)
    assert node.source is other
    node.source = red
    assert node.source is red
    node.set_source(None)
    assert node.source is None
    node.taps = [1, 2.5, 3, 4]
    assert node.taps == (1.0, 2.5, 3.0, 4.0) and all(type(t) is float for t in node.taps)
    third = float(np.float32(1.0 / 3.0))
    node.taps = np.array([1.0 / 3.0], np.float64)
    assert node.taps == (third,)                                   # held as f32
    for bad in (object(), 3, "source"):
        with pytest.raises(Exception):
            cls(bad, TAPS)
        with pytest.raises(Exception):
            node.set_source(bad)
    for bad, error in (((), ValueError), ([], ValueError), (None, TypeError), (3.0, TypeError), ("121", TypeError), ([1.0, "x"], TypeError), ([1.0, None], TypeError)):
        with pytest.raises(error):
            cls(red, bad)
        with pytest.raises(error):
            node.taps = bad
    assert node.taps == (third,)                                   # a refused list leaves the old one
    with pytest.raises(TypeError):
        cls(red)                                                   # taps have no default


def test_unsharp_arguments(process):
    red = process.SolidColorVideoSource((1, 0, 0, 1))
    node = process.VideoUnsharpMaskFilter(red, TAPS)
    assert node.amount == 1.0 and node.threshold == 0.0
    node = process.VideoUnsharpMaskFilter(red, TAPS, 0.5, 0.125)
    assert (node.amount, node.threshold) == (0.5, 0.125)
    node = process.VideoUnsharpMaskFilter(source=red, taps=TAPS, threshold=2.0, amount=-1.0)
    assert (node.amount, node.threshold) == (-1.0, 2.0)
    ramp = process.LerpFunc((0.0,), (2.0,), 3.0)
    node.amount = ramp
    assert node.amount is ramp
    node.threshold = float("inf")
    assert node.threshold == float("inf")
    node.amount = 1.5
    assert node.amount == 1.5
    with pytest.raises(Exception):
        node.amount = "much"
    assert node.amount == 1.5
    with pytest.raises(TypeError):
        process.VideoBlurFilter(red, TAPS, 1.0)                    # the blur has neither
    assert not hasattr(process.VideoBlurFilter(red, TAPS), "amount")


def test_gaussian_taps(process):
    from canvas_amd import synth
    got = process.gaussian_taps(1.5, 9)
    want = synth.gaussian_taps(9, 1.5)
    assert type(got) is tuple and all(type(t) is float for t in got)
    assert np.array_equal(np.array(got, np.float32).view(np.uint32), want.view(np.uint32))
    assert all(float(np.float32(t)) == t for t in got)             # f32 values
    assert len(process.gaussian_taps(1.5)) == 2 * 5 + 1 and len(process.gaussian_taps(sigma=0.5)) == 2 * 2 + 1
    assert process.gaussian_taps(2.0, ntaps=5) == tuple(float(t) for t in synth.gaussian_taps(5, 2.0))
    assert abs(sum(process.gaussian_taps(3.0)) - 1.0) < 1e-6
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            process.gaussian_taps(bad)
    with pytest.raises(ValueError):
        process.gaussian_taps(1.0, 0)


# ---------------------------------------------------------------- the model

def _frame(rng, h, w):
    codes = rng.integers(0, 0x3C01, (h, w, 4), dtype=np.uint16)
    codes[rng.uniform(size=codes.shape) < 0.05] = 0x8000
    codes[rng.uniform(size=codes.shape) < 0.05] = 0xBC00
    return codes


def test_model_amount_zero_and_infinite_threshold_give_the_source():
    rng = np.random.default_rng(3)
    s = um.widen(_frame(rng, 12, 9))
    b = blur_model(s, np.array(TAPS, np.float32))
    assert np.array_equal(um.mask(s, b, 0.0, 0.0).view(np.uint32)[..., 3], s.view(np.uint32)[..., 3])
    assert np.array_equal(um.mask(s, b, 0.0, 0.0), s)              # s + 0 * d: the colours, bit for bit but for -0 + 0
    assert np.array_equal(um.mask(s, b, 1.5, np.inf).view(np.uint32), s.view(np.uint32))
    sharp = um.mask(s, b, 1.5, 0.0)
    assert not np.array_equal(sharp[..., :3], s[..., :3]) and np.array_equal(sharp[..., 3], s[..., 3])


def test_model_statement_on_known_values():
    s = np.array([[[1.0, 0.5, 0.25, 0.75]]], np.float32)
    b = np.array([[[0.5, 0.5, 0.375, 0.0]]], np.float32)
    assert um.mask(s, b, 2.0, 0.0).tolist() == [[[2.0, 0.5, 0.0, 0.75]]]
    assert um.mask(s, b, 2.0, 0.25).tolist() == [[[2.0, 0.5, 0.25, 0.75]]]        # |d| = 0.125 < 0.25 left alone, 0.5 is not
    assert um.mask(s, b, -1.0, 0.0).tolist() == [[[0.5, 0.5, 0.375, 0.75]]]       # amount -1: the blur itself
    nan = np.array([[[np.nan, 1.0, 1.0, 1.0]]], np.float32)
    assert np.isnan(um.mask(s, nan, 1.0, np.inf)[0, 0, 0])                          # a NaN difference is sharpened, not kept
    assert um.widen(np.array([0x7C01, 0xFC01, 0x7E00], np.uint16)).view(np.uint32).tolist() == [0x7FC02000, 0xFFC02000, 0x7FC00000]


def test_model_blur_agrees_with_the_oracle(orc):
    """The model composes the right B: tests/models.py blur_model and the gcc oracle's blur give the same frame on the
    model's input, and expected() places the result in the window."""
    from canvas_amd.abi import HostFrame
    from tests.util import f32p
    rng = np.random.default_rng(8)
    codes = _frame(rng, 14, 11)
    full = (0, 0, 10, 13)
    for taps in (np.array(TAPS, np.float32), np.array([0.1, -0.2, 0.6, 0.3, 0.2], np.float32)):
        s = um.widen(codes)
        src = HostFrame(full, np.float32, s, full)
        out = HostFrame(full, np.float32)
        orc.lib().orc_fir_blur_f32(out.ref(), src.ref(), f32p(taps), len(taps))
        model = blur_model(s, taps)
        assert np.array_equal(out.array, model)
        before = np.full((16, 13, 4), 0x7E17, np.uint16)
        after, win = um.expected(before, (-1, -1, 11, 14), codes, full, full, lambda a, f, c, w: um.crop(model, full, w), 1.5, 0.0)
        assert win == full
        assert np.array_equal(um.crop(after, (-1, -1, 11, 14), full), f2h_rz_model(um.mask(s, model, 1.5, 0.0)))
        assert (after[0] == 0x7E17).all() and (after[:, 0] == 0x7E17).all()
    assert um.expected(before, (20, 20, 30, 30), codes, full, full, None, 1.0, 0.0)[1] is None
    assert um.expected(before, (-1, -1, 11, 14), codes, full, None, None, 1.0, 0.0)[1] is None


# ---------------------------------------------------------------- the code objects

def _kernels(obj):
    """{kernel name: (private segment bytes, spilled VGPRs)} of one object file's gfx950 code object."""
    readelf, objdump = "/opt/rocm/lib/llvm/bin/llvm-readelf", "/opt/rocm/lib/llvm/bin/llvm-objdump"
    build = os.path.join(ROOT, "canvas_amd", "csrc", "build")
    assert os.path.exists(os.path.join(build, obj)), "no kernel objects in tree: build first (python -c 'import __graft_entry__ as g; g.build()')"
    found = {}
    with tempfile.TemporaryDirectory(dir=build) as tmp:
        with open(os.path.join(build, obj), "rb") as f, open(os.path.join(tmp, obj), "wb") as g:
            g.write(f.read())
        subprocess.run([objdump, "-d", "--offloading", obj], cwd=tmp, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        for co in glob.glob(os.path.join(tmp, obj + "*gfx950")):
            notes = subprocess.run([readelf, "--notes", co], stdout=subprocess.PIPE, text=True).stdout
            for name, scratch, spills in re.findall(r"\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)", notes, re.S):
                found[name] = (int(scratch), int(spills))
    return found


@pytest.mark.parametrize("obj", ["unsharp_ops.hip.o", "unsharp_ops.fma.hip.o"])
def test_code_objects_hold_the_kernels_without_scratch(obj):
    assert os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"), "the ROCm LLVM tools the build itself needs are missing"
    found = _kernels(obj)
    fused = [n for n in found if "k_unsharp" in n and "combine" not in n]
    combine = [n for n in found if "k_unsharp_combine" in n]
    assert len(fused) == 6 * 2 * 2, sorted(found)                  # 3..13 taps x two strip widths x two formats
    assert len(combine) == 2, sorted(found)
    for name, (scratch, spills) in found.items():
        assert scratch == 0 and spills == 0, (name, scratch, spills)
    spec = __import__("importlib.util").util.spec_from_file_location("check_asm_loads", os.path.join(ROOT, "tools", "check_asm_loads.py"))
    chk = __import__("importlib.util").util.module_from_spec(spec)
    spec.loader.exec_module(chk)
    checked, problems = chk.check_paths([os.path.join(ROOT, "canvas_amd", "csrc", "build", obj)])
    assert checked >= 26 and not problems, problems[:5]


def test_both_flavours_are_linked_in():
    from canvas_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], stdout=subprocess.PIPE, text=True).stdout
    assert "cvs_unsharp_mask_f16_dev" in out
    symbols = subprocess.run(["nm", _lib.LIB_PATH], stdout=subprocess.PIPE, text=True).stdout
    for name in ("cvk_unsharp", "cvk_unsharp_fma", "cvk_unsharp_combine", "cvk_unsharp_combine_fma"):
        assert re.search(r"\b%s\b" % name, symbols), name


# ---------------------------------------------------------------- without a device

def test_pull_without_a_device_gives_an_empty_window_and_says_why():
    """In a child process that sees no GPU: both nodes, pulled as f16 and as f32, with and without a source."""
    script = r"""
import sys
sys.path.insert(0, %r)
from fluggo.media import process, basetypes
window = basetypes.box2i(0, 0, 31, 17)
red = process.SolidColorVideoSource((1, 0, 0, 1))
for source in (red, None):
    for node in (process.VideoBlurFilter(source, (0.25, 0.5, 0.25)), process.VideoUnsharpMaskFilter(source, (0.25, 0.5, 0.25), 1.5, 0.01)):
        assert node.get_frame_f16(0, window).current_window.empty()
        assert node.get_frame_f32(0, window).current_window.empty()
        assert process.last_error(), "no message"
print("message:", process.last_error())
""" % ROOT
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    p = subprocess.run([os.sys.executable, "-c", script], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout
    assert "message:" in p.stdout and re.search(r"device|HIP|hip", p.stdout), p.stdout
