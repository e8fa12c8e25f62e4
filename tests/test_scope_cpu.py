"""Video scopes without a GPU (DESIGN.md "Scopes"): the numpy model the GPU tests hold the kernels to against pixel-by-pixel
Python loops; the ranges of the integer Y, Cb, Cr; cvs_scope_count and cvs_scope_picture_size for every kind; the ctypes
struct against the C struct; every refusal of the two device entries and of the host entry -- each comes back as -1 with a
message before the device is touched, with the table (padded on both sides) and the target left as they were; the argument
errors of VideoScopeFilter and of source.get_scope; include/canvas_scope.h against the library and its bindings, and the
catalogue of tests/scope_cases.py against that header."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import scope_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PICTURE_KINDS = (sm.WAVEFORM, sm.PARADE, sm.VECTORSCOPE)


@pytest.fixture(scope="module")
def process():
    from fluggo.media import process
    return process


@pytest.fixture(scope="module")
def bt():
    from fluggo.media import basetypes
    return basetypes


@pytest.fixture(scope="module")
def lib():
    from canvas_amd import _lib
    return _lib.load()


# ---------------------------------------------------------------- the model

def _bytes(rng, w, h):
    px = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    px[rng.uniform(size=(h, w)) < 0.3, 3] = 0                    # transparent pixels for the flag to skip
    px[0, 0, :3] = (0, 0, 255)                                   # Cb reaches 256 here, and Cr on the next: the clamp
    if w > 1:
        px[0, 1, :3] = (255, 0, 0)
    return px


@pytest.mark.parametrize("kind", range(4))
def test_the_model_counts_what_the_loops_count(kind):
    rng = np.random.default_rng(10 + kind)
    for w, h in [(1, 1), (2, 1), (9, 5), (5, 4), (7, 3)]:
        cur = (-3, 2, -3 + w - 1, 2 + h - 1)
        px = _bytes(rng, w, h)
        for region in [cur, (cur[0] - 2, cur[1] - 1, cur[2] + 3, cur[3] + 2), (cur[0] + 1, cur[1], cur[2] + 4, cur[3]), (cur[0] - 5, cur[1], cur[0], cur[1]),
                       (cur[2] + 1, cur[1], cur[2] + 3, cur[3])]:
            for columns in (1, 3, w, 13):
                for skip in (False, True):
                    got = sm.table(kind, px, cur, region, columns, skip)
                    want = sm.table_by_loops(kind, px, cur, region, columns, skip)
                    assert got.dtype == np.uint32 and got.shape == (sm.count(kind, columns),)
                    assert np.array_equal(got, want), (kind, (w, h), region, columns, skip)
        assert not sm.table(kind, px, None, cur, 3).any() and not sm.table_by_loops(kind, px, None, cur, 3).any()
    # every pixel is counted once per row of its table
    px = _bytes(rng, 9, 5)
    rows = {sm.HISTOGRAM: 5, sm.WAVEFORM: 1, sm.PARADE: 3, sm.VECTORSCOPE: 1}[kind]
    assert sm.table(kind, px, (0, 0, 8, 4), (0, 0, 8, 4), 4).sum() == 45 * rows
    assert sm.table(kind, px, (0, 0, 8, 4), (0, 0, 8, 4), 4, True).sum() == int((px[..., 3] != 0).sum()) * rows


@pytest.mark.parametrize("kind", PICTURE_KINDS)
def test_the_model_draws_what_the_loops_draw(kind):
    rng = np.random.default_rng(20 + kind)
    columns = 3
    counts = rng.integers(0, 40, sm.count(kind, columns)).astype(np.uint32)
    counts[::7] = 0
    counts[5], counts[6] = 2 ** 32 - 1, 2 ** 24 + 1                       # (the second is no float: rounded to nearest, once)
    for gain in (0.0, 1.0 / 16.0, 1.0, 3.5, 2.0 ** -32):
        got = sm.picture(kind, counts, columns, gain)
        assert got.dtype == np.uint16 and got.shape == sm.picture_size(kind, columns)[::-1] + (4,)
        assert np.array_equal(got, sm.picture_by_loops(kind, counts, columns, gain)), (kind, gain)
        assert (got[..., 3] == 0x3C00).all()
    assert (sm.picture(kind, counts, columns, 0.0)[..., :3] == 0).all()
    one = sm.picture(kind, counts, columns, 1.0)
    assert set(np.unique(one[..., :3])) == {0, 0x3C00}


def test_luma_and_chroma_ranges_over_every_byte_triple():
    g, b = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), indexing="ij")
    lo, hi, top_b, top_r = [255, 255, 255], [0, 0, 0], [], []
    for r in range(256):
        y = sm.luma(r, g, b)
        cb = 128 + ((-7509 * r - 25259 * g + 32768 * b + 32768) >> 16)
        cr = 128 + ((32768 * r - 29763 * g - 3005 * b + 32768) >> 16)
        for k, v in enumerate((y, cb, cr)):
            lo[k], hi[k] = min(lo[k], int(v.min())), max(hi[k], int(v.max()))
        top_b += [(r, int(i), int(j)) for i, j in np.argwhere(cb == 256)]
        top_r += [(r, int(i), int(j)) for i, j in np.argwhere(cr == 256)]
    assert (lo, hi) == ([0, 1, 1], [255, 256, 256])
    assert top_b == [(0, 0, 255)] and top_r == [(255, 0, 0)]             # pure blue, pure red: hence the min
    v = np.arange(256, dtype=np.int64)
    assert np.array_equal(sm.luma(v, v, v), v)                           # a grey of level v gives v
    cb, cr = sm.chroma(v, v, v)
    assert (cb == 128).all() and (cr == 128).all()
    assert sm.chroma(np.int64(0), np.int64(0), np.int64(255)) == (255, 116) and sm.chroma(np.int64(255), np.int64(0), np.int64(0))[1] == 255
    # the products fit an int32
    assert 46871 * 255 * 2 < 2 ** 31 and (7509 + 25259) * 255 + 32768 < 2 ** 31 and 32768 * 255 + 32768 < 2 ** 31


# ---------------------------------------------------------------- the C surface

def test_count_and_picture_size_for_every_kind(lib):
    from canvas_amd import _lib
    from canvas_amd.abi import v2i
    for kind in range(4):
        for columns in (1, 7, 256, 4096):
            p = _lib.scope(kind, (0, 0, 9, 9), columns=columns)
            assert lib.cvs_scope_count(C.byref(p)) == sm.count(kind, columns), (kind, columns)
            size = v2i(-7, -7)
            rc = lib.cvs_scope_picture_size(C.byref(p), C.byref(size))
            if kind == sm.HISTOGRAM:
                assert rc == -1 and (size.x, size.y) == (-7, -7) and "histogram" in _lib.last_error()
            else:
                assert rc == 0 and (size.x, size.y) == sm.picture_size(kind, columns)
    # the other kinds ignore columns
    for kind in (sm.HISTOGRAM, sm.VECTORSCOPE):
        for columns in (0, -5, 5000):
            assert lib.cvs_scope_count(C.byref(_lib.scope(kind, (0, 0, 9, 9), columns=columns))) == sm.count(kind, 1)
    for kind, columns in [(sm.WAVEFORM, 0), (sm.WAVEFORM, 4097), (sm.PARADE, -1), (sm.PARADE, 4097), (4, 256), (-1, 256)]:
        lib.cvs_clear_last_error()
        p = _lib.scope(kind, (0, 0, 9, 9), columns=columns)
        assert lib.cvs_scope_count(C.byref(p)) == 0 and "cvs_scope_count" in _lib.last_error()
        assert lib.cvs_scope_picture_size(C.byref(p), C.byref(v2i(0, 0))) == -1
    lib.cvs_clear_last_error()
    assert lib.cvs_scope_count(None) == 0 and _lib.last_error()
    assert lib.cvs_scope_picture_size(None, C.byref(v2i(0, 0))) == -1 and lib.cvs_scope_picture_size(C.byref(_lib.scope(1, (0, 0, 1, 1))), None) == -1


def test_struct_mirror_has_the_c_layout():
    """sizeof, every offset and the constants, from a probe compiled against the header."""
    from canvas_amd import _lib
    fields = [name for name, _ in _lib.scope_params._fields_]
    assert fields == ["kind", "pre_lut", "rendering_intent", "columns", "flags", "region"]
    probe = ('#include <stddef.h>\n#include <stdio.h>\n#include "canvas_scope.h"\nint main(void) {\n    printf("%zu", sizeof(cvs_scope));\n'
             + "".join('    printf(" %%zu", offsetof(cvs_scope, %s));\n' % f for f in fields)
             + '    printf(" %d %d %d %d %d %d\\n", CVS_SCOPE_HISTOGRAM, CVS_SCOPE_WAVEFORM, CVS_SCOPE_PARADE, CVS_SCOPE_VECTORSCOPE, CVS_SCOPE_SKIP_TRANSPARENT, CVS_SCOPE_MAX_COLUMNS);\n'
             + "    return 0;\n}\n")
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "probe.c"), os.path.join(tmp, "probe")
        with open(src, "w") as f:
            f.write(probe)
        subprocess.run(["gcc", "-std=gnu11", "-I" + os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout.split()]
    want = ([C.sizeof(_lib.scope_params)] + [getattr(_lib.scope_params, f).offset for f in fields]
            + [_lib.SCOPE_HISTOGRAM, _lib.SCOPE_WAVEFORM, _lib.SCOPE_PARADE, _lib.SCOPE_VECTORSCOPE, _lib.SCOPE_SKIP_TRANSPARENT, _lib.SCOPE_MAX_COLUMNS])
    assert got == want and got[0] == 36
    p = _lib.scope(_lib.SCOPE_PARADE, (1, 2, 3, 4), columns=9, pre_lut=_lib.LUT_LINEAR_TO_SRGB, rendering_intent=1.25, flags=1)
    assert (p.kind, p.pre_lut, p.rendering_intent, p.columns, p.flags, p.region.tuple()) == (2, 3, 1.25, 9, 1, (1, 2, 3, 4))
    P = C.POINTER
    from canvas_amd.abi import box2i, v2i
    assert _lib.SCOPE_SIGNATURES["cvs_scope_count"] == (C.c_size_t, [P(_lib.scope_params)])
    assert _lib.SCOPE_SIGNATURES["cvs_scope_picture_size"] == (C.c_int, [P(_lib.scope_params), P(v2i)])
    assert _lib.SCOPE_SIGNATURES["cvs_scope_counts_f16_dev"] == (C.c_int, [C.c_void_p, P(_lib.rgba_frame_f16), P(_lib.scope_params), C.c_void_p])
    assert _lib.SCOPE_SIGNATURES["cvs_scope_render_f16_dev"] == (C.c_int, [P(_lib.rgba_frame_f16), P(box2i), C.c_void_p, P(_lib.scope_params), C.c_float, C.c_void_p])
    assert _lib.SCOPE_SIGNATURES["video_scope_counts"] == (C.c_int, [C.c_void_p, P(_lib.rgba_frame_f16), P(_lib.scope_params)])


def _declared(header):
    """(every function include/<header> declares with CVS_EXPORT, its cvs_*_dev functions whose last parameter is a cvs_stream_t)"""
    import re
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    text = "\n".join(l for l in text.splitlines() if not l.lstrip().startswith("#"))
    funcs = sorted(set(re.findall(r"CVS_EXPORT\s+[^;(]*?\b(\w+)\s*\(", text)))
    entries = [name for name, params in re.findall(r"CVS_EXPORT\s+int\s+(cvs_\w+_dev)\s*\(([^;{]*?)\)\s*;", text, flags=re.S)
               if params.split(",")[-1].split()[0] == "cvs_stream_t"]
    return funcs, sorted(entries)


def test_every_symbol_of_the_scope_header_is_exported_and_bound(lib):
    """What tests/test_abi_cpu.py holds canvas_hip.h to, for include/canvas_scope.h and its own table of bindings."""
    from canvas_amd import _lib
    funcs, entries = _declared("canvas_scope.h")
    assert funcs == sorted(_lib.SCOPE_SIGNATURES) and len(funcs) == 5
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert not [f for f in funcs if f not in exported]
    assert not set(_lib.SCOPE_SIGNATURES) & set(_lib.SIGNATURES)
    for name in funcs:
        assert getattr(lib, name).argtypes == _lib.SCOPE_SIGNATURES[name][1], name
    for name in entries:
        assert _lib.SCOPE_SIGNATURES[name][1][-1] is C.c_void_p, name
    # the header compiles as C and as C++ on its own
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "t.c")
        with open(src, "w") as f:
            f.write('#include "canvas_scope.h"\nint main(void) { cvs_scope p; v2i s; p.kind = CVS_SCOPE_PARADE; p.columns = 2; (void)s; return sizeof p == 36 ? 0 : 1; }\n')
        for cc, std, lang in (("gcc", "-std=c99", "c"), ("g++", "-std=c++14", "c++")):
            exe = os.path.join(tmp, "t_" + cc)
            subprocess.run([cc, std, "-Wall", "-Werror", "-x", lang, src, "-I", os.path.join(ROOT, "include"), "-o", exe], check=True)
            assert subprocess.run([exe]).returncode == 0


def test_every_device_entry_of_the_scope_header_has_its_catalogue_cases():
    """What tests/test_entry_cases_cpu.py holds tests/entry_cases.py to, for tests/scope_cases.py: every cvs_*_dev entry the
    header declares is CALLED by a case, each call is handed the factory's stream, every case has an output and asks for the same
    operands every time, and the Shifted factory moves every frame and every box -- the region inside the struct, the place --
    and changes no buffer, so the far-window harness runs the cases as it runs the catalogue's."""
    from tests import entry_cases as ec
    from tests import scope_cases as sc
    from tests.test_entry_cases_cpu import Geometry, HostOnly, Recorder, _check_shifted
    _funcs, entries = _declared("canvas_scope.h")
    assert entries == sorted(sc.ENTRIES)
    seen, stream = {}, 0x5EED
    for gid, build in sc.GROUPS:
        rec = Recorder()
        for what, case in build(rec):
            before = len(rec.calls)
            fac = HostOnly(rec, stream)
            assert case(fac) == 0
            made = rec.calls[before:]
            assert len(made) == 1 and made[0][1] == stream, (gid, what, made)
            seen.setdefault(made[0][0], []).append(what)
            assert any(o.out for o in fac.objects), (gid, what)
            again = HostOnly(rec, stream)
            case(again)
            spec = lambda f: [(o.cls, o.name, o.out, o.cmp, o.nbytes, o.row_bytes, o.reads) for o in f.objects]
            assert spec(fac) == spec(again), (gid, what)
            boxes = [(o.out, o.frame.c.full_window.tuple()) for o in fac.objects if o.frame is not None]
            assert len(ec.far_offsets(sc.FAR_RULE, boxes)) >= 4, (gid, what)
    assert sorted(seen) == entries and len(seen["cvs_scope_counts_f16_dev"]) == 32 and len(seen["cvs_scope_render_f16_dev"]) == 3
    frames = boxes_seen = 0
    for gid, build in sc.GROUPS:
        a, b = Geometry(), Geometry()
        for (what, near), (_, far) in zip(build(a), build(b)):
            frames += _check_shifted(gid, what, (near, far, a, b), sc.FAR_RULE["source_scale"])
            boxes_seen += sum(1 for _name, found in b.calls for _i, kind, _v in found if kind == "box")
    assert frames == 35 and boxes_seen >= 35 + 3          # a frame per case; the region of every struct, and the three places


class _Table:
    """A table with 64 bytes of padding on either side, all 0xA5: what a refused call must leave."""

    def __init__(self, counters=65536):
        self.raw = np.full(64 + counters * 4 + 64, 0xA5, np.uint8)
        self.ptr = self.raw.ctypes.data + 64
        assert self.ptr % 4 == 0

    def untouched(self):
        return bool((self.raw == 0xA5).all())


def _bad_scopes():
    """(word the message carries, struct) for everything both device entries refuse about the struct, in the contract's order"""
    from canvas_amd import _lib
    nan, inf = float("nan"), float("inf")
    region = (0, 0, 7, 7)
    bad = [("kind", _lib.scope(k, region)) for k in (-1, 4, 99)]
    bad += [("flags", _lib.scope(1, region, flags=f)) for f in (2, 3, -1, 0x100)]
    bad += [("transfer table", _lib.scope(1, region, pre_lut=t)) for t in (-2, 4, 100)]
    bad += [("rendering_intent", _lib.scope(1, region, rendering_intent=v)) for v in (-1.0, -1e-30, nan, inf, -inf)]
    bad += [("columns", _lib.scope(k, region, columns=c)) for k in (1, 2) for c in (0, -1, 4097, 2 ** 30)]
    return bad


def test_counts_entries_refuse_before_the_device_is_touched(lib):
    from canvas_amd import _lib
    from canvas_amd.abi import HostFrame
    full = (0, 0, 7, 7)
    lim = _lib.MAX_COORD
    for name in ("cvs_scope_counts_f16_dev", "video_scope_counts"):
        entry = getattr(lib, name)
        call = (lambda t, f, p: entry(t, f, p, None)) if name.endswith("_dev") else entry

        def refused(table_ptr, frame, p, word):
            lib.cvs_clear_last_error()
            assert call(table_ptr, frame, p) == -1, (name, word)
            assert name in _lib.last_error() and word in _lib.last_error(), (name, word, _lib.last_error())
        good = HostFrame(full, np.uint16, current_window=full)
        table = _Table()
        ok = _lib.scope(1, full)
        refused(None, good.ref(), C.byref(ok), "need")
        refused(table.ptr, None, C.byref(ok), "need")
        refused(table.ptr, good.ref(), None, "need")
        for off in (1, 2, 3):
            refused(table.ptr + off, good.ref(), C.byref(ok), "4-byte")
        for word, p in _bad_scopes():
            refused(table.ptr, good.ref(), C.byref(p), word)
        for region in [(0, 0, -1, -1), (3, 0, 2, 7), (0, 5, 7, 4)]:
            refused(table.ptr, good.ref(), C.byref(_lib.scope(0, region)), "region is empty")
        outside = HostFrame(full, np.uint16, current_window=(0, 0, 8, 7))
        refused(table.ptr, outside.ref(), C.byref(ok), "outside")
        # coordinates beyond the bound: frames that describe buffers nobody allocates (nothing is dereferenced)
        far = _lib.rgba_frame_f16(good.c.data, _lib.box2i.of(lim - 6, 0, lim + 1, 7), _lib.box2i.of(lim - 6, 0, lim + 1, 7))
        refused(table.ptr, C.byref(far), C.byref(ok), "beyond")
        far = _lib.rgba_frame_f16(good.c.data, _lib.box2i.of(0, -lim - 1, 7, -lim + 6), _lib.box2i.empty())
        refused(table.ptr, C.byref(far), C.byref(ok), "beyond")
        for region in [(0, 0, lim + 1, 7), (-lim - 1, 0, 7, 7), (0, -lim - 1, 7, 7), (0, 0, 7, lim + 1)]:
            refused(table.ptr, good.ref(), C.byref(_lib.scope(3, region)), "beyond")
        # 2^32 pixels to measure: 65536 x 65536
        huge = _lib.box2i.of(0, 0, 65535, 65535)
        refused(table.ptr, C.byref(_lib.rgba_frame_f16(good.c.data, huge, huge)), C.byref(_lib.scope(0, huge.tuple())), "32-bit counter")
        assert table.untouched() and good.current_window.tuple() == full
        # one pixel fewer passes every check: the call gets as far as the device
        fewer = _lib.box2i.of(0, 0, 65535, 65534)
        lib.cvs_clear_last_error()
        rc = call(table.ptr, C.byref(_lib.rgba_frame_f16(good.c.data, huge, fewer)), C.byref(_lib.scope(0, (0, 0, -1, -1))))
        assert rc == -1 and "region is empty" in _lib.last_error()
        if lib.cvs_device_count() == 0:
            # without a device a call that nothing refuses still fails, loudly, and computes nothing on the CPU
            lib.cvs_clear_last_error()
            assert call(table.ptr, good.ref(), C.byref(ok)) != 0 and "no CPU path" in _lib.last_error()
            assert table.untouched()


def test_render_refuses_before_the_device_is_touched(lib):
    from canvas_amd import _lib
    from canvas_amd.abi import HostFrame
    full = (0, 0, 31, 31)
    lim = _lib.MAX_COORD
    nan, inf = float("nan"), float("inf")
    name = "cvs_scope_render_f16_dev"
    table = _Table()
    sentinel = np.array([0x7E17, 0x1234, 0xFBCD, 0x0001], np.uint16)

    def target():
        return HostFrame(full, np.uint16, np.broadcast_to(sentinel, (32, 32, 4)).copy(), full)

    def refused(out, place, table_ptr, p, gain, word):
        lib.cvs_clear_last_error()
        assert lib.cvs_scope_render_f16_dev(None if out is None else out.ref(), place, table_ptr, p, gain, None) == -1, word
        assert name in _lib.last_error() and word in _lib.last_error(), (word, _lib.last_error())
        if out is not None:
            assert out.current_window.is_empty(), word
            assert (out.array == sentinel).all(), word
    ok = _lib.scope(_lib.SCOPE_WAVEFORM, (0, 0, 0, 0), columns=7)
    place = _lib.box2i.of(-2, -5, 4, 250)
    refused(None, C.byref(place), table.ptr, C.byref(ok), 1.0, "need")
    refused(target(), None, table.ptr, C.byref(ok), 1.0, "need")
    refused(target(), C.byref(place), None, C.byref(ok), 1.0, "need")
    refused(target(), C.byref(place), table.ptr, None, 1.0, "need")
    for off in (1, 2, 3):
        refused(target(), C.byref(place), table.ptr + off, C.byref(ok), 1.0, "4-byte")
    refused(target(), C.byref(place), table.ptr, C.byref(_lib.scope(_lib.SCOPE_HISTOGRAM, (0, 0, 0, 0))), 1.0, "histogram")
    for word, p in _bad_scopes():
        refused(target(), C.byref(place), table.ptr, C.byref(p), 1.0, word)
    # the place: empty, or not exactly the picture's size
    for kind, columns, box in [(1, 7, (0, 0, -1, -1)), (1, 7, (0, 0, 6, 254)), (1, 7, (0, 0, 7, 255)), (1, 7, (0, 0, 5, 255)), (2, 7, (0, 0, 6, 255)),
                               (2, 7, (0, 0, 21, 255)), (3, 7, (0, 0, 6, 255)), (3, 7, (0, 0, 255, 256)), (3, 7, (1, 0, 255, 255))]:
        refused(target(), C.byref(_lib.box2i.of(*box)), table.ptr, C.byref(_lib.scope(kind, (0, 0, 0, 0), columns=columns)), 1.0, "place")
    # a place no pixel of which lies within the bound (one that only overhangs it is clipped, as it is against the target)
    refused(target(), C.byref(_lib.box2i.of(lim + 1, 0, lim + 7, 255)), table.ptr, C.byref(ok), 1.0, "beyond")
    refused(target(), C.byref(_lib.box2i.of(0, -lim - 256, 6, -lim - 1)), table.ptr, C.byref(ok), 1.0, "beyond")
    out = target()
    far = _lib.rgba_frame_f16(out.c.data, _lib.box2i.of(lim - 30, 0, lim + 1, 31), _lib.box2i.of(lim - 30, 0, lim + 1, 31))
    lib.cvs_clear_last_error()
    assert lib.cvs_scope_render_f16_dev(C.byref(far), C.byref(place), table.ptr, C.byref(ok), 1.0, None) == -1
    assert "beyond" in _lib.last_error() and far.current_window.is_empty() and (out.array == sentinel).all()
    for gain in (-1.0, -1e-30, nan, inf, -inf):
        refused(target(), C.byref(place), table.ptr, C.byref(ok), gain, "gain")
    assert table.untouched()
    # render reads nothing of the region: an empty one, or one beyond the bound, is not what refuses a call
    # ... nor is a place that overhangs the bound
    for region, where in [((0, 0, -1, -1), place), ((0, 0, lim + 5, 0), place), ((0, 0, 0, 0), _lib.box2i.of(lim - 5, 0, lim + 1, 255)),
                          ((0, 0, 0, 0), _lib.box2i.of(0, -lim - 1, 6, -lim + 254))]:
        out = target()
        lib.cvs_clear_last_error()
        rc = lib.cvs_scope_render_f16_dev(out.ref(), C.byref(where), table.ptr, C.byref(_lib.scope(1, region, columns=7)), 1.0, None)
        if lib.cvs_device_count() == 0:
            assert rc != 0 and "no CPU path" in _lib.last_error()


# ---------------------------------------------------------------- the Python surface

def test_node_arguments_and_properties(process, bt):
    cls = process.VideoScopeFilter
    rect = bt.box2i(0, 0, 63, 35)
    red = process.SolidColorVideoSource((1.0, 0.0, 0.0, 1.0), rect)
    node = cls(red, "waveform", rect)
    assert (node.kind, node.columns, node.display, node.gain, node.skip_transparent) == ("waveform", 256, "export", 1.0 / 16.0, False)
    assert node.source is red and tuple(node.source_rect) == tuple(rect)
    node = cls(red, "parade", rect, 7, "widget", 0.5, True)
    assert (node.kind, node.columns, node.display, node.gain, node.skip_transparent) == ("parade", 7, "widget", 0.5, True)
    node = cls(source=red, kind="vectorscope", source_rect=rect, columns=9, display="export", gain=process.LerpFunc((0.0,), (1.0,), 4.0), skip_transparent=False)
    assert node.kind == "vectorscope" and isinstance(node.gain, process.LerpFunc)
    with pytest.raises(ValueError):
        cls(red, "histogram", rect)                                  # 1280 numbers are the caller's to draw: get_scope
    for kw in (dict(kind="scope"), dict(kind=""), dict(display="screen"), dict(columns=0), dict(columns=4097), dict(columns=-3)):
        with pytest.raises(ValueError):
            cls(**dict(dict(source=red, kind="waveform", source_rect=rect), **kw))
    for kw in (dict(kind=1), dict(kind=None), dict(display=2), dict(columns="wide"), dict(gain=None), dict(gain="bright"), dict(source_rect=(0, 0)),
               dict(source_rect=None), dict(source=object()), dict(source=3)):
        with pytest.raises(Exception):
            cls(**dict(dict(source=red, kind="waveform", source_rect=rect), **kw))
    with pytest.raises(TypeError):
        cls()
    with pytest.raises(TypeError):
        cls(red, "waveform")                                         # source_rect is required
    loose = cls(red, "vectorscope", rect, columns=0)                 # the kinds without columns ignore them ...
    assert loose.columns == 0
    for kind in ("waveform", "parade"):                              # ... and do not turn into a kind that cannot take them
        with pytest.raises(ValueError):
            loose.kind = kind
        assert loose.kind == "vectorscope"
    loose.columns = 9
    loose.kind = "parade"
    assert (loose.kind, loose.columns) == ("parade", 9)
    # a refused value leaves the old one
    node = cls(red, "waveform", rect)
    for name, bad, keeps in (("kind", "histogram", "waveform"), ("kind", "x", "waveform"), ("kind", 3, "waveform"), ("display", "tv", "export"),
                             ("columns", 0, 256), ("columns", 5000, 256), ("columns", 1.5, 256), ("gain", None, 1.0 / 16.0), ("gain", "x", 1.0 / 16.0),
                             ("skip_transparent", 1, False), ("source_rect", (1, 2), tuple(rect))):
        with pytest.raises(Exception):
            setattr(node, name, bad)
        got = getattr(node, name)
        assert (tuple(got) if name == "source_rect" else got) == keeps, name
    node.kind, node.display, node.columns, node.gain, node.skip_transparent, node.source_rect = "parade", "widget", 12, 2.0, True, bt.box2i(1, 2, 3, 4)
    assert (node.kind, node.display, node.columns, node.gain, node.skip_transparent, tuple(node.source_rect)) == ("parade", "widget", 12, 2.0, True, tuple(bt.box2i(1, 2, 3, 4)))
    node.set_source(None)
    assert node.source is None


def test_get_scope_arguments(process, bt):
    rect = bt.box2i(0, 0, 15, 7)
    red = process.SolidColorVideoSource((1.0, 0.0, 0.0, 1.0), rect)
    for args, kw in [((0, rect, "scope"), {}), ((0, rect, "waveform"), dict(display="tv")), ((0, rect, "waveform"), dict(columns=0)),
                     ((0, rect, "parade"), dict(columns=4097))]:
        with pytest.raises(ValueError):
            red.get_scope(*args, **kw)
    for args, kw in [((0, rect), {}), ((0, rect, 1), {}), ((0, (0, 0), "waveform"), {}), ((0, rect, "waveform"), dict(columns="x")), (("a", rect, "waveform"), {})]:
        with pytest.raises(TypeError):
            red.get_scope(*args, **kw)
    # an empty window has nothing to count, with or without a device
    counts, window = red.get_scope(0, bt.box2i(0, 0, -1, -1), "histogram")
    assert counts is None and (window.max.x < window.min.x or window.max.y < window.min.y)
