"""The catalogue of tests/entry_cases.py held to include/canvas_hip.h, without a GPU.

Every case of every group is run once on a factory that only keeps the operands on the host, against a stand-in for the
library that notes which function was called and with what as its last argument.  So the test knows which entries the
catalogue CALLS (not which it names), and that each call hands its entry the factory's stream."""
import ctypes as C
import os
import re

import numpy as np

from canvas_amd import _lib
from canvas_amd.abi import box2i, rgba_frame_f16, rgba_frame_f32
from tests import entry_cases as ec

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "canvas_hip.h")

# Device entries that no catalogue case calls, each with the property of the ENTRY that keeps it out of a recorded graph.
# (None today: the one device entry that runs host callbacks, video_get_frame_dev, is no cvs_*_dev function and is in the
# catalogue all the same, through the workspace's device slot.)
NOT_RECORDED = {}


def header_files():
    """Every header of the library, canvas_hip.h and the extension headers beside it: found, not listed."""
    import glob
    return sorted(glob.glob(os.path.join(os.path.dirname(HEADER), "canvas*.h")))


def declared(text):
    """[(entry, parameter text)] of every `CVS_EXPORT int cvs_*_dev(...);` a header's text declares outside its comments."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.findall(r"CVS_EXPORT\s+int\s+(cvs_\w+_dev)\s*\(([^;{]*?)\)\s*;", text, flags=re.S)


def device_entries(texts=None):
    """Every cvs_*_dev function whose last parameter is a cvs_stream_t: of include/canvas_hip.h, or of the header texts handed in."""
    found = {}
    for text in [open(HEADER).read()] if texts is None else texts:
        for name, params in declared(text):
            last = params.split(",")[-1].split()
            if last[0] == "cvs_stream_t":
                found[name] = last[-1]
    return found


class _HostOnlyFrame:
    def __init__(self, host, ptr):
        cls = rgba_frame_f16 if host.dtype == np.uint16 else rgba_frame_f32
        self.ptr = ptr
        self.c = cls(ptr, box2i.of(*host.full_window.tuple()), box2i.of(*host.current_window.tuple()))

    current_window = property(lambda self: self.c.current_window)

    def ref(self):
        return C.byref(self.c)


class HostOnly(ec.Factory):
    """Operands that exist as descriptions only: addresses that nothing dereferences."""

    def _make_frame(self, o, host):
        o.ptr = 0x10000 * (len(self.objects) + 1)
        o.frame = _HostOnlyFrame(host, o.ptr)

    def _make_buffer(self, o, data):
        o.ptr = 0x10000 * (len(self.objects) + 1)


class Recorder:
    """Stands in for the library: every function returns 0 and is noted with its last argument."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args[-1] if args else None))
            return 0
        return call


def _run_catalogue():
    stream = 0x5EED
    seen = {}                     # entry -> the cases that call it
    for gid, _pin, build in ec.GROUPS:
        rec = Recorder()
        for what, case in build(rec):
            before = len(rec.calls)
            fac = HostOnly(rec, stream)
            assert case(fac) == 0
            made = rec.calls[before:]
            assert made, "%s / %s calls nothing" % (gid, what)
            for name, last in made:
                if name.endswith("_dev"):
                    # (video_get_frame_dev's last argument is the rgba_frame_dev, by reference, that names the stream)
                    handed = last._obj.stream if hasattr(last, "_obj") else last
                    assert handed == stream, "%s / %s: %s is not handed the factory's stream" % (gid, what, name)
                    seen.setdefault(name, []).append("%s / %s" % (gid, what))
            assert fac.objects and any(o.out for o in fac.objects), "%s / %s has no output" % (gid, what)
    return seen


def test_the_header_parser_finds_the_device_entries():
    entries = device_entries()
    assert len(entries) >= 48, sorted(entries)           # 48 when this was written
    for name in ("cvs_half_lookup_dev", "cvs_chain_color_over_f16_dev", "cvs_blur_lanczos_f16_batch_dev", "cvs_frame_to_rgba8_intent_dev",
                 "cvs_scale_bilinear_f32_batch_dev", "cvs_subsample_dv_dev", "cvs_mix_cross_f16_dev"):
        assert name in entries, name
    # every one of them is bound (canvas_amd/_lib.py), with a pointer-sized last argument
    for name in entries:
        assert _lib.SIGNATURES[name][1][-1] is C.c_void_p, name


def test_every_device_entry_is_called_by_a_case_or_excluded_for_a_reason():
    entries = device_entries()
    seen = _run_catalogue()
    called = {n for n in seen if n in entries}
    both = sorted(called & set(NOT_RECORDED))
    assert not both, "called by the catalogue and excluded at once: %r" % both
    missing = sorted(set(entries) - called - set(NOT_RECORDED))
    assert not missing, "device entries that no catalogue case calls and NOT_RECORDED does not name: %r" % missing
    stale = sorted(set(NOT_RECORDED) - set(entries))
    assert not stale, "NOT_RECORDED names what the header does not declare: %r" % stale
    for name, reason in NOT_RECORDED.items():
        assert isinstance(reason, str) and len(reason.split()) >= 4 and "capture" not in reason.lower(), \
            "%s: the reason must be a property of the entry, not of what happens to it under capture" % name
    unknown = sorted(n for n in seen if n.startswith("cvs_") and n.endswith("_dev") and n not in entries)
    assert not unknown, "the catalogue calls device entries the header does not declare: %r" % unknown
    assert "video_get_frame_dev" in seen                    # the workspace stack, through the device slot


def test_group_ids_are_unique_and_cases_repeatable():
    ids = [g[0] for g in ec.GROUPS]
    assert len(ids) == len(set(ids))
    # a case asks for the same operands every time it runs: what lets one call's operands stand in for another's
    rec = Recorder()
    for gid, _pin, build in ec.GROUPS[::7]:
        for what, case in build(rec):
            a, b = HostOnly(rec, 1), HostOnly(rec, 1)
            case(a), case(b)
            spec = lambda f: [(o.cls, o.name, o.out, o.cmp, o.nbytes, o.row_bytes, o.reads) for o in f.objects]
            assert spec(a) == spec(b), "%s / %s" % (gid, what)


# ------------------------------------------------------------------ far from the origin: the classes and the Shifted factory

class KeepsPixels(HostOnly):
    """HostOnly that also keeps what every operand was made of."""

    def _make_frame(self, o, host):
        HostOnly._make_frame(self, o, host)
        o.held = host.array.tobytes()

    def _make_buffer(self, o, data):
        HostOnly._make_buffer(self, o, data)
        o.held = data.tobytes()


class Geometry(Recorder):
    """Stands in for the library and notes, per call, every frame, box, point and transform it is handed -- directly, by
    reference, through a table of pointers or inside a chain job -- as (argument index, kind, value)."""

    def __getattr__(self, name):
        def call(*args):
            seen = []
            for k, a in enumerate(args):
                _walk(a, k, seen, 0)
            self.calls.append((name, seen))
            return 0
        return call


def _walk(a, k, seen, depth):
    if depth > 4 or a is None:
        return
    a = getattr(a, "_obj", a)                                      # byref()
    if isinstance(a, box2i):
        seen.append((k, "box", a.tuple()))
    elif isinstance(a, ec.v2f):
        seen.append((k, "point", (a.x, a.y)))
    elif isinstance(a, _lib.transform_params):
        seen.append((k, "matrix", tuple(a.m)))
    elif isinstance(a, C.Structure) and hasattr(a, "full_window"):
        seen.append((k, "frame", (a.data, a.full_window.tuple(), a.current_window.tuple())))
    elif isinstance(a, C.Structure):
        for field in a._fields_:
            v = getattr(a, field[0])
            if isinstance(v, (C.Structure, C.Array, C._Pointer)):
                _walk(v, k, seen, depth + 1)
    elif isinstance(a, C.Array):
        if issubclass(a._type_, (C.Structure, C._Pointer)):
            for v in a:
                _walk(v, k, seen, depth + 1)
    elif isinstance(a, C._Pointer):
        if a and issubclass(a._type_, C.Structure):
            _walk(a.contents, k, seen, depth + 1)


def _moved(b, d):
    return ec.move_box(b, d)


OFFSET, SOURCE_SCALE = (2 ** 15 + 1, -2 ** 16), 2


def _check_shifted(gid, what, case, k, broken=None):
    """One case at the origin and through Shifted by OFFSET (inputs by k times that): what the stand-in receives.  `case`:
    (the case built against one stand-in, the same built against another, the two stand-ins) -- a catalogue case calls the
    library its group was built for, whatever factory runs it."""
    soff = (OFFSET[0] * k, OFFSET[1] * k)
    near_case, far_case, near_lib, far_lib = case
    near_lib.calls, far_lib.calls = [], []
    near = KeepsPixels(near_lib, 1)
    inner = KeepsPixels(far_lib, 1)
    far = (broken or ec.Shifted)(inner, OFFSET, soff)
    label = "%s / %s" % (gid, what)
    assert near_case(near) == 0 and far_case(far) == 0
    assert len(near.objects) == len(inner.objects) == len(far.moves), label
    move_of = {}
    for a, b, d in zip(near.objects, inner.objects, far.moves):
        assert (a.cls, a.name, a.out, a.cmp, a.nbytes, a.row_bytes, a.reads) == (b.cls, b.name, b.out, b.cmp, b.nbytes, b.row_bytes, b.reads), label
        assert a.held == b.held, "%s: %s was changed on the way through Shifted" % (label, a.name)
        assert a.ptr == b.ptr
        assert (d is None) == (a.frame is None) and (d is None or d == (OFFSET if a.out else soff)), label
        if d is not None:
            move_of[a.ptr] = d
            f, g = a.frame.c, b.frame.c
            assert g.full_window.tuple() == _moved(f.full_window.tuple(), d) and g.current_window.tuple() == _moved(f.current_window.tuple(), d), \
                "%s: %s is not translated by %r" % (label, a.name, d)
    back = far.windows_back()
    for a, w in zip(near.objects, back):
        assert (w is None) == (a.frame is None) and (w is None or w.tuple() == a.frame.c.current_window.tuple()), "%s: windows_back()" % label
    assert [n for n, _ in near_lib.calls] == [n for n, _ in far_lib.calls], label
    frames = 0
    for (name, seen_near), (_, seen_far) in zip(near_lib.calls, far_lib.calls):
        assert [(i, kind) for i, kind, _ in seen_near] == [(i, kind) for i, kind, _ in seen_far], "%s: %s" % (label, name)
        for (i, kind, v), (_, _, w) in zip(seen_near, seen_far):
            where = "%s: %s argument %d (%s)" % (label, name, i, kind)
            if kind == "frame":
                frames += 1
                assert v[0] == w[0] and v[0] in move_of, where
                d = move_of[v[0]]
                assert w[1] == _moved(v[1], d) and w[2] == _moved(v[2], d), "%s is not translated by %r: %r -> %r" % (where, d, v, w)
            elif kind == "box":
                assert w == _moved(v, OFFSET), "%s is not translated by %r: %r -> %r" % (where, OFFSET, v, w)
            elif kind == "point":
                # the scalers: (target, target point, source, source point, factors, ...)
                d = {1: OFFSET, 3: soff}.get(i, (0, 0)) if name.startswith("cvs_scale_bilinear") else None
                assert d is not None, where + ": a point no rule knows"
                assert w == (v[0] + d[0], v[1] + d[1]), "%s is not translated by %r: %r -> %r" % (where, d, v, w)
            elif kind == "matrix":
                # source + Ds = M (target + Dt) + c': the same map, seen from the moved planes (to f32's rounding of c')
                for row in (0, 3):
                    assert w[row:row + 2] == v[row:row + 2], where
                    want = v[row + 2] - (v[row] * OFFSET[0] + v[row + 1] * OFFSET[1]) + soff[row // 3]
                    assert abs(w[row + 2] - want) <= abs(want) * 2.0 ** -23, "%s: translation %r, want %r" % (where, w[row + 2], want)
    return frames


def _cases_twice():
    """(gid, what, (the case built against one Geometry stand-in, against another, the two stand-ins)) for every case"""
    for gid, _pin, build in ec.GROUPS:
        rec_a, rec_b = Geometry(), Geometry()
        for (what, a), (_, b) in zip(build(rec_a), build(rec_b)):
            yield gid, what, (a, b, rec_a, rec_b)


def test_every_group_is_in_exactly_one_class_and_every_entry_has_a_far_run():
    prefixes = {gid.split("[")[0] for gid, _, _ in ec.GROUPS}
    assert prefixes == set(ec.FAR_CLASSES), prefixes ^ set(ec.FAR_CLASSES)
    for prefix, _text, _factors in ec.MODELLED_CASES:
        assert ec.FAR_CLASSES[prefix][0] == "equivariant", prefix
    used, without_offsets, cases = set(), [], 0
    entries = device_entries()
    run_far = {}                          # entry -> classes of its cases that tests/test_far_windows_gpu.py runs
    rec = Recorder()
    for gid, _pin, build in ec.GROUPS:
        for what, case in build(rec):
            cls, rule = ec.far_class(gid, what)
            assert cls in ("equivariant", "modelled", "anchored", "unwindowed")
            used |= {m for m in ec.MODELLED_CASES if m[0] == gid.split("[")[0] and m[1] in what}
            before = len(rec.calls)
            fac = HostOnly(rec, 1)
            case(fac)
            if cls in ("equivariant", "modelled"):              # no case of either class without far offsets: counted
                boxes = [(o.out, o.frame.c.full_window.tuple()) for o in fac.objects if o.frame is not None]
                offsets = ec.far_offsets_for(gid, what, boxes)
                cases += 1
                if len(offsets) < 4:
                    without_offsets.append("%s / %s: %r" % (gid, what, offsets))
                for _name, d, s in offsets:
                    assert not rule["even_dy"] or d[1] % 2 == 0
                    lim = rule["limit"]
                    assert all(-lim <= v <= lim for o, b in boxes for v in ec.move_box(b, d if o else s)), (gid, what, d, s)
                if rule["even_dy"]:
                    odd = ec.odd_dy_offsets(rule, boxes)
                    assert len(odd) >= 4 and all(d[1] % 2 == 1 for _n, d, _s in odd), (gid, what)
            for name, _ in rec.calls[before:]:
                run_far.setdefault(name, set()).add(cls)
    assert not without_offsets and cases >= 900, (cases, without_offsets)      # 902 of the 1 023 cases have a window to move
    assert used == set(ec.MODELLED_CASES), "MODELLED_CASES names no case: %r" % sorted(set(ec.MODELLED_CASES) - used)
    without = sorted(n for n in entries if n not in run_far)
    assert not without, "device entries without any far run: %r" % without
    assert len(entries) >= 48
    windowed = sorted(n for n in entries if run_far[n] == {"unwindowed"})
    assert windowed == ["cvs_float_to_half_dev", "cvs_float_to_half_fast_dev", "cvs_half_lookup_dev", "cvs_half_to_float_dev", "cvs_half_to_float_fast_dev"]


def test_shifted_translates_every_operand_and_changes_no_buffer():
    frames = 0
    for gid, what, case in _cases_twice():
        cls, rule = ec.far_class(gid, what)
        frames += _check_shifted(gid, what, case, rule["source_scale"] if rule else 1)
    assert frames > 1000                     # the walk does find the frames: by reference, in tables, in chain jobs


def test_a_shifted_that_forgets_one_operand_is_caught():
    """Teeth for the proof above: a factory that leaves its second frame where it was must not pass."""
    class Forgetful(ec.Shifted):
        def frame(self, host, out=False, **kw):
            if len(self.objects) == 1:
                self.moves.append(self.offset if out else self.source_offset)
                self.hosts.append(host)
                return self.inner.frame(host, out=out, **kw)
            return ec.Shifted.frame(self, host, out=out, **kw)
    gid, what, case = next(c for c in _cases_twice() if c[0] == "copies_and_conversions")
    try:
        _check_shifted(gid, what, case, 1, broken=Forgetful)
    except AssertionError as e:
        assert "is not translated by" in str(e)
    else:
        raise AssertionError("a Shifted that does not move its second frame passed")
