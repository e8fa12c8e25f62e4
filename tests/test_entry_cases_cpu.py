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


def device_entries():
    """Every cvs_*_dev function the header declares whose last parameter is a cvs_stream_t."""
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    found = {}
    for name, params in re.findall(r"CVS_EXPORT\s+int\s+(cvs_\w+_dev)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
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
