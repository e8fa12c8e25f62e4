#!/usr/bin/env python3
"""HIP-event timing of the chroma key (cvs_chroma_key_f16_dev / _f32_dev) on device-resident frames at 3840x2160 and 1920x1080,
next to cvs_gain_offset_f16_dev -- the existing entry with the same 8 B read + 8 B written per pixel -- on the same frames in
the same alternating rounds.  The picture is the synthetic green-screen shot of tests/key_model.py with the settings the tests
key it with, so the ramps and the despill are live on a fair share of the pixels.  The ops:
    gain_offset     cvs_gain_offset_f16_dev                       the yardstick
    key_f16         f16 frames, no spill suppression (colour codes copied)
    key_f16_spill   f16 frames with the despill
    key_f16_matte   f16 frames, matte view
    key_f16_inplace f16 frames with the despill, target = source frame
    key_f32_spill   f32 frames with the despill (16 B + 16 B per pixel)
One JSON line per (op, size): microseconds per call (median round, min, max, and every round), the algorithmic bytes over the
median as a fraction of 8 TB/s (for the f16 ops that is 16 B per pixel), and the ratio to gain_offset of the same run with
gain_offset's own min-max spread relative to its median beside it: the margin within which "costs the same" is meant.

Sources and targets rotate over more than 256 MiB of device frames each so that no call is served from the 256 MiB Infinity
Cache; the rounds alternate the ops so that a drift of the machine shows in all of them.  The numbers include the launch.
Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats -- python3 tools/time_key.py`."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from canvas_amd import _lib  # noqa: E402
from tests import key_model as km  # noqa: E402
from tests.models import f2h_rz_model  # noqa: E402

SIZES = [(3840, 2160), (1920, 1080)]
PEAK = 8.0e12
ROTATE_BYTES = 288 << 20
SHOT = dict(tolerance=0.08, softness=0.25, spill=0.8, spill_range=0.4)


def params(spill=True, matte=False):
    return _lib.chroma_key((C.c_float * 3)(*km.GREEN), SHOT["tolerance"], SHOT["softness"], SHOT["spill"] if spill else 0.0, SHOT["spill_range"],
                           _lib.KEY_SHOW_MATTE if matte else 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sizes", default=",".join("%dx%d" % s for s in SIZES))
    args = ap.parse_args()
    from canvas_amd.device import DeviceFrame
    lib = _lib.load()
    _lib.check(lib.cvs_init(0), "cvs_init")
    lib.init_half()
    stream = lib.cvs_stream_create()
    e0, e1 = lib.cvs_event_create(), lib.cvs_event_create()
    plain, spill, matte = params(spill=False), params(), params(matte=True)
    for size in args.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        full = (0, 0, w - 1, h - 1)
        shot = km.green_screen(w, h, 0)
        frames = {}
        for name, dtype, px, pixels in (("f16", np.uint16, 8, f2h_rz_model(shot)), ("f32", np.float32, 16, shot)):
            count = max(3, -(-ROTATE_BYTES // (w * h * px)))
            frames[name] = ([DeviceFrame(full, dtype) for _ in range(count)], [DeviceFrame(full, dtype) for _ in range(count)], pixels)
            for f in frames[name][0]:
                f.upload(pixels, stream)
        _lib.check(lib.cvs_stream_sync(stream), "sync")
        s16, t16, codes = frames["f16"]
        s32, t32, _ = frames["f32"]
        n16, n32 = len(s16), len(s32)

        def restore():
            for f in s16:                                              # the in-place op keys its sources
                f.upload(codes, stream)
                f.c.current_window = f.c.full_window

        # (op, call, bytes per pixel)
        ops = [("gain_offset", lambda i: lib.cvs_gain_offset_f16_dev(t16[i % n16].ref(), s16[i % n16].ref(), 1.25, 0.0625, stream), 16),
               ("key_f16", lambda i: lib.cvs_chroma_key_f16_dev(t16[i % n16].ref(), s16[i % n16].ref(), C.byref(plain), stream), 16),
               ("key_f16_spill", lambda i: lib.cvs_chroma_key_f16_dev(t16[i % n16].ref(), s16[i % n16].ref(), C.byref(spill), stream), 16),
               ("key_f16_matte", lambda i: lib.cvs_chroma_key_f16_dev(t16[i % n16].ref(), s16[i % n16].ref(), C.byref(matte), stream), 16),
               ("key_f32_spill", lambda i: lib.cvs_chroma_key_f32_dev(t32[i % n32].ref(), s32[i % n32].ref(), C.byref(spill), stream), 32),
               ("key_f16_inplace", lambda i: lib.cvs_chroma_key_f16_dev(s16[i % n16].ref(), s16[i % n16].ref(), C.byref(spill), stream), 16)]
        times = {name: [] for name, _, _ in ops}
        for name, call, _ in ops:
            for i in range(args.warmup):
                _lib.check(call(i), name)
        restore()
        _lib.check(lib.cvs_stream_sync(stream), "sync")
        for _ in range(args.rounds):
            for name, call, _ in ops:                                  # the in-place op comes last in a round; restore() follows it
                lib.cvs_event_record(e0, stream)
                for i in range(args.calls):
                    _lib.check(call(i), name)
                lib.cvs_event_record(e1, stream)
                lib.cvs_event_sync(e1)
                times[name].append(lib.cvs_event_elapsed_ms(e0, e1) / args.calls)
            restore()
            _lib.check(lib.cvs_stream_sync(stream), "sync")
        base = statistics.median(times["gain_offset"])
        margin = (max(times["gain_offset"]) - min(times["gain_offset"])) / base
        for name, _, px in ops:
            ms = statistics.median(times[name])
            print(json.dumps({"op": name, "size": "%dx%d" % (w, h), "us_per_call": round(ms * 1e3, 2), "us_min": round(min(times[name]) * 1e3, 2),
                              "us_max": round(max(times[name]) * 1e3, 2), "us_rounds": [round(t * 1e3, 2) for t in times[name]],
                              "vs_gain_offset": round(ms / base, 3), "gain_offset_spread": round(margin, 3),
                              "fraction_of_8TBps_on_%dBpx" % px: round(w * h * px / (ms * 1e-3) / PEAK, 3),
                              "frames_f16": n16, "frames_f32": n32, "calls": args.calls}), flush=True)
        for f in s16 + t16 + s32 + t32:
            f.free()
    lib.cvs_event_destroy(e0)
    lib.cvs_event_destroy(e1)
    lib.cvs_stream_destroy(stream)


if __name__ == "__main__":
    main()
