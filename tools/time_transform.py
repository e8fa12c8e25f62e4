#!/usr/bin/env python3
"""HIP-event timing of the affine transform (cvs_transform_f16_dev / _f32_dev) on device-resident frames at 3840x2160 and
1920x1080, next to the stream it is measured against and the path's other geometry kernel, on the same frames in the same
alternating rounds:
    gain_offset        cvs_gain_offset_f16_dev                      the 8 B read + 8 B written per pixel stream
    scale_f16          cvs_scale_bilinear_f16_dev, factor 0.5 about the centre
    shift_f16          f16 frames, shift (0.5, 0.5), bilinear        axis-aligned: rows read as they are written
    rot30_f16          f16 frames, 30 degrees about the centre, bilinear
    rot90_f16          f16 frames, 90 degrees about the centre       the copy path, columns read along rows
    half_f16           f16 frames, scale 0.5 about the centre, bilinear
    rot30_near_f16     f16 frames, 30 degrees, nearest
    double_f16         f16 frames, scale 2 about the centre, bilinear
    rot30_f32          f32 frames, 30 degrees, bilinear (16 B + 16 B per pixel)
    shift_cubic_f16, rot30_cubic_f16, half_cubic_f16, double_cubic_f16, rot30_cubic_f32
                       the same maps under the Catmull-Rom filter (sixteen taps where bilinear has four), each beside its bilinear
                       row in the same rounds; `vs_bilinear` is the ratio of the two medians
One JSON line per (op, size): microseconds per call (median round, min, max, and every round), the bytes of the window written
(read once, written once) over the median as a fraction of 8 TB/s, the window's share of the frame, the ratio to gain_offset
in the same run, and gain_offset's own min-max spread relative to its median: the margin within which "costs the same" is meant.

Sources and targets rotate over more than 256 MiB of device frames each so that no call is served from the 256 MiB Infinity
Cache; the rounds alternate the ops so that a drift of the machine shows in all of them.  The numbers include the launch.

--plans 32x8,64x4,32x8p,... repeats the whole table once per tile plan (p: the two horizontal taps of a half pixel in one 16-byte
load) and checks that every plan writes the same bytes; it needs the diagnostic build (make -C canvas_amd/csrc diag), whose
host/transform.c reads CVS_TRANSFORM_PLAN.  Without it the package's library and its built-in plan are measured."""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from canvas_amd import _lib  # noqa: E402
from canvas_amd.abi import v2f  # noqa: E402
from tests import cubic_model as cm  # noqa: E402
from tests import key_model as km  # noqa: E402
from tests import transform_model as tm  # noqa: E402
from tests.models import f2h_rz_model  # noqa: E402

SIZES = [(3840, 2160), (1920, 1080)]
PEAK = 8.0e12
ROTATE_BYTES = 288 << 20
CUBIC = _lib.TRANSFORM_CATMULL_ROM
SHOT = dict(tolerance=0.08, softness=0.25, spill=0.8, spill_range=0.4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sizes", default=",".join("%dx%d" % s for s in SIZES))
    ap.add_argument("--plans", default="")
    args = ap.parse_args()
    plans = [p for p in args.plans.split(",") if p]
    if plans:
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        from _diag import use_diag_library
        use_diag_library()
    from canvas_amd.device import DeviceFrame
    lib = _lib.load()
    _lib.check(lib.cvs_init(0), "cvs_init")
    lib.init_half()
    stream = lib.cvs_stream_create()
    e0, e1 = lib.cvs_event_create(), lib.cvs_event_create()
    for size in args.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        full = (0, 0, w - 1, h - 1)
        cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
        mid = dict(anchor=(cx, cy), position=(cx, cy))
        shot = km.key_f32(km.green_screen(w, h, 0), km.GREEN, **SHOT)     # a keyed layer: soft edges, a flat inside, a transparent outside
        frames = {}
        for name, dtype, px, pixels in (("f16", np.uint16, 8, f2h_rz_model(shot)), ("f32", np.float32, 16, shot)):
            count = max(3, -(-ROTATE_BYTES // (w * h * px)))
            frames[name] = ([DeviceFrame(full, dtype) for _ in range(count)], [DeviceFrame(full, dtype) for _ in range(count)])
            for f in frames[name][0]:
                f.upload(pixels, stream)
        _lib.check(lib.cvs_stream_sync(stream), "sync")
        s16, t16 = frames["f16"]
        s32, t32 = frames["f32"]
        n16, n32 = len(s16), len(s32)
        centre, halve = v2f(cx, cy), v2f(0.5, 0.5)

        def warp(parts, filt, half=True):
            t = _lib.transform(tm.from_parts(**parts), filt)
            win = cm.transform_target_window(tuple(t.m), full, full) if filt == CUBIC else tm.target_window(tuple(t.m), filt, full, full)
            share = (win[2] - win[0] + 1) * (win[3] - win[1] + 1) / float(w * h)
            if half:
                return (lambda i: lib.cvs_transform_f16_dev(t16[i % n16].ref(), s16[i % n16].ref(), C.byref(t), stream)), 16, share
            return (lambda i: lib.cvs_transform_f32_dev(t32[i % n32].ref(), s32[i % n32].ref(), C.byref(t), stream)), 32, share

        ops = [("gain_offset", (lambda i: lib.cvs_gain_offset_f16_dev(t16[i % n16].ref(), s16[i % n16].ref(), 1.25, 0.0625, stream), 16, 1.0)),
               ("scale_f16", (lambda i: lib.cvs_scale_bilinear_f16_dev(t16[i % n16].ref(), centre, s16[i % n16].ref(), centre, halve, stream), 16, 0.25)),
               ("shift_f16", warp(dict(position=(0.5, 0.5)), tm.BILINEAR)),
               ("rot30_f16", warp(dict(mid, rotation=30), tm.BILINEAR)),
               ("rot90_f16", warp(dict(mid, rotation=90), tm.BILINEAR)),
               ("half_f16", warp(dict(mid, scale=(0.5, 0.5)), tm.BILINEAR)),
               ("rot30_near_f16", warp(dict(mid, rotation=30), tm.NEAREST)),
               ("double_f16", warp(dict(mid, scale=(2, 2)), tm.BILINEAR)),
               ("rot30_f32", warp(dict(mid, rotation=30), tm.BILINEAR, half=False)),
               ("shift_cubic_f16", warp(dict(position=(0.5, 0.5)), CUBIC)),
               ("rot30_cubic_f16", warp(dict(mid, rotation=30), CUBIC)),
               ("half_cubic_f16", warp(dict(mid, scale=(0.5, 0.5)), CUBIC)),
               ("double_cubic_f16", warp(dict(mid, scale=(2, 2)), CUBIC)),
               ("rot30_cubic_f32", warp(dict(mid, rotation=30), CUBIC, half=False))]
        digests = {}
        for plan in plans or [None]:
            if plan:
                os.environ["CVS_TRANSFORM_PLAN"] = plan
            times = {name: [] for name, _ in ops}
            for name, (call, _, _) in ops:
                for i in range(args.warmup):
                    _lib.check(call(i), name)
                _lib.check(lib.cvs_stream_sync(stream), "sync")
                out = (t32 if name.endswith("f32") else t16)[0].download(stream).array
                digests.setdefault(name, set()).add(hashlib.sha1(out.tobytes()).hexdigest())
            for _ in range(args.rounds):
                for name, (call, _, _) in ops:
                    lib.cvs_event_record(e0, stream)
                    for i in range(args.calls):
                        _lib.check(call(i), name)
                    lib.cvs_event_record(e1, stream)
                    lib.cvs_event_sync(e1)
                    times[name].append(lib.cvs_event_elapsed_ms(e0, e1) / args.calls)
            base = statistics.median(times["gain_offset"])
            margin = (max(times["gain_offset"]) - min(times["gain_offset"])) / base
            for name, (_, px, share) in ops:
                ms = statistics.median(times[name])
                line = {"op": name, "size": "%dx%d" % (w, h), "plan": plan or "built-in", "us_per_call": round(ms * 1e3, 2),
                        "us_min": round(min(times[name]) * 1e3, 2), "us_max": round(max(times[name]) * 1e3, 2),
                        "us_rounds": [round(t * 1e3, 2) for t in times[name]], "vs_gain_offset": round(ms / base, 3),
                        "gain_offset_spread": round(margin, 3), "window_share": round(share, 3),
                        "fraction_of_8TBps_on_%dBpx" % px: round(share * w * h * px / (ms * 1e-3) / PEAK, 3),
                        "frames_f16": n16, "frames_f32": n32, "calls": args.calls}
                if "_cubic" in name:
                    line["vs_bilinear"] = round(ms / statistics.median(times[name.replace("_cubic", "")]), 3)
                print(json.dumps(line), flush=True)
        differing = sorted(name for name, seen in digests.items() if len(seen) != 1)
        print(json.dumps({"size": "%dx%d" % (w, h), "plans": plans or ["built-in"], "ops_whose_bytes_differ_between_plans": differing}), flush=True)
        for f in s16 + t16 + s32 + t32:
            f.free()
        if differing:
            raise SystemExit("plans disagree: %s" % differing)
    lib.cvs_event_destroy(e0)
    lib.cvs_event_destroy(e1)
    lib.cvs_stream_destroy(stream)


if __name__ == "__main__":
    main()
