#!/usr/bin/env python3
"""HIP-event timing of the corner pin (cvs_perspective_f16_dev / _f32_dev) on device-resident frames at 3840x2160 and 1920x1080,
next to the stream it is measured against and the affine transform it shares its tap code with, on the same frames in the same
alternating rounds:
    gain_offset        cvs_gain_offset_f16_dev                         the 8 B read + 8 B written per pixel stream
    rot30_f16          cvs_transform_f16_dev, 30 degrees about the centre, bilinear
    identity_f16       the frame's own corners: affine coefficients (w == 1), every pixel on a sample -- the copy path
    keystone_f16       top edge 0.6 of the bottom, centred: w varies along y
    general_f16        a general convex quad inside the frame
    identity_f32 / keystone_f32 / general_f32                          the same on f32 frames (16 B + 16 B per pixel)
    keystone_cubic_f16 / general_cubic_f16                             the two quads under the Catmull-Rom filter (sixteen taps where
                       bilinear has four), each beside its bilinear row in the same rounds; `vs_bilinear` is the ratio of the medians
All other pins bilinear.  One JSON line per (op, size): microseconds per call (median round, min, max, and every round), the bytes of
the window written (read once, written once) over the median as a fraction of 8 TB/s, the window's share of the frame, the ratios
to gain_offset and to rot30_f16 of the same run, and gain_offset's own min-max spread relative to its median: the margin within
which "costs the same" is meant.

CANVAS_LIB=<path> times another build of the library (an A/B of a kernel variant: tools/experiments/perspective_divides.patch).

Sources and targets rotate over more than 256 MiB of device frames each so that no call is served from the 256 MiB Infinity
Cache; the rounds alternate the ops so that a drift of the machine shows in all of them.  The numbers include the launch."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from canvas_amd import _lib  # noqa: E402
from tests import cubic_model as cm  # noqa: E402
from tests import key_model as km  # noqa: E402
from tests import perspective_model as pm  # noqa: E402
from tests import transform_model as tm  # noqa: E402
from tests.models import f2h_rz_model  # noqa: E402

if os.environ.get("CANVAS_LIB"):                      # A/B runs: another build of the library (never set by the package)
    _lib.LIB_PATH = os.path.abspath(os.environ["CANVAS_LIB"])

SIZES = [(3840, 2160), (1920, 1080)]
PEAK = 8.0e12
ROTATE_BYTES = 288 << 20
SHOT = dict(tolerance=0.08, softness=0.25, spill=0.8, spill_range=0.4)


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
    for size in args.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        full = (0, 0, w - 1, h - 1)
        cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
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

        def share_of(win):
            return (win[2] - win[0] + 1) * (win[3] - win[1] + 1) / float(w * h)

        def pin(quad, half=True, filt=pm.BILINEAR):
            triple = pm.from_quad(pm.outer(full), quad)
            p = _lib.perspective(*triple, filter=filt)
            share = share_of(cm.perspective_target_window(triple, full, full) if filt == _lib.TRANSFORM_CATMULL_ROM else pm.target_window(triple, filt, full, full))
            if half:
                return (lambda i: lib.cvs_perspective_f16_dev(t16[i % n16].ref(), s16[i % n16].ref(), C.byref(p), stream)), 16, share
            return (lambda i: lib.cvs_perspective_f32_dev(t32[i % n32].ref(), s32[i % n32].ref(), C.byref(p), stream)), 32, share

        t = _lib.transform(tm.from_parts(anchor=(cx, cy), position=(cx, cy), rotation=30), tm.BILINEAR)
        rot30 = (lambda i: lib.cvs_transform_f16_dev(t16[i % n16].ref(), s16[i % n16].ref(), C.byref(t), stream)), 16, share_of(tm.target_window(tuple(t.m), tm.BILINEAR, full, full))
        W, H = float(w), float(h)
        quads = [("identity", pm.rect_quad(pm.outer(full))),
                 ("keystone", [(0.2 * W - 0.5, -0.5), (0.8 * W - 0.5, -0.5), (W - 0.5, H - 0.5), (-0.5, H - 0.5)]),
                 ("general", [(0.08 * W, 0.05 * H), (0.93 * W, 0.17 * H), (0.81 * W, 0.96 * H), (0.03 * W, 0.78 * H)])]
        ops = [("gain_offset", (lambda i: lib.cvs_gain_offset_f16_dev(t16[i % n16].ref(), s16[i % n16].ref(), 1.25, 0.0625, stream), 16, 1.0)),
               ("rot30_f16", rot30)]
        ops += [(name + "_f16", pin(quad)) for name, quad in quads] + [(name + "_f32", pin(quad, half=False)) for name, quad in quads]
        ops += [(name + "_cubic_f16", pin(quad, filt=_lib.TRANSFORM_CATMULL_ROM)) for name, quad in quads[1:]]
        times = {name: [] for name, _ in ops}
        for name, (call, _, _) in ops:
            for i in range(args.warmup):
                _lib.check(call(i), name)
            _lib.check(lib.cvs_stream_sync(stream), "sync")
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
            # the transform of the same rounds: round by round, then the median of the ratios
            ratios = [a / b for a, b in zip(times[name], times["rot30_f16"])]
            line = {"op": name, "size": "%dx%d" % (w, h), "us_per_call": round(ms * 1e3, 2),
                    "us_min": round(min(times[name]) * 1e3, 2), "us_max": round(max(times[name]) * 1e3, 2),
                    "us_rounds": [round(v * 1e3, 2) for v in times[name]], "vs_gain_offset": round(ms / base, 3),
                    "vs_rot30_f16": round(statistics.median(ratios), 3), "gain_offset_spread": round(margin, 3), "window_share": round(share, 3),
                    "fraction_of_8TBps_on_%dBpx" % px: round(share * w * h * px / (ms * 1e-3) / PEAK, 3),
                    "frames_f16": n16, "frames_f32": n32, "calls": args.calls}
            if "_cubic" in name:
                line["vs_bilinear"] = round(ms / statistics.median(times[name.replace("_cubic", "")]), 3)
            print(json.dumps(line), flush=True)
        for f in s16 + t16 + s32 + t32:
            f.free()
    lib.cvs_event_destroy(e0)
    lib.cvs_event_destroy(e1)
    lib.cvs_stream_destroy(stream)


if __name__ == "__main__":
    main()
