#!/usr/bin/env python3
"""HIP-event timing of the median (cvs_median_f16_dev / _f32_dev) on device-resident frames at 3840x2160 (--sizes for others),
next to cvs_copy_frame_f16_dev -- the 8 B read + 8 B written per pixel the median moves -- and the 9-tap cvs_fir_blur_f16_dev,
the spatial filter an editor would otherwise reach for, on the same frames in the same alternating rounds.  The ops:
    copy, blur9                                  the yardsticks (f16)
    median_<f16|f32>_r<1|2>_<all|a>[_gated]      radius 1 (3 x 3) or 2 (5 x 5); every channel or alpha alone; threshold 0, or
                                                 (_gated) the tests' 0.0625
on two pictures: `speck`, the test picture of tests/median_model.py (ramps with noise, 15 % speck pixels, specials, a flat
block), and `flat`, one colour everywhere.  A selection network does the same work on both; the pictures differ in how the
per-pixel decision of the gated ops falls.
One JSON line per (op, picture, size): microseconds per call (median round, min, max, every round), the ratio to the copy of
the same run with the copy's own min-max spread beside it, and the algorithmic bytes over the median as a fraction of 8 TB/s.

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
from canvas_amd import _lib, synth  # noqa: E402
from tests import median_model as mm  # noqa: E402

SIZES = [(3840, 2160)]
PEAK = 8.0e12
ROTATE_BYTES = 288 << 20
GATE = 0.0625


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sizes", default=",".join("%dx%d" % s for s in SIZES))
    ap.add_argument("--pictures", default="speck,flat")
    args = ap.parse_args()
    from canvas_amd.device import DeviceFrame
    lib = _lib.load()
    _lib.check(lib.cvs_init(0), "cvs_init")
    lib.init_half()
    stream = lib.cvs_stream_create()
    e0, e1 = lib.cvs_event_create(), lib.cvs_event_create()
    taps = np.ascontiguousarray(synth.gaussian_taps(9, 1.5), np.float32)
    tap_ptr = taps.ctypes.data_as(C.POINTER(C.c_float))
    for size in args.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        full = (0, 0, w - 1, h - 1)
        frames = {}
        for name, dtype, px in (("f16", np.uint16, 8), ("f32", np.float32, 16)):
            count = max(3, -(-ROTATE_BYTES // (w * h * px)))
            frames[name] = ([DeviceFrame(full, dtype) for _ in range(count)], [DeviceFrame(full, dtype) for _ in range(count)])
        (s16, t16), (s32, t32) = frames["f16"], frames["f32"]
        n16, n32 = len(s16), len(s32)
        # (op, call, bytes per pixel)
        ops = [("copy", lambda i: lib.cvs_copy_frame_f16_dev(t16[i % n16].ref(), s16[i % n16].ref(), stream), 16),
               ("blur9", lambda i: lib.cvs_fir_blur_f16_dev(t16[i % n16].ref(), s16[i % n16].ref(), tap_ptr, 9, stream), 16)]
        keep = []
        for fmt, entry, src, dst, n, px in (("f16", lib.cvs_median_f16_dev, s16, t16, n16, 16), ("f32", lib.cvs_median_f32_dev, s32, t32, n32, 32)):
            for radius in (1, 2):
                for cname, channels in (("all", _lib.MEDIAN_ALL), ("a", _lib.MEDIAN_A)):
                    for gated in (False, True):
                        p = _lib.median(radius, GATE if gated else 0.0, channels)
                        keep.append(p)
                        ops.append(("median_%s_r%d_%s%s" % (fmt, radius, cname, "_gated" if gated else ""),
                                    lambda i, entry=entry, src=src, dst=dst, n=n, p=p: entry(dst[i % n].ref(), src[i % n].ref(), C.byref(p), stream), px))
        for picture in args.pictures.split(","):
            for dtype, sources in ((np.uint16, s16), (np.uint32, s32)):
                if picture == "speck":
                    bits = mm.speck_picture(np.random.default_rng(1), w, h, dtype)
                else:
                    bits = np.broadcast_to(np.array([0.5, 0.25, 0.75, 1.0], np.float16).view(np.uint16) if dtype == np.uint16
                                           else np.array([0.5, 0.25, 0.75, 1.0], np.float32).view(np.uint32), (h, w, 4)).copy()
                for f in sources:
                    f.upload(bits if dtype == np.uint16 else bits.view(np.float32), stream)
            _lib.check(lib.cvs_stream_sync(stream), "sync")
            times = {name: [] for name, _, _ in ops}
            for name, call, _ in ops:
                for i in range(args.warmup):
                    _lib.check(call(i), name)
            _lib.check(lib.cvs_stream_sync(stream), "sync")
            for _ in range(args.rounds):
                for name, call, _ in ops:
                    lib.cvs_event_record(e0, stream)
                    for i in range(args.calls):
                        _lib.check(call(i), name)
                    lib.cvs_event_record(e1, stream)
                    lib.cvs_event_sync(e1)
                    times[name].append(lib.cvs_event_elapsed_ms(e0, e1) / args.calls)
            base = statistics.median(times["copy"])
            margin = (max(times["copy"]) - min(times["copy"])) / base
            for name, _, px in ops:
                ms = statistics.median(times[name])
                print(json.dumps({"op": name, "picture": picture, "size": "%dx%d" % (w, h), "us_per_call": round(ms * 1e3, 2),
                                  "us_min": round(min(times[name]) * 1e3, 2), "us_max": round(max(times[name]) * 1e3, 2),
                                  "us_rounds": [round(t * 1e3, 2) for t in times[name]], "vs_copy": round(ms / base, 3), "copy_spread": round(margin, 3),
                                  "fraction_of_8TBps_on_%dBpx" % px: round(w * h * px / (ms * 1e-3) / PEAK, 3),
                                  "frames_f16": n16, "frames_f32": n32, "calls": args.calls}), flush=True)
        for f in s16 + t16 + s32 + t32:
            f.free()
    lib.cvs_event_destroy(e0)
    lib.cvs_event_destroy(e1)
    lib.cvs_stream_destroy(stream)


if __name__ == "__main__":
    main()
