#!/usr/bin/env python3
"""HIP-event timing of back-to-back calls of cvs_deinterlace_adaptive_f16_dev with two, one and no neighbours on a static, a
moving and a mixed picture and, in the same run as yardsticks, of cvs_copy_frame_f16_dev and cvs_field_to_frame_f16_dev, at
720x480, 1920x1080 and 3840x2160, after warm-up (tools/time_fields.py's model).  One JSON line per (op, picture, size): ms per
call, the ratio to the copy's time in the same run, the bytes the call has to move (8 B written + 8 B read per frame read, per
pixel: 32 with both neighbours, 24 with one; no neighbour is cvs_field_to_frame's 12) and that rate as a fraction of 8 TB/s.

The frames rotate over at least 512 MB of device memory so that no call is served from the 256 MiB Infinity Cache: call i
deinterlaces frame i of the ring against frames i - 1 and i + 1.  static: every frame of the ring holds one picture (k = 0
everywhere: woven); moving: two pictures alternate (k = 1 everywhere: interpolated); mixed: the left half of every frame is one
picture, the right half alternates.  The rounds alternate the ops (--rounds) so that a drift of the machine shows in all of
them; the line reports the median round.  This script's numbers include the launch."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from canvas_amd import _lib, synth  # noqa: E402
from canvas_amd.device import DeviceFrame  # noqa: E402

SIZES = [(720, 480), (1920, 1080), (3840, 2160)]
PEAK = 8.0e12
ROTATE_BYTES = 512 << 20
BYTES_PER_PIXEL = {"copy": 16, "field_to_frame": 12, "adaptive0": 12, "adaptive1": 24, "adaptive2": 32}
PICTURES = ["static", "moving", "mixed"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", default=",".join("%dx%d" % s for s in SIZES))
    ap.add_argument("--threshold", type=float, default=0.02)
    ap.add_argument("--softness", type=float, default=0.04)
    args = ap.parse_args()
    lib = _lib.load()
    _lib.check(lib.cvs_init(0), "cvs_init")
    lib.init_half()
    stream = lib.cvs_stream_create()
    e0, e1 = lib.cvs_event_create(), lib.cvs_event_create()
    params = [_lib.deinterlace_adaptive(f, args.threshold, args.softness) for f in (0, 1)]
    entry = lib.cvs_deinterlace_adaptive_f16_dev
    for size in args.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        full = (0, 0, w - 1, h - 1)
        count = max(4, -(-ROTATE_BYTES // (w * h * 8)))
        count += count & 1                                              # two pictures alternate round the ring
        a, b = synth.layer_frame(w, h, 0, 0).array, synth.layer_frame(w, h, 1, 0).array
        mixed = a.copy()
        mixed[:, w // 2:] = b[:, w // 2:]
        sources = [DeviceFrame(full, np.uint16) for _ in range(count)]
        targets = [DeviceFrame(full, np.uint16) for _ in range(count)]
        src = lambda i: sources[i % count].ref()
        ops = {
            "copy": lambda i: lib.cvs_copy_frame_f16_dev(targets[i % count].ref(), src(i), stream),
            "field_to_frame": lambda i: lib.cvs_field_to_frame_f16_dev(targets[i % count].ref(), src(i), i & 1, stream),
            "adaptive0": lambda i: entry(targets[i % count].ref(), None, src(i), None, C.byref(params[i & 1]), stream),
            "adaptive1": lambda i: entry(targets[i % count].ref(), src(i - 1), src(i), None, C.byref(params[i & 1]), stream),
            "adaptive2": lambda i: entry(targets[i % count].ref(), src(i - 1), src(i), src(i + 1), C.byref(params[i & 1]), stream),
        }
        for picture in PICTURES:
            for k, f in enumerate(sources):
                f.upload(a if picture == "static" or (k & 1) == 0 else (b if picture == "moving" else mixed), stream)
            _lib.check(lib.cvs_stream_sync(stream), "sync")
            times = {name: [] for name in ops}
            for name, call in ops.items():
                for i in range(args.warmup):
                    _lib.check(call(i), name)
            _lib.check(lib.cvs_stream_sync(stream), "sync")
            for _ in range(args.rounds):
                for name, call in ops.items():
                    lib.cvs_event_record(e0, stream)
                    for i in range(args.calls):
                        _lib.check(call(i), name)
                    lib.cvs_event_record(e1, stream)
                    lib.cvs_event_sync(e1)
                    times[name].append(lib.cvs_event_elapsed_ms(e0, e1) / args.calls)
            for name in ops:
                ms = statistics.median(times[name])
                moved = w * h * BYTES_PER_PIXEL[name]
                print(json.dumps({"op": name, "picture": picture, "size": "%dx%d" % (w, h), "ms_per_call": round(ms, 5),
                                  "ms_rounds": [round(t, 5) for t in times[name]], "vs_copy": round(ms / statistics.median(times["copy"]), 3),
                                  "moved_bytes": moved, "GBps": round(moved / (ms * 1e-3) / 1e9, 1),
                                  "fraction_of_8TBps": round(moved / (ms * 1e-3) / PEAK, 3), "frames": count, "calls": args.calls}), flush=True)
        for f in sources + targets:
            f.free()
    lib.cvs_event_destroy(e0)
    lib.cvs_event_destroy(e1)
    lib.cvs_stream_destroy(stream)


if __name__ == "__main__":
    main()
