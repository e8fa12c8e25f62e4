#!/usr/bin/env python3
"""HIP-event timing of back-to-back calls of cvs_temporal_denoise_f16_dev with 1, 2, 3 and 4 neighbours present, all channels
and alpha alone, on a static and a moving picture and, in the same run as yardsticks, of cvs_copy_frame_f16_dev and of
cvs_deinterlace_adaptive_f16_dev with both neighbours, per 3840x2160 f16 frame (--sizes for others), after warm-up
(tools/time_deinterlace.py's model).  One JSON line per (op, picture, size): ms per call, the ratio to the copy's time in the same
run, the bytes the call has to move (8 B written + 8 B read per frame read, per pixel: 24, 32, 40 and 48 with 1 .. 4 neighbours;
the copy's 16) and that rate as a fraction of 8 TB/s.

The frames rotate over at least 512 MB of device memory so that no call is served from the 256 MiB Infinity Cache: call i
denoises frame i of the ring against frames i - 2 .. i + 2.  static: every frame of the ring holds one picture (every weight 1:
every neighbour is summed); moving: two pictures alternate, so the near frames differ from cur everywhere (every weight 0, the far
frames' by the chain rule).  The kernel runs the same instructions either way.  The rounds alternate the ops (--rounds) so that a
drift of the machine shows in all of them; the line reports the median round.  This script's numbers include the launch."""
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

PEAK = 8.0e12
ROTATE_BYTES = 512 << 20
PICTURES = ["static", "moving"]
# which of prev2, prev1, next1, next2 are handed in, by the number of neighbours
GIVEN = {1: (0, 1, 0, 0), 2: (0, 1, 1, 0), 3: (1, 1, 1, 0), 4: (1, 1, 1, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sizes", default="3840x2160")
    ap.add_argument("--threshold", type=float, default=0.02)
    ap.add_argument("--softness", type=float, default=0.04)
    args = ap.parse_args()
    lib = _lib.load()
    _lib.check(lib.cvs_init(0), "cvs_init")
    lib.init_half()
    stream = lib.cvs_stream_create()
    e0, e1 = lib.cvs_event_create(), lib.cvs_event_create()
    deint = [_lib.deinterlace_adaptive(f, args.threshold, args.softness) for f in (0, 1)]
    params = {"": _lib.temporal_denoise(args.threshold, args.softness, _lib.MEDIAN_ALL), "_alpha": _lib.temporal_denoise(args.threshold, args.softness, _lib.MEDIAN_A)}
    entry = lib.cvs_temporal_denoise_f16_dev
    for size in args.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        full = (0, 0, w - 1, h - 1)
        count = max(6, -(-ROTATE_BYTES // (w * h * 8)))
        count += count & 1                                              # two pictures alternate round the ring
        a, b = synth.layer_frame(w, h, 0, 0).array, synth.layer_frame(w, h, 1, 0).array
        sources = [DeviceFrame(full, np.uint16) for _ in range(count)]
        targets = [DeviceFrame(full, np.uint16) for _ in range(count)]
        src = lambda i: sources[i % count].ref()

        def temporal(n, p):
            g = GIVEN[n]
            return lambda i: entry(targets[i % count].ref(), src(i - 2) if g[0] else None, src(i - 1) if g[1] else None, src(i),
                                   src(i + 1) if g[2] else None, src(i + 2) if g[3] else None, C.byref(p), stream)

        ops = {"copy": lambda i: lib.cvs_copy_frame_f16_dev(targets[i % count].ref(), src(i), stream),
               "deinterlace2": lambda i: lib.cvs_deinterlace_adaptive_f16_dev(targets[i % count].ref(), src(i - 1), src(i), src(i + 1), C.byref(deint[i & 1]), stream)}
        moved_per_pixel = {"copy": 16, "deinterlace2": 32}
        for suffix, p in params.items():
            for n in GIVEN:
                ops["temporal%d%s" % (n, suffix)] = temporal(n, p)
                moved_per_pixel["temporal%d%s" % (n, suffix)] = 16 + 8 * n
        for picture in PICTURES:
            for k, f in enumerate(sources):
                f.upload(a if picture == "static" or (k & 1) == 0 else b, stream)
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
                moved = w * h * moved_per_pixel[name]
                print(json.dumps({"op": name, "picture": picture, "size": "%dx%d" % (w, h), "ms_per_call": round(ms, 5),
                                  "ms_rounds": [round(t, 5) for t in times[name]], "vs_copy": round(ms / statistics.median(times["copy"]), 3),
                                  "aim_vs_copy": round(moved_per_pixel[name] / 16.0, 2),
                                  "moved_bytes": moved, "GBps": round(moved / (ms * 1e-3) / 1e9, 1),
                                  "fraction_of_8TBps": round(moved / (ms * 1e-3) / PEAK, 3), "frames": count, "calls": args.calls}), flush=True)
        for f in sources + targets:
            f.free()
    lib.cvs_event_destroy(e0)
    lib.cvs_event_destroy(e1)
    lib.cvs_stream_destroy(stream)


if __name__ == "__main__":
    main()
