#!/usr/bin/env python3
"""HIP-event timing of back-to-back calls of the three field-conversion entries (cvs_field_to_frame_f16_dev,
cvs_soften_fields_f16_dev, cvs_interlace_fields_f16_dev) and, in the same run as the yardstick, of cvs_copy_frame_f16_dev,
at 720x480, 1920x1080 and 3840x2160, after warm-up.  One JSON line per (op, size): ms per call, the bytes the call has to move
(copy, soften, interlace: 8 B read + 8 B written per pixel; field_to_frame: 4 + 8) and that rate as a fraction of 8 TB/s.

Sources and targets each rotate over at least 512 MB of device frames so that no call is served from the 256 MiB Infinity
Cache.  The rounds alternate the four ops (--rounds) so that a drift of the machine shows in all of them; the line reports
the median round.  Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats -- python3
tools/time_fields.py`; this script's own numbers include the launch."""
import argparse
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
BYTES_PER_PIXEL = {"copy": 16, "field_to_frame": 12, "soften": 16, "interlace": 16}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", default=",".join("%dx%d" % s for s in SIZES))
    args = ap.parse_args()
    lib = _lib.load()
    _lib.check(lib.cvs_init(0), "cvs_init")
    lib.init_half()
    stream = lib.cvs_stream_create()
    e0, e1 = lib.cvs_event_create(), lib.cvs_event_create()
    for size in args.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        full = (0, 0, w - 1, h - 1)
        count = max(3, -(-ROTATE_BYTES // (w * h * 8)))
        codes = synth.layer_frame(w, h, 0, 0).array
        sources = [DeviceFrame(full, np.uint16) for _ in range(count)]
        targets = [DeviceFrame(full, np.uint16) for _ in range(count)]
        for f in sources:
            f.upload(codes, stream)
        _lib.check(lib.cvs_stream_sync(stream), "sync")
        ops = {
            "copy": lambda i: lib.cvs_copy_frame_f16_dev(targets[i % count].ref(), sources[i % count].ref(), stream),
            "field_to_frame": lambda i: lib.cvs_field_to_frame_f16_dev(targets[i % count].ref(), sources[i % count].ref(), i & 1, stream),
            "soften": lambda i: lib.cvs_soften_fields_f16_dev(targets[i % count].ref(), sources[i % count].ref(), stream),
            "interlace": lambda i: lib.cvs_interlace_fields_f16_dev(targets[i % count].ref(), sources[i % count].ref(), sources[(i + 1) % count].ref(), stream),
        }
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
            print(json.dumps({"op": name, "size": "%dx%d" % (w, h), "ms_per_call": round(ms, 5), "ms_rounds": [round(t, 5) for t in times[name]],
                              "vs_copy": round(ms / statistics.median(times["copy"]), 3), "moved_bytes": moved,
                              "GBps": round(moved / (ms * 1e-3) / 1e9, 1), "fraction_of_8TBps": round(moved / (ms * 1e-3) / PEAK, 3),
                              "frames": count, "calls": args.calls}), flush=True)
        for f in sources + targets:
            f.free()
    lib.cvs_event_destroy(e0)
    lib.cvs_event_destroy(e1)
    lib.cvs_stream_destroy(stream)


if __name__ == "__main__":
    main()
