#!/usr/bin/env python3
"""HIP-event timing of the scopes (cvs_scope_counts_f16_dev, every kind; cvs_scope_render_f16_dev) on device-resident 3840x2160
f16 frames, next to cvs_frame_to_bytes_dev -- the display edge, which makes the same reads through the same byte table and
writes 4 B per pixel more -- on the same frames in the same alternating rounds.  Four contents, because a counting kernel's
time depends on where its pixels land:
    synthetic  the project's synthetic layer (canvas_amd/synth.py), what the other tools time
    noise      uniform random halfs in 0..1, every channel on its own: counters hit evenly, the vectorscope's widest spread
    ramp       a horizontal ramp 0..1, the same in r, g, b: neighbouring lanes share counters
    flat       one colour: every pixel in one counter, the worst case for atomics
One JSON line per (op, content): microseconds per call (median round, min, max, every round), the ratio to to_bytes on the same
content with to_bytes' own min-max spread beside it, and the 8 B per pixel read over the median as a fraction of 8 TB/s.

The scope calls include the zeroing of the table (a memset on the same stream) and the launch.  Sources rotate over more than
256 MiB of device frames so that no call is served from the 256 MiB Infinity Cache; the rounds alternate the ops so that a
drift of the machine shows in all of them.  Kernel times come from a separate run under
`rocprofv3 --kernel-trace --stats -- python3 tools/time_scope.py`."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from canvas_amd import _lib, synth  # noqa: E402

if os.environ.get("CANVAS_LIB"):                      # A/B runs: another build of the library (never set by the package)
    _lib.LIB_PATH = os.environ["CANVAS_LIB"]

PEAK = 8.0e12
ROTATE_BYTES = 288 << 20
KINDS = [("histogram", _lib.SCOPE_HISTOGRAM), ("waveform", _lib.SCOPE_WAVEFORM), ("parade", _lib.SCOPE_PARADE), ("vectorscope", _lib.SCOPE_VECTORSCOPE)]


def contents(w, h):
    rng = np.random.default_rng(1)
    noise = rng.uniform(0.0, 1.0, (h, w, 4)).astype(np.float16).view(np.uint16)
    ramp = np.broadcast_to(np.linspace(0.0, 1.0, w, dtype=np.float32).astype(np.float16).view(np.uint16)[None, :, None], (h, w, 4)).copy()
    ramp[..., 3] = 0x3C00
    flat = np.broadcast_to(np.array([0.5, 0.25, 0.125, 1.0], np.float16).view(np.uint16), (h, w, 4)).copy()
    return [("synthetic", synth.layer_frame(w, h, 0, 0).array), ("noise", noise), ("ramp", ramp), ("flat", flat)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--size", default="3840x2160")
    ap.add_argument("--columns", type=int, default=256)
    ap.add_argument("--contents", default="synthetic,noise,ramp,flat")
    args = ap.parse_args()
    from canvas_amd.device import DeviceFrame
    lib = _lib.load()
    _lib.check(lib.cvs_init(0), "cvs_init")
    lib.init_half()
    stream = lib.cvs_stream_create()
    e0, e1 = lib.cvs_event_create(), lib.cvs_event_create()
    w, h = (int(v) for v in args.size.split("x"))
    full = (0, 0, w - 1, h - 1)
    count = max(3, -(-ROTATE_BYTES // (w * h * 8)))
    sources = [DeviceFrame(full, np.uint16) for _ in range(count)]
    out_bytes = lib.cvs_malloc(w * h * 4)
    scopes = {name: _lib.scope(kind, full, columns=args.columns) for name, kind in KINDS}
    tables = {name: lib.cvs_malloc(lib.cvs_scope_count(C.byref(p)) * 4) for name, p in scopes.items()}
    size = _lib.v2i()
    _lib.check(lib.cvs_scope_picture_size(C.byref(scopes["parade"]), C.byref(size)), "picture size")
    picture = DeviceFrame((0, 0, size.x - 1, size.y - 1), np.uint16)
    place = _lib.box2i.of(0, 0, size.x - 1, size.y - 1)
    ops = [("to_bytes", lambda i: lib.cvs_frame_to_bytes_dev(out_bytes, sources[i % count].ref(), _lib.LUT_NONE, _lib.DISPLAY_RGBA8, stream))]
    for name, _ in KINDS:
        ops.append((name, lambda i, name=name: lib.cvs_scope_counts_f16_dev(tables[name], sources[i % count].ref(), C.byref(scopes[name]), stream)))
    ops.append(("render_parade", lambda i: lib.cvs_scope_render_f16_dev(picture.ref(), C.byref(place), tables["parade"], C.byref(scopes["parade"]), 1.0 / 16.0, stream)))
    for what, pixels in [c for c in contents(w, h) if c[0] in args.contents.split(",")]:
        for f in sources:
            f.upload(pixels, stream)
        _lib.check(lib.cvs_stream_sync(stream), "sync")
        times = {name: [] for name, _ in ops}
        for name, call in ops:
            for i in range(args.warmup):
                _lib.check(call(i), name)
        _lib.check(lib.cvs_stream_sync(stream), "sync")
        for _ in range(args.rounds):
            for name, call in ops:
                lib.cvs_event_record(e0, stream)
                for i in range(args.calls):
                    _lib.check(call(i), name)
                lib.cvs_event_record(e1, stream)
                lib.cvs_event_sync(e1)
                times[name].append(lib.cvs_event_elapsed_ms(e0, e1) / args.calls)
        base = statistics.median(times["to_bytes"])
        margin = (max(times["to_bytes"]) - min(times["to_bytes"])) / base
        for name, _ in ops:
            ms = statistics.median(times[name])
            line = {"op": name, "content": what, "size": "%dx%d" % (w, h), "columns": args.columns, "us_per_call": round(ms * 1e3, 2),
                    "us_min": round(min(times[name]) * 1e3, 2), "us_max": round(max(times[name]) * 1e3, 2), "us_rounds": [round(t * 1e3, 2) for t in times[name]],
                    "vs_to_bytes": round(ms / base, 3), "to_bytes_spread": round(margin, 3), "frames": count, "calls": args.calls}
            if name != "render_parade":
                line["fraction_of_8TBps_on_8Bpx_read"] = round(w * h * 8 / (ms * 1e-3) / PEAK, 3)
            print(json.dumps(line), flush=True)
    for f in sources + [picture]:
        f.free()
    lib.cvs_free(out_bytes)
    for ptr in tables.values():
        lib.cvs_free(ptr)
    lib.cvs_event_destroy(e0)
    lib.cvs_event_destroy(e1)
    lib.cvs_stream_destroy(stream)


if __name__ == "__main__":
    main()
