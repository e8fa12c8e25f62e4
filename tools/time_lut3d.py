#!/usr/bin/env python3
"""HIP-event timing of the 3D LUT (cvs_lut3d_f16_dev / _f32_dev) on device-resident 3840x2160 frames, next to
cvs_gain_offset_f16_dev -- the same row stream, 8 B read + 8 B written per pixel, without the four vertex loads -- on the same
frames in the same alternating rounds.  Lattices of 17, 33 and 65 nodes per axis (79 KB, 575 KB, 4.4 MB on the device), an
identity with a little noise in every node.  Three contents, the scopes' three:
    noise   uniform random colours: every lane of a wave in another cell, the worst case for the vertex loads
    ramp    a horizontal ramp: neighbouring lanes in the same or the next cell
    flat    one colour: every lane loads the same four nodes
The ops: gain_offset (the yardstick), lut_f16_N and lut_f32_N for each N.  One JSON line per (op, content): microseconds per call
(median round, min, max, and every round), the frame's algorithmic bytes (16 B per pixel on f16 frames, 32 on f32; the lattice is
not counted) over the median as a fraction of 8 TB/s, and the ratio to gain_offset of the same run with gain_offset's own min-max
spread relative to its median beside it: the margin within which "costs the same" is meant.

Sources and targets rotate over more than 256 MiB of device frames each so that no call is served from the 256 MiB Infinity
Cache; the rounds alternate the ops so that a drift of the machine shows in all of them.  The numbers include the launch.
CANVAS_LIB=<path> times another build of the library (an A/B of a kernel variant).  Kernel times come from a separate run
under `rocprofv3 --kernel-trace --stats -- python3 tools/time_lut3d.py`."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from canvas_amd import _lib  # noqa: E402
from tests import lut3d_model as lm  # noqa: E402
from tests.models import f2h_rz_model  # noqa: E402

if os.environ.get("CANVAS_LIB"):
    _lib.LIB_PATH = os.path.abspath(os.environ["CANVAS_LIB"])

W, H = 3840, 2160
PEAK = 8.0e12
ROTATE_BYTES = 288 << 20
LATTICES = [17, 33, 65]
CONTENTS = ["noise", "ramp", "flat"]


def content(name):
    """(H, W, 4) f32, opaque"""
    s = np.ones((H, W, 4), np.float32)
    if name == "noise":
        s[..., :3] = np.random.default_rng(0).uniform(0, 1, (H, W, 3)).astype(np.float32)
    elif name == "ramp":
        x = np.linspace(0.0, 1.0, W, dtype=np.float32)[None, :]
        s[..., 0], s[..., 1], s[..., 2] = x, 1.0 - x, 0.5 * x + 0.25
    else:
        s[..., :3] = np.array([0.3, 0.55, 0.2], np.float32)
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--contents", default=",".join(CONTENTS))
    ap.add_argument("--lattices", default=",".join(str(n) for n in LATTICES))
    args = ap.parse_args()
    from canvas_amd.device import DeviceFrame
    lib = _lib.load()
    _lib.check(lib.cvs_init(0), "cvs_init")
    lib.init_half()
    stream = lib.cvs_stream_create()
    e0, e1 = lib.cvs_event_create(), lib.cvs_event_create()
    full = (0, 0, W - 1, H - 1)
    sizes = [int(n) for n in args.lattices.split(",")]
    tables = {}
    for n in sizes:
        lat = (lm.identity(n) + np.random.default_rng(n).uniform(-0.02, 0.02, (n, n, n, 3)).astype(np.float32)).astype(np.float32)
        flat = lm.packed(lat)
        dev = lib.cvs_malloc(flat.nbytes)
        assert dev, _lib.last_error()
        _lib.check(lib.cvs_memcpy_h2d(dev, flat.ctypes.data, flat.nbytes, None), "h2d")
        tables[n] = (dev, _lib.lut3d(n))
    n16, n32 = max(3, -(-ROTATE_BYTES // (W * H * 8))), max(3, -(-ROTATE_BYTES // (W * H * 16)))
    s16, t16 = [DeviceFrame(full, np.uint16) for _ in range(n16)], [DeviceFrame(full, np.uint16) for _ in range(n16)]
    s32, t32 = [DeviceFrame(full, np.float32) for _ in range(n32)], [DeviceFrame(full, np.float32) for _ in range(n32)]
    for name in args.contents.split(","):
        pixels = content(name)
        codes = f2h_rz_model(pixels)
        for f in s16:
            f.upload(codes, stream)
        for f in s32:
            f.upload(pixels, stream)
        _lib.check(lib.cvs_stream_sync(stream), "sync")
        # (op, call, bytes per pixel)
        ops = [("gain_offset", lambda i: lib.cvs_gain_offset_f16_dev(t16[i % n16].ref(), s16[i % n16].ref(), 1.25, 0.0625, stream), 16)]
        for n in sizes:
            dev, p = tables[n]
            ops.append(("lut_f16_%d" % n, lambda i, dev=dev, p=p: lib.cvs_lut3d_f16_dev(t16[i % n16].ref(), s16[i % n16].ref(), dev, C.byref(p), stream), 16))
        for n in sizes:
            dev, p = tables[n]
            ops.append(("lut_f32_%d" % n, lambda i, dev=dev, p=p: lib.cvs_lut3d_f32_dev(t32[i % n32].ref(), s32[i % n32].ref(), dev, C.byref(p), stream), 32))
        times = {op: [] for op, _, _ in ops}
        for op, call, _ in ops:
            for i in range(args.warmup):
                _lib.check(call(i), op)
        _lib.check(lib.cvs_stream_sync(stream), "sync")
        for _ in range(args.rounds):
            for op, call, _ in ops:
                lib.cvs_event_record(e0, stream)
                for i in range(args.calls):
                    _lib.check(call(i), op)
                lib.cvs_event_record(e1, stream)
                lib.cvs_event_sync(e1)
                times[op].append(lib.cvs_event_elapsed_ms(e0, e1) / args.calls)
        base = statistics.median(times["gain_offset"])
        margin = (max(times["gain_offset"]) - min(times["gain_offset"])) / base
        for op, _, px in ops:
            ms = statistics.median(times[op])
            print(json.dumps({"op": op, "content": name, "size": "%dx%d" % (W, H), "us_per_call": round(ms * 1e3, 2), "us_min": round(min(times[op]) * 1e3, 2),
                              "us_max": round(max(times[op]) * 1e3, 2), "us_rounds": [round(t * 1e3, 2) for t in times[op]],
                              "spread": round((max(times[op]) - min(times[op])) / ms, 3), "vs_gain_offset": round(ms / base, 3),
                              "gain_offset_spread": round(margin, 3), "fraction_of_8TBps_on_%dBpx" % px: round(W * H * px / (ms * 1e-3) / PEAK, 3),
                              "frames_f16": n16, "frames_f32": n32, "calls": args.calls}), flush=True)
    for f in s16 + t16 + s32 + t32:
        f.free()
    for dev, _ in tables.values():
        lib.cvs_free(dev)
    lib.cvs_event_destroy(e0)
    lib.cvs_event_destroy(e1)
    lib.cvs_stream_destroy(stream)


if __name__ == "__main__":
    main()
