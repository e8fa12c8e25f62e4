#!/usr/bin/env python3
"""HIP-event timing of the matte refine (cvs_matte_refine_f16_dev / _f32_dev) on device-resident frames at 3840x2160 and
1920x1080, next to the two existing entries it sits between, on the same frames in the same alternating rounds:
    gain_offset        cvs_gain_offset_f16_dev                      the 8 B read + 8 B written per pixel stream
    matte_f16_c1       f16 frames, choke 1, no feather
    matte_f16_c2_t9    f16 frames, choke 2, 9 Gaussian taps         the middle setting
    matte_f16_c16_t25  f16 frames, choke 16, 25 taps                the largest halo
    matte_f32_c2_t9    f32 frames at the middle setting (16 B + 16 B per pixel)
    blur_f16_t9        cvs_fir_blur_f16_dev, the same 9 taps        the four-channel neighbourhood kernel
    blur_f16_t25       cvs_fir_blur_f16_dev, the same 25 taps
The picture is the keyed synthetic green-screen shot of tests/key_model.py, so the matte has a soft edge, a flat inside and a flat
outside.  One JSON line per (op, size): microseconds per call (median round, min, max, and every round), the algorithmic bytes
over the median as a fraction of 8 TB/s, the ratio to gain_offset and to the blur of the same tap count in the same run, and
gain_offset's own min-max spread relative to its median: the margin within which "costs the same" is meant.

Sources and targets rotate over more than 256 MiB of device frames each so that no call is served from the 256 MiB Infinity
Cache; the rounds alternate the ops so that a drift of the machine shows in all of them.  The numbers include the launch.
Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats -- python3 tools/time_matte.py`."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from canvas_amd import _lib, synth  # noqa: E402
from tests import key_model as km  # noqa: E402
from tests.models import f2h_rz_model  # noqa: E402

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
    taps9 = np.ascontiguousarray(synth.gaussian_taps(9, 1.5), np.float32)
    taps25 = np.ascontiguousarray(synth.gaussian_taps(25, 4.0), np.float32)
    p9, p25 = taps9.ctypes.data_as(C.POINTER(C.c_float)), taps25.ctypes.data_as(C.POINTER(C.c_float))
    c1, c2t9, c16t25 = _lib.matte(1), _lib.matte(2, taps9), _lib.matte(16, taps25)
    for size in args.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        full = (0, 0, w - 1, h - 1)
        shot = km.key_f32(km.green_screen(w, h, 0), km.GREEN, **SHOT)
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

        # (op, call, bytes per pixel, the blur it is compared with)
        ops = [("gain_offset", lambda i: lib.cvs_gain_offset_f16_dev(t16[i % n16].ref(), s16[i % n16].ref(), 1.25, 0.0625, stream), 16, None),
               ("matte_f16_c1", lambda i: lib.cvs_matte_refine_f16_dev(t16[i % n16].ref(), s16[i % n16].ref(), C.byref(c1), stream), 16, None),
               ("matte_f16_c2_t9", lambda i: lib.cvs_matte_refine_f16_dev(t16[i % n16].ref(), s16[i % n16].ref(), C.byref(c2t9), stream), 16, "blur_f16_t9"),
               ("matte_f16_c16_t25", lambda i: lib.cvs_matte_refine_f16_dev(t16[i % n16].ref(), s16[i % n16].ref(), C.byref(c16t25), stream), 16, "blur_f16_t25"),
               ("matte_f32_c2_t9", lambda i: lib.cvs_matte_refine_f32_dev(t32[i % n32].ref(), s32[i % n32].ref(), C.byref(c2t9), stream), 32, None),
               ("blur_f16_t9", lambda i: lib.cvs_fir_blur_f16_dev(t16[i % n16].ref(), s16[i % n16].ref(), p9, 9, stream), 16, None),
               ("blur_f16_t25", lambda i: lib.cvs_fir_blur_f16_dev(t16[i % n16].ref(), s16[i % n16].ref(), p25, 25, stream), 16, None)]
        times = {name: [] for name, _, _, _ in ops}
        for name, call, _, _ in ops:
            for i in range(args.warmup):
                _lib.check(call(i), name)
        _lib.check(lib.cvs_stream_sync(stream), "sync")
        for _ in range(args.rounds):
            for name, call, _, _ in ops:
                lib.cvs_event_record(e0, stream)
                for i in range(args.calls):
                    _lib.check(call(i), name)
                lib.cvs_event_record(e1, stream)
                lib.cvs_event_sync(e1)
                times[name].append(lib.cvs_event_elapsed_ms(e0, e1) / args.calls)
        base = statistics.median(times["gain_offset"])
        margin = (max(times["gain_offset"]) - min(times["gain_offset"])) / base
        for name, _, px, blur in ops:
            ms = statistics.median(times[name])
            line = {"op": name, "size": "%dx%d" % (w, h), "us_per_call": round(ms * 1e3, 2), "us_min": round(min(times[name]) * 1e3, 2),
                    "us_max": round(max(times[name]) * 1e3, 2), "us_rounds": [round(t * 1e3, 2) for t in times[name]],
                    "vs_gain_offset": round(ms / base, 3), "gain_offset_spread": round(margin, 3),
                    "fraction_of_8TBps_on_%dBpx" % px: round(w * h * px / (ms * 1e-3) / PEAK, 3),
                    "frames_f16": n16, "frames_f32": n32, "calls": args.calls}
            if blur:
                line["vs_" + blur] = round(ms / statistics.median(times[blur]), 3)
            print(json.dumps(line), flush=True)
        for f in s16 + t16 + s32 + t32:
            f.free()
    lib.cvs_event_destroy(e0)
    lib.cvs_event_destroy(e1)
    lib.cvs_stream_destroy(stream)


if __name__ == "__main__":
    main()
