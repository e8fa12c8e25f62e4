#!/usr/bin/env python3
"""HIP-event timing of the unsharp mask (cvs_unsharp_mask_f16_dev) on device-resident f16 frames at 3840x2160 and 1920x1080,
9 Gaussian taps, in both arithmetic flavours, next to its yardsticks in the same run.  The ops:
    blur                    cvs_fir_blur_f16_dev as the library dispatches it (k_blur_pair, two columns per lane)
    blur_one_column         the same pinned to k_blur (FIR_PATH_ONE_COLUMN): the sweep k_unsharp is built on
    unsharp_fused           cvs_unsharp_mask_f16_dev: k_unsharp, one launch
    unsharp_general_tables  the same call under FIR_PATH_TABLES: the mask's general path, that is the TABLE blur kernel
                            (k_fir_hv / k_fir2d) into a pooled f32 frame, then k_unsharp_combine
    blur_tables             the blur alone under the same pin, f16 -> f16: what of the line above is the table blur
The general path over the register-window blur (k_blur into an f32 frame + k_unsharp_combine) is not timed: every tap list that
k_blur takes and k_unsharp does not is outside "9 taps", and no pin sends a 9-tap list that way.
One JSON line per (op, size, flavour): microseconds per call (median round, and every round), the algorithmic bytes (8 B read +
8 B written per pixel) over that time as a fraction of 8 TB/s, and the ratio to `blur` of the same run.

--lib PATH times another build of the library (the parent commit's, for the A/B of the blur): only the ops that build has.
Sources and targets rotate over at least 512 MB of device frames so that no call is served from the 256 MiB Infinity Cache; the
rounds alternate the ops so that a drift of the machine shows in all of them.  Kernel times come from a separate run under
`rocprofv3 --kernel-trace --stats -- python3 tools/time_unsharp.py`; this script's own numbers include the launch."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from canvas_amd import _lib, synth  # noqa: E402

SIZES = [(3840, 2160), (1920, 1080)]
PEAK = 8.0e12
ROTATE_BYTES = 512 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--ntaps", type=int, default=9)
    ap.add_argument("--sigma", type=float, default=1.5)
    ap.add_argument("--sizes", default=",".join("%dx%d" % s for s in SIZES))
    ap.add_argument("--lib", default=None, help="time this libcanvas_hip.so instead of the package's")
    args = ap.parse_args()
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
        other = C.CDLL(_lib.LIB_PATH)
        for name in [n for n in _lib.SIGNATURES if not hasattr(other, n)]:      # an older build: bind what it exports
            del _lib.SIGNATURES[name]
    from canvas_amd.device import DeviceFrame
    lib = _lib.load()
    _lib.check(lib.cvs_init(0), "cvs_init")
    lib.init_half()
    has_unsharp = hasattr(C.CDLL(_lib.LIB_PATH), "cvs_unsharp_mask_f16_dev")
    stream = lib.cvs_stream_create()
    e0, e1 = lib.cvs_event_create(), lib.cvs_event_create()
    taps = np.ascontiguousarray(synth.gaussian_taps(args.ntaps, args.sigma), np.float32)
    tp = taps.ctypes.data_as(C.POINTER(C.c_float))
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

        def blur(i):
            return lib.cvs_fir_blur_f16_dev(targets[i % count].ref(), sources[i % count].ref(), tp, len(taps), stream)

        def unsharp(i):
            return lib.cvs_unsharp_mask_f16_dev(targets[i % count].ref(), sources[i % count].ref(), tp, len(taps), 1.5, 2.0 ** -6, stream)

        def pinned(call, pin):
            def run(i):
                lib.cvs_fir_path_override(pin)
                try:
                    return call(i)
                finally:
                    lib.cvs_fir_path_override(_lib.FIR_PATH_AUTO)
            return run

        # (op, call, the cvs_fir_last_kernel() it must report)
        ops = [("blur", blur, _lib.FIR_KERNEL_WINDOW_PAIR), ("blur_one_column", pinned(blur, _lib.FIR_PATH_ONE_COLUMN), _lib.FIR_KERNEL_WINDOW)]
        if has_unsharp:
            ops += [("unsharp_fused", unsharp, _lib.FIR_KERNEL_UNSHARP), ("unsharp_general_tables", pinned(unsharp, _lib.FIR_PATH_TABLES), None),
                    ("blur_tables", pinned(blur, _lib.FIR_PATH_TABLES), None)]
        for flavour, mode in (("separate", _lib.ARITH_SEPARATE), ("contracted", _lib.ARITH_CONTRACTED)):
            lib.cvs_set_arithmetic(mode)
            times = {name: [] for name, _, _ in ops}
            kernels = {}
            for name, call, want in ops:
                for i in range(args.warmup):
                    _lib.check(call(i), name)
                kernels[name] = lib.cvs_fir_last_kernel()
                if want is not None and kernels[name] != want:
                    raise SystemExit("%s went to kernel %d, not %d" % (name, kernels[name], want))
            _lib.check(lib.cvs_stream_sync(stream), "sync")
            for _ in range(args.rounds):
                for name, call, _ in ops:
                    lib.cvs_event_record(e0, stream)
                    for i in range(args.calls):
                        _lib.check(call(i), name)
                    lib.cvs_event_record(e1, stream)
                    lib.cvs_event_sync(e1)
                    times[name].append(lib.cvs_event_elapsed_ms(e0, e1) / args.calls)
            base = statistics.median(times["blur"])
            for name, _, _ in ops:
                ms = statistics.median(times[name])
                moved = w * h * 16
                print(json.dumps({"op": name, "size": "%dx%d" % (w, h), "flavour": flavour, "ntaps": len(taps), "kernel": kernels[name],
                                  "us_per_call": round(ms * 1e3, 2), "us_rounds": [round(t * 1e3, 2) for t in times[name]],
                                  "vs_blur": round(ms / base, 3), "fraction_of_8TBps_on_16Bpx": round(moved / (ms * 1e-3) / PEAK, 3),
                                  "frames": count, "calls": args.calls, "lib": os.path.relpath(_lib.LIB_PATH)}), flush=True)
        lib.cvs_set_arithmetic(_lib.ARITH_SEPARATE)
        for f in sources + targets:
            f.free()
    lib.cvs_event_destroy(e0)
    lib.cvs_event_destroy(e1)
    lib.cvs_stream_destroy(stream)


if __name__ == "__main__":
    main()
