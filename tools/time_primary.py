#!/usr/bin/env python3
"""HIP-event timing of the primary colour corrector (cvs_primary_f16_dev / _f32_dev) on device-resident 3840x2160 frames, next to
four yardsticks on the same frames in the same alternating rounds:
    gain_offset     cvs_gain_offset_f16_dev: the same 8 B read + 8 B written per pixel, no table
    copy            cvs_copy_frame_f16_dev
    color_matrix    cvs_color_matrix_f16_to_dev with both transfer tables: the nearest function the library had (3 x 3 matrix, one
                    half -> half table for all channels on either side)
    lut3d_17        cvs_lut3d_f16_dev at N = 17, the other LDS-staged gather
The corrector's configurations: pre only, matrix only, pre + matrix + post, the curves at K = 1025 and K = 4097 (a linear -> Rec.709
and a Rec.709 -> linear curve with a little noise in every node), in f16 and in f32.  Three contents:
    noise   uniform random colours: the 64 lanes of a wave hit 64 different nodes of every table, the worst case for the LDS banks
    ramp    a horizontal ramp: neighbouring lanes hit the same or neighbouring nodes
    flat    one colour: every lane reads the same two nodes
One JSON line per (op, content): microseconds per call (median round, min, max, and every round), the frame's algorithmic bytes
(16 B per pixel on f16 frames, 32 on f32; tables not counted) over the median as a fraction of 8 TB/s, the ratios to gain_offset
and to the copy of the same run, and the copy's and gain_offset's own min-max spreads relative to their medians beside them: the
margin within which "costs the same" is meant.

Sources and targets rotate over more than 256 MiB of device frames each so that no call is served from the 256 MiB Infinity
Cache; the rounds alternate the ops so that a drift of the machine shows in all of them.  The numbers include the launch.
CANVAS_LIB=<path> times another build of the library (an A/B of a kernel variant)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from canvas_amd import _lib  # noqa: E402
from fluggo.media import grade  # noqa: E402
from tests import lut3d_model as lm  # noqa: E402
from tests.models import f2h_rz_model  # noqa: E402

if os.environ.get("CANVAS_LIB"):
    _lib.LIB_PATH = os.path.abspath(os.environ["CANVAS_LIB"])

W, H = 3840, 2160
PEAK = 8.0e12
ROTATE_BYTES = 288 << 20
SIZES = [1025, 4097]
CONTENTS = ["noise", "ramp", "flat"]
MATRIX = grade.saturation_matrix(0.8)
MATRIX[3], MATRIX[7], MATRIX[11] = 0.01, -0.01, 0.005


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


def curves(lib, name, size):
    """a transfer curve with a little noise in every node -> its device form"""
    table = np.array(grade.transfer_curves(name, size), np.float32)
    table += np.random.default_rng(size).uniform(-0.002, 0.002, table.shape).astype(np.float32)
    planar = np.ascontiguousarray(table.T).reshape(-1)
    dev = lib.cvs_malloc(planar.nbytes)
    assert dev, _lib.last_error()
    _lib.check(lib.cvs_memcpy_h2d(dev, planar.ctypes.data, planar.nbytes, None), "h2d")
    return dev


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--contents", default=",".join(CONTENTS))
    ap.add_argument("--sizes", default=",".join(str(n) for n in SIZES))
    args = ap.parse_args()
    from canvas_amd.device import DeviceFrame
    lib = _lib.load()
    _lib.check(lib.cvs_init(0), "cvs_init")
    lib.init_half()
    stream = lib.cvs_stream_create()
    e0, e1 = lib.cvs_event_create(), lib.cvs_event_create()
    full = (0, 0, W - 1, H - 1)
    sizes = [int(n) for n in args.sizes.split(",")]
    held = []
    configs = []                                                          # (name, params, pre, post)
    for k in sizes:
        pre, post = curves(lib, "rec709_to_linear_scene", k), curves(lib, "linear_to_rec709", k)
        held += [pre, post]
        configs.append(("pre_%d" % k, _lib.primary(k), pre, None))
        configs.append(("pre_matrix_post_%d" % k, _lib.primary(k, MATRIX, k), pre, post))
    configs.insert(0, ("matrix", _lib.primary(None, MATRIX), None, None))
    lat = (lm.identity(17) + np.random.default_rng(17).uniform(-0.02, 0.02, (17, 17, 17, 3)).astype(np.float32)).astype(np.float32)
    flat = lm.packed(lat)
    lattice = lib.cvs_malloc(flat.nbytes)
    assert lattice, _lib.last_error()
    _lib.check(lib.cvs_memcpy_h2d(lattice, flat.ctypes.data, flat.nbytes, None), "h2d")
    held.append(lattice)
    lp = _lib.lut3d(17)
    m9 = (C.c_float * 9)(*[MATRIX[4 * r + c] for r in range(3) for c in range(3)])
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
        ops = [("gain_offset", lambda i: lib.cvs_gain_offset_f16_dev(t16[i % n16].ref(), s16[i % n16].ref(), 1.25, 0.0625, stream), 16),
               ("copy", lambda i: lib.cvs_copy_frame_f16_dev(t16[i % n16].ref(), s16[i % n16].ref(), stream), 16),
               ("color_matrix", lambda i: lib.cvs_color_matrix_f16_to_dev(t16[i % n16].ref(), s16[i % n16].ref(), m9, _lib.LUT_REC709_TO_LINEAR_SCENE, _lib.LUT_LINEAR_TO_REC709, stream), 16),
               ("lut3d_17", lambda i: lib.cvs_lut3d_f16_dev(t16[i % n16].ref(), s16[i % n16].ref(), lattice, C.byref(lp), stream), 16)]
        for cname, p, pre, post in configs:
            ops.append(("primary_f16_" + cname, lambda i, p=p, pre=pre, post=post: lib.cvs_primary_f16_dev(t16[i % n16].ref(), s16[i % n16].ref(), C.byref(p), pre, post, stream), 16))
        for cname, p, pre, post in configs:
            ops.append(("primary_f32_" + cname, lambda i, p=p, pre=pre, post=post: lib.cvs_primary_f32_dev(t32[i % n32].ref(), s32[i % n32].ref(), C.byref(p), pre, post, stream), 32))
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
        base, copy = statistics.median(times["gain_offset"]), statistics.median(times["copy"])
        margin = (max(times["gain_offset"]) - min(times["gain_offset"])) / base
        copy_margin = (max(times["copy"]) - min(times["copy"])) / copy
        for op, _, px in ops:
            ms = statistics.median(times[op])
            print(json.dumps({"op": op, "content": name, "size": "%dx%d" % (W, H), "us_per_call": round(ms * 1e3, 2), "us_min": round(min(times[op]) * 1e3, 2),
                              "us_max": round(max(times[op]) * 1e3, 2), "us_rounds": [round(t * 1e3, 2) for t in times[op]],
                              "spread": round((max(times[op]) - min(times[op])) / ms, 3), "vs_gain_offset": round(ms / base, 3), "vs_copy": round(ms / copy, 3),
                              "gain_offset_spread": round(margin, 3), "copy_spread": round(copy_margin, 3),
                              "fraction_of_8TBps_on_%dBpx" % px: round(W * H * px / (ms * 1e-3) / PEAK, 3),
                              "frames_f16": n16, "frames_f32": n32, "calls": args.calls}), flush=True)
    for f in s16 + t16 + s32 + t32:
        f.free()
    for dev in held:
        lib.cvs_free(dev)
    lib.cvs_event_destroy(e0)
    lib.cvs_event_destroy(e1)
    lib.cvs_stream_destroy(stream)


if __name__ == "__main__":
    main()
