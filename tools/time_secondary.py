#!/usr/bin/env python3
"""HIP-event timing of the secondaries (cvs_qualify_f16_dev / _f32_dev, cvs_matte_mix_f16_dev / _f32_dev) on device-resident frames
at 3840x2160 and 1920x1080, on noise, a ramp and a flat frame, next to the three existing entries their bytes are measured
against, on the same frames in the same alternating rounds:
    copy            cvs_copy_frame_f16_dev                  8 B read + 8 B written per pixel: the frame copy
    key             cvs_chroma_key_f16_dev, no spill        16 B/px: what the qualifier without a key frame should cost
    key_again       the same call once more in every round: its medians against `key`'s are the run's own spread
    cross           cvs_mix_cross_f16_dev                   24 B/px: the mix through a matte moves 32, so 32/24 of this
    qual_hue        the qualifier, hue alone                16 B/px
    qual_all        the qualifier, all three axes           16 B/px (two divides per pixel)
    qual_key        all three axes, a distinct key frame    24 B/px
    mmix            the mix through a matte, by alpha       32 B/px
    mmix_luma       the mix through a matte, by luma        32 B/px
    qual_all_f32, mmix_f32                                  the same on f32 frames: 32 and 64 B/px
One JSON line per (op, picture, size): microseconds per call (median round, min, max, every round), the algorithmic bytes over the
median as a fraction of 8 TB/s, the ratio to `key` of the same run and to the expectation by bytes (key x bytes / 16 for the
qualifier, cross x 32 / 24 for the mix), and `key_spread`: |key_again - key| / key and key's own (max - min) / median, whichever is
larger -- the margin within which "costs what its bytes cost" is meant.  The lines are also written to
profiles/secondary/time_secondary.jsonl (--out).

Sources and targets rotate over more than 256 MiB of device frames each so that no call is served from the 256 MiB Infinity
Cache; the rounds alternate the ops so that a drift of the machine shows in all of them.  The numbers include the launch."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from canvas_amd import _lib  # noqa: E402
from tests.models import f2h_rz_model  # noqa: E402

SIZES = [(3840, 2160), (1920, 1080)]
PEAK = 8.0e12
ROTATE_BYTES = 288 << 20
ALL = dict(hue=(350.0, 40.0, 20.0), saturation=(0.2, float("inf"), 0.1, 0.0), luma=(0.1, 0.9, 0.05, 0.1))


def picture(kind, w, h, seed):
    """(h, w, 4) f32: uniform noise, a ramp of hue along x and value along y, or one flat colour"""
    if kind == "noise":
        return np.random.default_rng(seed).uniform(0.0, 1.0, (h, w, 4)).astype(np.float32)
    out = np.empty((h, w, 4), np.float32)
    if kind == "flat":
        out[...] = (0.25, 0.5, 0.75, 0.5)
        return out
    x = np.linspace(0.0, 1.0, w, dtype=np.float32)[None, :]
    y = np.linspace(0.0, 1.0, h, dtype=np.float32)[:, None]
    out[..., 0], out[..., 1], out[..., 2], out[..., 3] = x * y, (1 - x) * y, np.abs(2 * x - 1) * y, x * np.ones_like(y)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", default=",".join("%dx%d" % s for s in SIZES))
    ap.add_argument("--pictures", default="noise,ramp,flat")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "secondary", "time_secondary.jsonl"))
    args = ap.parse_args()
    from canvas_amd.device import DeviceFrame
    lib = _lib.load()
    _lib.check(lib.cvs_init(0), "cvs_init")
    lib.init_half()
    stream = lib.cvs_stream_create()
    e0, e1 = lib.cvs_event_create(), lib.cvs_event_create()
    plain = _lib.chroma_key((C.c_float * 3)(0.1, 0.8, 0.15), 0.08, 0.25, 0.0, 0.0, 0)
    hue, every = _lib.qualifier(hue=ALL["hue"]), _lib.qualifier(**ALL)
    by_alpha, by_luma = _lib.matte_mix(), _lib.matte_mix(luma=True)
    lines = []
    for size in args.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        full = (0, 0, w - 1, h - 1)
        n16, n32 = max(3, -(-ROTATE_BYTES // (w * h * 8))), max(3, -(-ROTATE_BYTES // (w * h * 16)))
        # three sets of inputs and one of targets per format; the pictures are uploaded into them in turn
        a16, b16, m16, t16 = ([DeviceFrame(full, np.uint16) for _ in range(n16)] for _ in range(4))
        a32, b32, m32, t32 = ([DeviceFrame(full, np.float32) for _ in range(n32)] for _ in range(4))
        for kind in args.pictures.split(","):
            for k, (set16, set32) in enumerate(((a16, a32), (b16, b32), (m16, m32))):
                pixels = picture(kind, w, h, k)
                codes = f2h_rz_model(pixels)
                for f in set16:
                    f.upload(codes, stream)
                for f in set32:
                    f.upload(pixels, stream)
            _lib.check(lib.cvs_stream_sync(stream), "sync")
            key = lambda i: lib.cvs_chroma_key_f16_dev(t16[i % n16].ref(), a16[i % n16].ref(), C.byref(plain), stream)      # noqa: E731
            # (op, call, bytes per pixel, what its bytes are measured against and by what factor)
            ops = [("copy", lambda i: lib.cvs_copy_frame_f16_dev(t16[i % n16].ref(), a16[i % n16].ref(), stream), 16, None),
                   ("key", key, 16, None),
                   ("cross", lambda i: lib.cvs_mix_cross_f16_dev(t16[i % n16].ref(), a16[i % n16].ref(), b16[i % n16].ref(), 0.3, stream), 24, None),
                   ("qual_hue", lambda i: lib.cvs_qualify_f16_dev(t16[i % n16].ref(), a16[i % n16].ref(), None, C.byref(hue), stream), 16, ("key", 1.0)),
                   ("qual_all", lambda i: lib.cvs_qualify_f16_dev(t16[i % n16].ref(), a16[i % n16].ref(), None, C.byref(every), stream), 16, ("key", 1.0)),
                   ("qual_key", lambda i: lib.cvs_qualify_f16_dev(t16[i % n16].ref(), a16[i % n16].ref(), b16[i % n16].ref(), C.byref(every), stream), 24, ("key", 1.5)),
                   ("mmix", lambda i: lib.cvs_matte_mix_f16_dev(t16[i % n16].ref(), a16[i % n16].ref(), b16[i % n16].ref(), m16[i % n16].ref(), C.byref(by_alpha), stream), 32, ("cross", 32 / 24)),
                   ("mmix_luma", lambda i: lib.cvs_matte_mix_f16_dev(t16[i % n16].ref(), a16[i % n16].ref(), b16[i % n16].ref(), m16[i % n16].ref(), C.byref(by_luma), stream), 32, ("cross", 32 / 24)),
                   ("key_again", key, 16, None),
                   ("qual_all_f32", lambda i: lib.cvs_qualify_f32_dev(t32[i % n32].ref(), a32[i % n32].ref(), None, C.byref(every), stream), 32, ("key", 2.0)),
                   ("mmix_f32", lambda i: lib.cvs_matte_mix_f32_dev(t32[i % n32].ref(), a32[i % n32].ref(), b32[i % n32].ref(), m32[i % n32].ref(), C.byref(by_alpha), stream), 64, ("cross", 64 / 24))]
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
            med = {name: statistics.median(t) for name, t in times.items()}
            spread = max(abs(med["key_again"] - med["key"]) / med["key"], (max(times["key"]) - min(times["key"])) / med["key"])
            for name, _, px, against in ops:
                ms = med[name]
                line = {"op": name, "picture": kind, "size": "%dx%d" % (w, h), "us_per_call": round(ms * 1e3, 2), "us_min": round(min(times[name]) * 1e3, 2),
                        "us_max": round(max(times[name]) * 1e3, 2), "us_rounds": [round(t * 1e3, 2) for t in times[name]], "bytes_per_pixel": px,
                        "fraction_of_8TBps": round(w * h * px / (ms * 1e-3) / PEAK, 3), "vs_key": round(ms / med["key"], 3), "key_spread": round(spread, 3),
                        "frames_f16": n16, "frames_f32": n32, "calls": args.calls}
                if against:
                    line["expected_by_bytes"] = "%s x %.3f" % against
                    line["vs_expected"] = round(ms / (med[against[0]] * against[1]), 3)
                lines.append(json.dumps(line))
                print(lines[-1], flush=True)
        for f in a16 + b16 + m16 + t16 + a32 + b32 + m32 + t32:
            f.free()
    lib.cvs_event_destroy(e0)
    lib.cvs_event_destroy(e1)
    lib.cvs_stream_destroy(stream)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
