#!/usr/bin/env python3
"""HIP-event timing of back-to-back cvs_reconstruct_420_dev and cvs_subsample_420_dev calls (the 4:2:0 Y'CbCr edges, DESIGN.md
"4:2:0 Y'CbCr edges") in every layout at 1920x1080, 3840x2160 and (import only) 7680x4320, after warm-up -- and, in the same run,
beside them: cvs_reconstruct_mpeg2_dev progressive, cvs_subsample_mpeg2_dev, the planar 4:2:2 edges and the frame copy.  One JSON
line per case and repeat: ms per call, the bytes the call has to move and that rate as a fraction of 8 TB/s.  Algorithmic bytes per
pixel: 8 for the frame plus 1.5 (8-bit 4:2:0, the MPEG-2 edges), 3 (10-bit 4:2:0), 2 or 4 (planar 4:2:2); the copy's 16.

The yardstick of a 4:2:0 layout is the MPEG-2 edge of the same direction scaled by bytes moved (9.5 -> 9.5 or 11 per pixel);
--repeat N runs every case N times, so that the same run shows the spread the yardstick itself has.  --flags takes the CVS_YCC_*
bits of the 4:2:0 calls (default CVS_YCC_REC709 = 2: left siting, studio range, the transfer on).

Frames and sample buffers each rotate over at least 512 MB so that no call is served from the 256 MiB Infinity Cache.  Import
samples are random bytes, export frames uniform halfs in [0, 1) (every lane's table gather lands on a different entry).

Kernel times come from a run of their own under the profiler, one size per run so that a kernel name means one case:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 tools/time_ycc420.py --sizes 1920x1080 --calls 50
    python3 tools/time_ycc420.py --sizes 1920x1080 --calls 50 --summarise DIR/.../*_kernel_trace.csv
--summarise reads the trace, takes the runs of warmup + calls consecutive launches of one kernel in the order of the cases and
prints per case the median and the minimum of the timed launches; this script's own numbers include the launch.
CANVAS_LIB=<path> times another build of the library (an A/B of a kernel variant)."""
import argparse
import csv
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from canvas_amd import _lib  # noqa: E402
from canvas_amd.device import DeviceFrame  # noqa: E402

if os.environ.get("CANVAS_LIB"):                      # A/B runs: another build of the library (never set by the package)
    _lib.LIB_PATH = os.environ["CANVAS_LIB"]

SIZES = [(1920, 1080), (3840, 2160), (7680, 4320)]
IMPORT_ONLY_FROM = 7680 * 4320                         # pixels: no delivery format is this large yet
LAYOUTS = ["planar8", "planar10", "nv12", "p010"]
SAMPLE_BYTES = {"planar8": 1.5, "planar10": 3.0, "nv12": 1.5, "p010": 3.0}
PLANAR_422 = [("planar8", 0, 2.0), ("planar10", 1, 4.0)]
PEAK = 8.0e12
ROTATE_BYTES = 512 << 20


def directions(w, h):
    return ("reconstruct",) if w * h >= IMPORT_ONLY_FROM else ("reconstruct", "subsample")


def cases(w, h):
    """[(label, bytes moved per call)] in the order the script runs them"""
    out = []
    for direction in directions(w, h):
        out += [("%s 420 %s" % (direction, layout), w * h * (8.0 + SAMPLE_BYTES[layout])) for layout in LAYOUTS]
        out.append(("%s mpeg2%s" % (direction, " progressive" if direction == "reconstruct" else ""), w * h * 9.5))
        out += [("%s 422 %s" % (direction, name), w * h * (8.0 + b)) for name, _lid, b in PLANAR_422]
    out.append(("frame copy", w * h * 16.0))
    return out


def strides_of(fn, layout, w, h):
    s, n = (C.c_int * 3)(), (C.c_int * 3)()
    planes = fn(layout, w, h, s, n)
    assert planes > 0, _lib.last_error()
    return list(s)[:planes], list(n)[:planes]


def sample_sets(lib, stream, strides, lines, rng, fill_random):
    """Coded images over one arena, enough of them to cover ROTATE_BYTES; every plane on a 256-byte boundary"""
    sizes = [(s * n + 255) // 256 * 256 for s, n in zip(strides, lines)]
    set_bytes = sum(sizes)
    sets = max(2, -(-ROTATE_BYTES // set_bytes))
    arena = lib.cvs_malloc(sets * set_bytes)
    assert arena, _lib.last_error()
    if fill_random:
        one = rng.integers(0, 256, set_bytes, dtype=np.uint8)
        for i in range(sets):
            _lib.check(lib.cvs_memcpy_h2d(arena + i * set_bytes, one.ctypes.data, one.nbytes, stream), "h2d")
        _lib.check(lib.cvs_stream_sync(stream), "sync")
    imgs = []
    for i in range(sets):
        img, off = _lib.coded_image(), arena + i * set_bytes
        for p, size in enumerate(sizes):
            img.data[p], img.stride[p], img.line_count[p] = off, strides[p], lines[p]
            off += size
        imgs.append(img)
    return arena, imgs


def timed(lib, stream, events, args, label, moved, size, call):
    for i in range(args.warmup):
        call(i)
    _lib.check(lib.cvs_stream_sync(stream), "sync")
    for rep in range(args.repeat):
        lib.cvs_event_record(events[0], stream)
        for i in range(args.calls):
            call(i)
        lib.cvs_event_record(events[1], stream)
        lib.cvs_event_sync(events[1])
        ms = lib.cvs_event_elapsed_ms(events[0], events[1]) / args.calls
        print(json.dumps({"case": label, "size": "%dx%d" % size, "repeat": rep, "ms_per_call": round(ms, 5), "moved_bytes": int(moved),
                          "GBps": round(moved / (ms * 1e-3) / 1e9, 1), "fraction_of_8TBps": round(moved / (ms * 1e-3) / PEAK, 3), "calls": args.calls}),
              flush=True)


def run_size(lib, stream, events, args, w, h):
    full = (0, 0, w - 1, h - 1)
    rng = np.random.default_rng(w)
    count = max(2, -(-ROTATE_BYTES // (w * h * 8)))
    frames = [DeviceFrame(full, np.uint16) for _ in range(count)]
    codes = rng.uniform(0.0, 1.0, (h, w, 4)).astype(np.float16).view(np.uint16)
    for f in frames:
        f.upload(codes, stream)
    _lib.check(lib.cvs_stream_sync(stream), "sync")
    todo = dict(cases(w, h))

    def one(label, strides, lines, direction, recon, sub):
        arena, imgs = sample_sets(lib, stream, strides, lines, rng, direction == "reconstruct")
        if direction == "reconstruct":
            def call(i):
                _lib.check(recon(frames[i % count].ref(), C.byref(imgs[i % len(imgs)])), label)
        else:
            def call(i):
                _lib.check(sub(C.byref(imgs[i % len(imgs)]), frames[i % count].ref()), label)
        timed(lib, stream, events, args, label, todo[label], (w, h), call)
        _lib.check(lib.cvs_stream_sync(stream), "sync")
        lib.cvs_free(arena)

    for direction in directions(w, h):
        for lid, layout in enumerate(LAYOUTS):
            strides, lines = strides_of(lib.cvs_ycc420_layout, lid, w, h)
            one("%s 420 %s" % (direction, layout), strides, lines, direction,
                lambda f, img, lid=lid: lib.cvs_reconstruct_420_dev(f, img, w, h, lid, args.flags, stream),
                lambda img, f, lid=lid: lib.cvs_subsample_420_dev(img, f, w, h, lid, args.flags, stream))
        one("%s mpeg2%s" % (direction, " progressive" if direction == "reconstruct" else ""), [w, w // 2, w // 2], [h, h // 2, h // 2], direction,
            lambda f, img: lib.cvs_reconstruct_mpeg2_dev(f, img, w, h, _lib.YCC_PROGRESSIVE | _lib.YCC_REC709, stream),
            lambda img, f: lib.cvs_subsample_mpeg2_dev(img, f, w, h, stream))
        for name, lid, _b in PLANAR_422:
            strides, lines = strides_of(lib.cvs_ycc422_layout, lid, w, h)
            one("%s 422 %s" % (direction, name), strides, lines, direction,
                lambda f, img, lid=lid: lib.cvs_reconstruct_422_dev(f, img, w, h, lid, _lib.YCC_REC709, stream),
                lambda img, f, lid=lid: lib.cvs_subsample_422_dev(img, f, w, h, lid, _lib.YCC_REC709, stream))

    def copy(i):
        _lib.check(lib.cvs_copy_frame_f16_dev(frames[(i + 1) % count].ref(), frames[i % count].ref(), stream), "copy")
    timed(lib, stream, events, args, "frame copy", todo["frame copy"], (w, h), copy)
    for f in frames:
        f.free()


def summarise(args, w, h):
    """The kernel trace of one run of this script at one size -> per case the median and minimum kernel duration"""
    with open(args.summarise, newline="") as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    runs = []
    for r in rows:
        ns = int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        if runs and runs[-1][0] == r["Kernel_Name"]:
            runs[-1][1].append(ns)
        else:
            runs.append([r["Kernel_Name"], [ns], "%s threads in workgroups of %s" % (r.get("Grid_Size_X", r.get("Grid_Size", "?")), r.get("Workgroup_Size_X", r.get("Workgroup_Size", "?")))])
    launches = args.warmup + args.calls * args.repeat
    runs = [r for r in runs if len(r[1]) == launches]
    want = cases(w, h)
    if len(runs) != len(want):
        sys.exit("%d runs of %d launches in the trace, %d cases: %r" % (len(runs), launches, len(want), [r[0][:60] for r in runs]))
    print("# %dx%d: kernel durations from rocprofv3 --kernel-trace (tools/time_ycc420.py --calls %d --warmup %d --repeat %d); per case the %d timed launches;" % (
        w, h, args.calls, args.warmup, args.repeat, launches - args.warmup))
    print("# fraction = bytes moved / median / 8 TB/s")
    for (label, moved), (name, ns, shape) in zip(want, runs):
        t = np.array(ns[args.warmup:]) / 1000.0
        med = float(np.median(t))
        print("%-34s median %7.2f us  min %7.2f us  fraction %.3f  %s  %s" % (label, med, t.min(), moved / (med * 1e-6) / PEAK, shape, name.split("(")[0][-70:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeat", type=int, default=1, help="timed windows per case: the run-to-run spread in one run")
    ap.add_argument("--flags", type=int, default=2, help="CVS_YCC_* bits of the 4:2:0 calls (default CVS_YCC_REC709)")
    ap.add_argument("--sizes", default=",".join("%dx%d" % s for s in SIZES))
    ap.add_argument("--summarise", metavar="KERNEL_TRACE_CSV", help="summarise the kernel trace of a profiled run at ONE size")
    args = ap.parse_args()
    sizes = [tuple(int(v) for v in s.split("x")) for s in args.sizes.split(",")]
    if args.summarise:
        if len(sizes) != 1:
            ap.error("--summarise takes the one size of the profiled run")
        return summarise(args, *sizes[0])
    lib = _lib.load()
    _lib.check(lib.cvs_init(0), "cvs_init")
    lib.init_half()
    stream = lib.cvs_stream_create()
    events = (lib.cvs_event_create(), lib.cvs_event_create())
    for w, h in sizes:
        run_size(lib, stream, events, args, w, h)
    for e in events:
        lib.cvs_event_destroy(e)
    lib.cvs_stream_destroy(stream)


if __name__ == "__main__":
    main()
