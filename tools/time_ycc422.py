#!/usr/bin/env python3
"""HIP-event timing of back-to-back cvs_reconstruct_422_dev and cvs_subsample_422_dev calls (the 4:2:2 Y'CbCr edges, DESIGN.md
4.23) in every layout at 720x486, 1920x1080 and 3840x2160, after warm-up -- and, in the same run, of the MPEG-2 4:2:0 edge of the
same direction and of the frame copy beside them.  One JSON line per case: ms per call, the bytes the call has to move and that
rate as a fraction of 8 TB/s.  Algorithmic bytes per pixel: 8 for the frame plus 2 (planar8, uyvy), 4 (planar10) or 2.67 (v210)
for the samples; the MPEG-2 edges' 9.5; the copy's 16.

Frames and sample buffers each rotate over at least 512 MB so that no call is served from the 256 MiB Infinity Cache.  Import
samples are random bytes, export frames uniform halfs in [0, 1) (every lane's table gather lands on a different entry).  The
MPEG-2 edge takes the raster's height rounded down to a multiple of 4 (720x484 beside 720x486).

Kernel times come from a run of their own under the profiler, one size per run so that a kernel name means one case:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 tools/time_ycc422.py --sizes 1920x1080 --calls 50
    python3 tools/time_ycc422.py --sizes 1920x1080 --calls 50 --summarise DIR/.../*_kernel_trace.csv
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

SIZES = [(720, 486), (1920, 1080), (3840, 2160)]
LAYOUTS = ["planar8", "planar10", "uyvy", "v210"]
SAMPLE_BYTES = {"planar8": 2.0, "planar10": 4.0, "uyvy": 2.0, "v210": 16.0 / 6.0}
PEAK = 8.0e12
ROTATE_BYTES = 512 << 20


def cases(w, h):
    """[(label, bytes moved per call)] in the order the script runs them"""
    h4 = h // 4 * 4
    out = []
    for direction in ("reconstruct", "subsample"):
        out += [("%s %s" % (direction, layout), w * h * (8.0 + SAMPLE_BYTES[layout])) for layout in LAYOUTS]
        out.append(("%s mpeg2 %dx%d" % (direction, w, h4), w * h4 * 9.5))
    out.append(("frame copy", w * h * 16.0))
    return out


def strides_of(lib, layout, w, h):
    s, n = (C.c_int * 3)(), (C.c_int * 3)()
    planes = lib.cvs_ycc422_layout(layout, w, h, s, n)
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
    lib.cvs_event_record(events[0], stream)
    for i in range(args.calls):
        call(i)
    lib.cvs_event_record(events[1], stream)
    lib.cvs_event_sync(events[1])
    ms = lib.cvs_event_elapsed_ms(events[0], events[1]) / args.calls
    print(json.dumps({"case": label, "size": "%dx%d" % size, "ms_per_call": round(ms, 5), "moved_bytes": int(moved),
                      "GBps": round(moved / (ms * 1e-3) / 1e9, 1), "fraction_of_8TBps": round(moved / (ms * 1e-3) / PEAK, 3), "calls": args.calls}), flush=True)


def run_size(lib, stream, events, args, w, h):
    full, h4 = (0, 0, w - 1, h - 1), h // 4 * 4
    rng = np.random.default_rng(w)
    count = max(2, -(-ROTATE_BYTES // (w * h * 8)))
    frames = [DeviceFrame(full, np.uint16) for _ in range(count)]
    codes = rng.uniform(0.0, 1.0, (h, w, 4)).astype(np.float16).view(np.uint16)
    for f in frames:
        f.upload(codes, stream)
    _lib.check(lib.cvs_stream_sync(stream), "sync")
    todo = dict(cases(w, h))
    for direction in ("reconstruct", "subsample"):
        for layout in LAYOUTS:
            lid = LAYOUTS.index(layout)
            strides, lines = strides_of(lib, lid, w, h)
            arena, imgs = sample_sets(lib, stream, strides, lines, rng, direction == "reconstruct")
            if direction == "reconstruct":
                def call(i):
                    _lib.check(lib.cvs_reconstruct_422_dev(frames[i % count].ref(), C.byref(imgs[i % len(imgs)]), w, h, lid, _lib.YCC_REC709, stream), "reconstruct")
            else:
                def call(i):
                    _lib.check(lib.cvs_subsample_422_dev(C.byref(imgs[i % len(imgs)]), frames[i % count].ref(), w, h, lid, _lib.YCC_REC709, stream), "subsample")
            label = "%s %s" % (direction, layout)
            timed(lib, stream, events, args, label, todo[label], (w, h), call)
            _lib.check(lib.cvs_stream_sync(stream), "sync")
            lib.cvs_free(arena)
        arena, imgs = sample_sets(lib, stream, [w, w // 2, w // 2], [h4, h4 // 2, h4 // 2], rng, direction == "reconstruct")
        if direction == "reconstruct":
            def call(i):
                _lib.check(lib.cvs_reconstruct_mpeg2_dev(frames[i % count].ref(), C.byref(imgs[i % len(imgs)]), w, h4, 0, stream), "mpeg2 reconstruct")
        else:
            def call(i):
                _lib.check(lib.cvs_subsample_mpeg2_dev(C.byref(imgs[i % len(imgs)]), frames[i % count].ref(), w, h4, stream), "mpeg2 subsample")
        label = "%s mpeg2 %dx%d" % (direction, w, h4)
        timed(lib, stream, events, args, label, todo[label], (w, h), call)
        _lib.check(lib.cvs_stream_sync(stream), "sync")
        lib.cvs_free(arena)
        for f in frames:                         # (the MPEG-2 reconstruction's raster may be lower: whole frames again)
            f.c.current_window = f.c.full_window

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
    runs = [r for r in runs if len(r[1]) == args.warmup + args.calls]
    want = cases(w, h)
    if len(runs) != len(want):
        sys.exit("%d runs of %d launches in the trace, %d cases: %r" % (len(runs), args.warmup + args.calls, len(want), [r[0][:60] for r in runs]))
    print("# %dx%d: kernel durations from rocprofv3 --kernel-trace (tools/time_ycc422.py --calls %d --warmup %d); per case the %d timed launches;" % (
        w, h, args.calls, args.warmup, args.calls))
    print("# fraction = bytes moved / median / 8 TB/s")
    for (label, moved), (name, ns, shape) in zip(want, runs):
        t = np.array(ns[args.warmup:]) / 1000.0
        med = float(np.median(t))
        print("%-28s median %7.2f us  min %7.2f us  fraction %.3f  %s  %s" % (label, med, t.min(), moved / (med * 1e-6) / PEAK, shape, name.split("(")[0][-70:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
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
