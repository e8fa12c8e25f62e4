#!/usr/bin/env python3
"""HIP-event timing of back-to-back cvs_subsample_mpeg2_dev calls (MPEG-2 4:2:0 subsample) at 720x480, 1920x1080 and
3840x2160, after warm-up.  One JSON line per (size, content): ms per call, the bytes the call has to move (8 B read +
1 + 0.5 B written per source pixel) and that rate as a fraction of 8 TB/s.

The sources rotate over at least 512 MB of device frames so that no call is served from the 256 MiB Infinity Cache.  Two
contents: `random` (uniform halfs in [0, 1): every lane's table gather lands on a different entry) and `layers` (the
bench's synthetic layer frame: smooth).  Kernel times come from a separate run under
`rocprofv3 --kernel-trace --stats -- python3 tools/time_mpeg2.py`; this script's own numbers include the launch.

--table lds | l2 | lds_unstaged runs the diagnostic build (make -C canvas_amd/csrc diag) with that table placement forced:
the table staged into LDS (shipped above a megapixel), gathered from L2 (shipped up to one), or LDS without the staging copy (timing only, wrong pixels:
what staging the table costs).

--reconstruct times cvs_reconstruct_mpeg2_dev instead (the import edge, 4:2:0 planes -> half RGBA): 1.5 B read + 8 B written per
pixel; random planes, two cases per size (interlaced Rec.601, progressive Rec.709); the source planes and the target frames each
rotate over at least 512 MB.  --table lds | l2 forces its table placement in the diagnostic build."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from canvas_amd import _lib, synth  # noqa: E402
from canvas_amd.device import DeviceFrame  # noqa: E402

SIZES = [(720, 480), (1920, 1080), (3840, 2160)]
PEAK = 8.0e12
ROTATE_BYTES = 512 << 20
TABLES = {"lds": 0, "l2": 1, "lds_unstaged": 3}             # kernels/table_placement.hpp kTable*


def time_reconstruct(lib, stream, e0, e1, args, w, h):
    full = (0, 0, w - 1, h - 1)
    strides, lines = (w, w // 2, w // 2), (h, h // 2, h // 2)
    sizes = [s * n for s, n in zip(strides, lines)]
    set_bytes = sum((b + 255) // 256 * 256 for b in sizes)
    sets = max(2, -(-ROTATE_BYTES // set_bytes))
    frames = [DeviceFrame(full, np.uint16) for _ in range(max(2, -(-ROTATE_BYTES // (w * h * 8))))]
    arena = lib.cvs_malloc(sets * set_bytes)
    assert arena, _lib.last_error()
    rng = np.random.default_rng(w)
    one = np.concatenate([np.pad(rng.integers(0, 256, b, dtype=np.uint8), (0, (b + 255) // 256 * 256 - b)) for b in sizes])
    for i in range(sets):
        _lib.check(lib.cvs_memcpy_h2d(arena + i * set_bytes, one.ctypes.data, one.nbytes, stream), "h2d")
    _lib.check(lib.cvs_stream_sync(stream), "sync")
    imgs = []
    for i in range(sets):
        img, off = _lib.coded_image(), arena + i * set_bytes
        for p in range(3):
            img.data[p], img.stride[p], img.line_count[p] = off, strides[p], lines[p]
            off += (sizes[p] + 255) // 256 * 256
        imgs.append(img)
    for name, flags in (("interlaced_601", 0), ("progressive_709", _lib.YCC_PROGRESSIVE | _lib.YCC_REC709)):
        def call(i):
            _lib.check(lib.cvs_reconstruct_mpeg2_dev(frames[i % len(frames)].ref(), C.byref(imgs[i % sets]), w, h, flags, stream), "cvs_reconstruct_mpeg2_dev")

        for i in range(args.warmup):
            call(i)
        _lib.check(lib.cvs_stream_sync(stream), "sync")
        lib.cvs_event_record(e0, stream)
        for i in range(args.calls):
            call(i)
        lib.cvs_event_record(e1, stream)
        lib.cvs_event_sync(e1)
        ms = lib.cvs_event_elapsed_ms(e0, e1) / args.calls
        moved = w * h * 9.5
        print(json.dumps({"op": "reconstruct", "size": "%dx%d" % (w, h), "content": name, "table": args.table or "default", "ms_per_call": round(ms, 5),
                          "moved_bytes": int(moved), "GBps": round(moved / (ms * 1e-3) / 1e9, 1), "fraction_of_8TBps": round(moved / (ms * 1e-3) / PEAK, 3),
                          "sources": sets, "targets": len(frames), "calls": args.calls}), flush=True)
    for f in frames:
        f.free()
    lib.cvs_free(arena)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--sizes", default=",".join("%dx%d" % s for s in SIZES))
    ap.add_argument("--table", choices=sorted(TABLES), help="force a table placement (diagnostic build)")
    ap.add_argument("--reconstruct", action="store_true", help="time cvs_reconstruct_mpeg2_dev (planes -> frame)")
    args = ap.parse_args()
    if args.reconstruct and args.table == "lds_unstaged":
        ap.error("--table lds_unstaged exists for the subsample only")
    if args.table:
        from tools._diag import use_diag_library
        use_diag_library()
        os.environ["CVS_MPEG2_TABLE"] = str(TABLES[args.table])
    lib = _lib.load()
    _lib.check(lib.cvs_init(0), "cvs_init")
    lib.init_half()
    stream = lib.cvs_stream_create()
    e0, e1 = lib.cvs_event_create(), lib.cvs_event_create()
    if args.reconstruct:
        for size in args.sizes.split(","):
            time_reconstruct(lib, stream, e0, e1, args, *(int(v) for v in size.split("x")))
    for size in ([] if args.reconstruct else args.sizes.split(",")):
        w, h = (int(v) for v in size.split("x"))
        full = (0, 0, w - 1, h - 1)
        frame_bytes = w * h * 8
        count = max(2, -(-ROTATE_BYTES // frame_bytes))
        strides, lines = (w, w // 2, w // 2), (h, h // 2, h // 2)
        planes = [lib.cvs_malloc(s * n) for s, n in zip(strides, lines)]
        img = _lib.coded_image()
        for p in range(3):
            img.data[p], img.stride[p], img.line_count[p] = planes[p], strides[p], lines[p]
        rng = np.random.default_rng(w)
        contents = {"random": rng.uniform(0.0, 1.0, (h, w, 4)).astype(np.float16).view(np.uint16),
                    "layers": synth.layer_frame(w, h, 0, 0).array}
        frames = [DeviceFrame(full, np.uint16) for _ in range(count)]
        for name, codes in contents.items():
            for f in frames:
                f.upload(codes, stream)
            _lib.check(lib.cvs_stream_sync(stream), "sync")

            def call(i):
                _lib.check(lib.cvs_subsample_mpeg2_dev(C.byref(img), frames[i % count].ref(), w, h, stream), "cvs_subsample_mpeg2_dev")

            for i in range(args.warmup):
                call(i)
            _lib.check(lib.cvs_stream_sync(stream), "sync")
            lib.cvs_event_record(e0, stream)
            for i in range(args.calls):
                call(i)
            lib.cvs_event_record(e1, stream)
            lib.cvs_event_sync(e1)
            ms = lib.cvs_event_elapsed_ms(e0, e1) / args.calls
            moved = w * h * 9.5
            print(json.dumps({"size": "%dx%d" % (w, h), "content": name, "table": args.table or "default", "ms_per_call": round(ms, 5), "moved_bytes": int(moved),
                              "GBps": round(moved / (ms * 1e-3) / 1e9, 1), "fraction_of_8TBps": round(moved / (ms * 1e-3) / PEAK, 3),
                              "sources": count, "calls": args.calls}), flush=True)
        for f in frames:
            f.free()
        for p in planes:
            lib.cvs_free(p)
    lib.cvs_event_destroy(e0)
    lib.cvs_event_destroy(e1)
    lib.cvs_stream_destroy(stream)


if __name__ == "__main__":
    main()
