#!/usr/bin/env python3
"""A small timeline built from the same `fluggo.media.process` objects the Canvas editor creates
(fluggo/editor/graph/video.py): two clips cut together with a crossfade, a picture-in-picture layer scaled down over
them, a chroma-keyed layer with its matte refined, a title bar on top, one clip graded through a 3D LUT, an RGB parade of the cut in a corner.  Every frame is rendered on the GPU; only the 8-bit preview crosses PCIe.

    python examples/timeline.py [out_dir]        # writes frame_000.png ... (and prints Mpx/s)
"""
import os
import struct
import sys
import time
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fluggo.media import cube, process  # noqa: E402
from fluggo.media.basetypes import box2i  # noqa: E402

W, H, FRAMES = 1280, 720, 60


def write_png(path, rgba, w, h):
    """RGBA8 rows -> PNG (zlib only)."""
    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)
    rows = b"".join(b"\0" + bytes(rgba[y * w * 4:(y + 1) * w * 4]) for y in range(h))
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(rows, 6)) + chunk(b"IEND", b""))

out_dir = sys.argv[1] if len(sys.argv) > 1 else None

assert process.check_context_supported(), process.last_error()


def clip(start, end, gain):
    """A 'clip': a colour that drifts over time, graded (half-native: the gain filter works on f16 frames)."""
    return process.VideoGainOffsetFilter(process.SolidColorVideoSource(process.LerpFunc(start, end, FRAMES)), gain=gain, offset=0.0)


a = clip((0.8, 0.2, 0.1, 1.0), (0.9, 0.6, 0.1, 1.0), 1.0)
b = clip((0.1, 0.3, 0.8, 1.0), (0.1, 0.7, 0.6, 1.0), 1.1)

# clip b is graded: a CDL (slope, offset, power) and a little less saturation, baked into a 17-point cube and looked up on the GPU
def look(r, g, bl):
    r, g, bl = (max(1.1 * r + 0.02, 0.0) ** 0.9, max(1.0 * g, 0.0) ** 0.95, max(0.9 * bl - 0.01, 0.0) ** 1.05)
    y = 0.2126 * r + 0.7152 * g + 0.0722 * bl
    return tuple(y + 0.85 * (c - y) for c in (r, g, bl))


b = process.VideoLut3DFilter(b, process.Lut3D(*cube.lattice_from_function(look, 17)))

# cut + crossfade: a for 20 frames, a -> b over 20 frames (an AnimationFunc drives the mix), b for 20 frames
fade = process.AnimationFunc()
fade.add(process.POINT_LINEAR, 0.0, 0.0)
fade.add(process.POINT_HOLD, 20.0, 1.0)
sequence = process.VideoSequence()
sequence.append((a, 0, 20))
sequence.append((process.VideoMixFilter(src_a=process.VideoPassThroughFilter(a, offset=20), src_b=b, mix_b=fade), 0, 20))
sequence.append((process.VideoPassThroughFilter(b, offset=20), 0, 20))

# picture in picture: clip b at quarter size, placed at (W - 360, 40), half transparent through its gain node's alpha
pip_source = process.VideoGainOffsetFilter(process.SolidColorVideoSource((0.95, 0.95, 0.2, 0.6), box2i(0, 0, W - 1, H - 1)), gain=1.0)
pip = process.VideoScaler(pip_source, target_point=(W - 360, 40), source_point=(0, 0), scale_factors=(0.25, 0.25),
                          source_rect=box2i(0, 0, W - 1, H - 1))
pip = process.VideoUnsharpMaskFilter(pip, process.gaussian_taps(1.0, 5), amount=0.8, threshold=1.0 / 256)    # sharpen what the downscale softened
# a keyed layer: a 'green-screen shot' (a green ground whose colour drifts towards the subject's orange) loses its ground and its spill
shot = process.SolidColorVideoSource(process.LerpFunc((0.08, 0.62, 0.12, 1.0), (0.8, 0.45, 0.1, 1.0), FRAMES), box2i(60, 60, 420, 300))
keyed = process.VideoChromaKeyFilter(shot, key=(0.08, 0.62, 0.12, 1.0), tolerance=0.08, softness=0.25, spill=0.8, spill_range=0.4)
keyed = process.VideoMatteFilter(keyed, choke=1, feather=process.gaussian_taps(1.0))    # take the rim off the matte, soften its edge
title = process.SolidColorVideoSource((0.0, 0.0, 0.0, 0.7), box2i(0, H - 90, W - 1, H - 1))
# a second picture in picture that turns: a card at 40 % size spinning about its own centre, its edges keeping their colour
card = process.SolidColorVideoSource((0.2, 0.85, 0.9, 0.9), box2i(0, 0, 479, 269))
card = process.VideoTransformFilter(card, box2i(0, 0, 479, 269), anchor=(239.5, 134.5), scale=(0.4, 0.4),
                                    rotation=process.LerpFunc((0.0,), (180.0,), FRAMES), position=(160, 120))
# an RGB parade of the cut underneath, picture in picture: 96 columns per panel (288 x 256) from the bytes the preview shows, moved from
# (0, 0), where a scope's picture sits, to the lower right above the title
parade = process.VideoScopeFilter(sequence, "parade", box2i(0, 0, W - 1, H - 1), columns=96, display="widget", gain=1.0 / 64)
parade = process.VideoTransformFilter(parade, box2i(0, 0, 287, 255), position=(W - 300, H - 360))

timeline = process.VideoWorkspace()
timeline.add(source=sequence, x=0, length=FRAMES, z=0, offset=0)
timeline.add(source=pip, x=10, length=40, z=1, offset=0)
timeline.add(source=keyed, x=0, length=FRAMES, z=2, offset=0)
timeline.add(source=title, x=0, length=FRAMES, z=3, offset=0)
timeline.add(source=card, x=0, length=FRAMES, z=4, offset=0)
timeline.add(source=parade, x=0, length=FRAMES, z=5, offset=0)

window = box2i(0, 0, W - 1, H - 1)
timeline.get_frame_rgba8(0, window)                       # first use: tables, code objects
t0 = time.perf_counter()
for i in range(FRAMES):
    rgba, cur = timeline.get_frame_rgba8(i, window)      # sRGB bytes made on the device, 4 B/px downloaded
dt = time.perf_counter() - t0
print("%d frames of %dx%d in %.1f ms: %.0f Mpx/s through the Python surface (preview bytes included)" % (FRAMES, W, H, dt * 1e3, FRAMES * W * H / dt / 1e6))
if out_dir:
    os.makedirs(out_dir, exist_ok=True)
    for i in range(0, FRAMES, 10):
        rgba, cur = timeline.get_frame_rgba8(i, window)
        if rgba is not None:
            write_png(os.path.join(out_dir, "frame_%03d.png" % i), rgba, cur.max.x - cur.min.x + 1, cur.max.y - cur.min.y + 1)
