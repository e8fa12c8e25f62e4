"""The catalogue of device-entry calls by EXTENT: windows taller or wider than any picture (DESIGN.md "Extents").

tests/entry_cases.py fixes the geometry of its cases; here a builder takes it: build(cvs, width, height) -> [(what, case), ...],
each case(fac) one call on operands from a factory, as that module's conventions have it -- pixels from px16 / px32 with their
special values, targets from blank() with a sentinel in every pixel, every explicit box through fac.box(), the stream
fac.stream.  Per group the windows are the whole buffer and one window that starts at an odd column and ends one row short of
the buffer, so that a launcher that writes one row too many is seen.  The shapes are the smallest that cross each line of the
launch arithmetic: what is under test is how a launcher folds rows and columns into its grid, not throughput.

GROUPS lists every group with the extents it runs at; tests/test_extents_cpu.py holds it to the headers and proves the
expectations on the reference side (tests/reference_library.py), tests/test_extents_gpu.py runs it in a guarded arena.

Not in this catalogue: the DV pair (cvs_reconstruct_dv_dev, cvs_subsample_dv_dev) -- the DV raster is fixed at 720 x 480, so
those two entries have no extent to vary -- and the five flat-array entries, which have no window.

The entries of the extension headers are here too, on the operands of their own catalogues (tests/deinterlace_cases.py,
temporal_cases.py, perspective_cases.py, ycc422_cases.py, ycc420_cases.py; thin groups over median_cases.py, primary_cases.py and
secondary_cases.py), at the lines of their launchers: rowstream::shape with `made` lanes for the row-stream pair, warp::launch_bands
for the corner pin, cvs::plan_strips and table_grid for the edges.

One line stays without a case: plan_strips refuses a launch of more than 2^31 - 2^20 units (runs per row times rows of units),
the margin its kernels' `int u += stride` walk needs.  With coordinates within 2^30 that takes a raster of hundreds of
gigapixels -- at the 126 columns of a run and one row of units per row, 2^31 units are 270 gigapixels, some two terabytes of
half pixels -- which no buffer a test can hold reaches.  The refusal is read, not run."""
import ctypes as C
import functools

import numpy as np

from canvas_amd import _lib
from canvas_amd.abi import HostFrame, box2i
from tests import deinterlace_cases as dc
from tests import deinterlace_model as dm
from tests import entry_cases as ec
from tests import median_cases as mdc
from tests import median_model as mdm
from tests import primary_cases as prc
from tests import secondary_cases as sec
from tests import temporal_cases as tc
from tests import temporal_model as tpm
from tests import ycc420_cases as y420
from tests import ycc420_model as y420m
from tests import ycc422_cases as y422
from tests import ycc422_model as y422m
from tests.entry_cases import blank, px, px16, px32
from tests.util import f32p

# width x height
AT_16_BITS = [(2, 65535), (2, 65536), (3, 70001)]          # grid.y = rows at and past 16 bits; k_unsharp_combine's cap of 32 768
WIDE = [(70001, 3), (131073, 2)]                           # widths nothing had run
WEAVE_ROWS = [(2, 131075)]                                 # the weave launches rows / 2
TRANSFORM_ROWS = [(1, 524280), (1, 524281), (1, 524320)]   # 65 535 tiles of 8 rows; the first row of the next tile; five tiles more
MATTE_ROWS = [(1, 2097120), (1, 2097121), (1, 2097221)]    # 65 535 tiles of 32 rows; one row more; four tiles more
STREAM_ROWS = [(1, 4194305)]                               # more than 65 535 segments of kMaxSeg = 64 rows (stream_common.hpp)
# a 1.1 M-row target of the enlarging scaler.  Pinned to the tiles it still runs on the strips of k_fir_vh: k_fir_tile_vh takes no
# target narrower than 256 columns, so its own grid.y cannot pass 65 535 segments below a 2 GB target, which no test here holds
SCALER_ROWS = [(2, 1100000)]

# Cases (by the start of their name) whose result is defined inside the reported window only, as tests/test_gpu_parity.py
# compares them: the scaler between half frames, the crossfade of halfs, the chain, blur + over, the workspace stack.
WINDOW_ONLY = ("scale f16", "scale batch f16", "cross f16", "chain, ", "blur over ", "workspace stack")
EXEMPT = {"cvs_reconstruct_dv_dev": "the DV raster is fixed at 720 x 480", "cvs_subsample_dv_dev": "the DV raster is fixed at 720 x 480"}


def windows(width, height):
    """[(name, full window, current window)]: the whole buffer; from an odd column to one row short of the buffer.  From
    2^19 rows on (one column wide, at a launcher's own line) the whole buffer alone: a row too many then lands in a guard."""
    full = (0, 0, width - 1, height - 1)
    if height >= 1 << 19:
        return [("whole", full, full)]
    return [("whole", full, full), ("inset", full, (1 if width > 1 else 0, 0, width - 1, max(height - 2, 0)))]


def _name(what, width, height, wname):
    return "%s, %d x %d, %s" % (what, width, height, wname)


# ------------------------------------------------------------------ copies, conversions, fills, gain, colour

def copies_and_conversions(cvs, width, height):
    cases = []
    for wname, full, cur in windows(width, height):
        def make(entry, out_half, in_half, cmp, extra=(), full=full, cur=cur, wname=wname):
            def case(fac):
                src = fac.frame(px(np.random.default_rng(2100), in_half, full, cur))
                out = fac.frame(blank(out_half, full), out=True, cmp=cmp)
                return getattr(cvs, entry)(out.ref(), src.ref(), *extra, fac.stream)
            return (_name(entry, width, height, wname), case)
        cases += [make("cvs_copy_frame_f16_dev", True, True, "exact"),
                  make("cvs_copy_frame_alpha_f32_dev", False, False, "f32", (C.c_float(0.4),)),
                  make("cvs_frame_f16_to_f32_dev", False, True, "f32"),
                  make("cvs_frame_f32_to_f16_dev", True, False, "f16"),
                  make("cvs_gain_offset_f16_dev", True, True, "f16", (C.c_float(1.5), C.c_float(0.0625)))]
    return cases


def attenuate_in_place(cvs, width, height):
    cases = []
    for wname, full, cur in windows(width, height):
        def case(fac, full=full, cur=cur):
            f = fac.frame(px32(np.random.default_rng(2150), full, cur), out=True, cmp="f32", in_place=True)
            return cvs.cvs_copy_frame_alpha_f32_dev(f.ref(), f.ref(), C.c_float(0.4), fac.stream)
        cases.append((_name("attenuate in place", width, height, wname), case))
    return cases


def solid_fills(cvs, width, height):
    color = _lib.rgba_f32(1.0, 0.5, 0.333333, 0.2)
    cases = []
    everywhere = (ec.INT_MIN, ec.INT_MIN, ec.INT_MAX, ec.INT_MAX)
    for wname, full, win in windows(width, height) + [("everywhere", (0, 0, width - 1, height - 1), everywhere)]:
        for half in (True, False):
            def case(fac, full=full, win=win, half=half):
                f = fac.frame(blank(half, full), out=True)
                b = box_of(fac, win)
                entry = cvs.cvs_fill_solid_f16_dev if half else cvs.cvs_fill_solid_f32_dev
                return entry(f.ref(), C.byref(b), C.byref(color), fac.stream)
            cases.append((_name("fill %s" % ("f16" if half else "f32"), width, height, wname), case))
    return cases


def box_of(fac, win):
    """fac.box() for a window inside the bound; "everywhere" is what it is wherever the frames lie."""
    if win[0] == ec.INT_MIN:
        return box2i.of(*win)
    return fac.box(*win)


def colour_matrix(cvs, width, height, pre, post):
    m = np.array(ec.REC709_RGB_TO_YPBPR, np.float32)
    cases = []
    for wname, full, cur in windows(width, height):
        def in_place(fac, full=full, cur=cur):
            f = fac.frame(px16(np.random.default_rng(2300), full, cur), out=True, cmp="f16", in_place=True)
            return cvs.cvs_color_matrix_f16_dev(f.ref(), f32p(m), pre, post, fac.stream)

        def to(fac, full=full, cur=cur):
            src = fac.frame(px16(np.random.default_rng(2301), full, cur))
            out = fac.frame(blank(True, full), out=True, cmp="f16")
            return cvs.cvs_color_matrix_f16_to_dev(out.ref(), src.ref(), f32p(m), pre, post, fac.stream)
        cases += [(_name("colour matrix in place", width, height, wname), in_place), (_name("colour matrix out of place", width, height, wname), to)]
    return cases


# ------------------------------------------------------------------ mixers, weave

def mixers_f32(cvs, width, height):
    """The lower frame's window is the buffer, the upper one's starts at an odd column in the last rows: the two overlap in the
    buffer's last rows, up to its last pixel."""
    full = (0, 0, width - 1, height - 1)
    pw, qw = full, (1, max(1, height - 3), width - 1, height - 1)

    def over(fac):
        rng = np.random.default_rng(2400)
        out = fac.frame(px32(rng, full, pw), out=True, cmp="f32", in_place=True)
        upper = fac.frame(px32(rng, full, qw))
        return cvs.cvs_mix_over_f32_dev(out.ref(), upper.ref(), C.c_float(0.35), fac.stream)

    def cross(fac):
        rng = np.random.default_rng(2450)
        a, b = fac.frame(px32(rng, full, pw)), fac.frame(px32(rng, full, qw))
        out = fac.frame(blank(False, full), out=True, cmp="f32")
        return cvs.cvs_mix_cross_f32_dev(out.ref(), a.ref(), b.ref(), C.c_float(0.2), fac.stream)
    return [(_name("mix over", width, height, "last rows"), over), (_name("mix cross", width, height, "last rows"), cross)]


def weave_fields(cvs, width, height):
    cases = []
    for wname, full, cur in windows(width, height):
        def case(fac, full=full, cur=cur):
            rng = np.random.default_rng(2200)
            frame = fac.frame(px16(rng, full, cur), out=True, in_place=True)
            other = fac.frame(px16(rng, cur, cur))
            return cvs.cvs_weave_fields_f16_dev(frame.ref(), other.ref(), fac.stream)
        cases.append((_name("weave", width, height, wname), case))
    return cases


def mix_cross_f16(cvs, width, height):
    """Whole windows (one fused launch) and the mixers' windows (node by node through pooled f32 frames)."""
    full = (0, 0, width - 1, height - 1)
    cases = []
    for wname, pw, qw in [("whole", full, full), ("last rows", full, (1, max(1, height - 3), width - 1, height - 1))]:
        def case(fac, pw=pw, qw=qw):
            rng = np.random.default_rng(2500)
            a, b = fac.frame(px16(rng, full, pw)), fac.frame(px16(rng, full, qw))
            out = fac.frame(blank(True, full), out=True, cmp="f16")
            return cvs.cvs_mix_cross_f16_dev(out.ref(), a.ref(), b.ref(), C.c_float(0.3), fac.stream)
        cases.append((_name("cross f16", width, height, wname), case))
    return cases


# ------------------------------------------------------------------ the chain, blur + over

def _ragged(width, height):
    """Windows of the upper layers of a ragged stack: their min.y above zero, so that video_mix.c:265's `left` selector (min.x
    compared with the other frame's min.Y) picks the geometrically left frame, as tests/test_gpu_parity.py chooses them."""
    return [(1, 1, width - 1, max(height - 2, 1)), (0, max(height - 3, 1), width - 2, height - 1)]


def chain(cvs, width, height):
    """1, 4 and 8 layers in one job each, a batch of two jobs with both tables, and a ragged job, which goes node by node."""
    m = np.array(ec.REC709_RGB_TO_YPBPR, np.float32)
    full = (0, 0, width - 1, height - 1)

    def make(what, njobs, nlayers, pre, post, windows=None):
        def case(fac):
            jobs = (_lib.chain_job * njobs)()
            for j in range(njobs):
                layers = [ec.synth.layer_frame(width, height, k, j) for k in range(nlayers)]
                for k, win in enumerate(windows or ()):
                    layers[k + 1] = ec.HostFrame(full, np.uint16, layers[k + 1].array, win)
                dl = [fac.frame(l, name="job %d layer %d" % (j, k)) for k, l in enumerate(layers)]
                out = fac.frame(blank(True, full), out=True, cmp="f16", name="job %d output" % j)
                jobs[j].out = C.pointer(out.c)
                for k, l in enumerate(dl):
                    jobs[j].layers[k] = C.pointer(l.c)
                jobs[j].nlayers = nlayers
            return cvs.cvs_chain_color_over_f16_dev(jobs, njobs, f32p(m), pre, post, fac.stream)
        return (_name("chain, %s" % what, width, height, "whole" if windows is None else "ragged"), case)
    scene, srgb = _lib.LUT_REC709_TO_LINEAR_SCENE, _lib.LUT_LINEAR_TO_SRGB
    return [make("1 layer", 1, 1, scene, _lib.LUT_NONE), make("4 layers", 1, 4, scene, _lib.LUT_NONE), make("8 layers", 1, 8, scene, _lib.LUT_NONE),
            make("a batch of two, both tables", 2, 2, scene, srgb), make("a ragged job", 1, 3, scene, _lib.LUT_NONE, _ragged(width, height))]


def blur_over(cvs, width, height):
    """Blur + over in one launch (whole windows, 9 taps, one overlay) and node by node (4 taps; ragged overlays)."""
    full = (0, 0, width - 1, height - 1)

    def make(what, ntaps, wins):
        taps = ec.synth.gaussian_taps(ntaps | 1, 1.5)[:ntaps].copy()

        def case(fac):
            rng = np.random.default_rng(3100 + ntaps)
            src = fac.frame(px16(rng, full), name="blur source")
            ov = [fac.frame(px16(rng, full, w), name="overlay %d" % k) for k, w in enumerate(wins)]
            out = fac.frame(blank(True, full), out=True, cmp="f16", name="blur output")
            return cvs.cvs_blur_over_f16_dev(out.ref(), src.ref(), f32p(taps), ntaps, ec._table(ov), len(wins), fac.stream)
        return (_name("blur over %s" % what, width, height, "whole"), case)
    return [make("in one launch, 9 taps, 1 overlay", 9, [full]), make("node by node, 4 taps, 2 overlays", 4, [full] * 2),
            make("node by node, 9 taps, ragged overlays", 9, _ragged(width, height))]


# ------------------------------------------------------------------ row streams: fields and key

def field_conversions(cvs, width, height, op):
    cases = []
    for wname, full, cur in windows(width, height):
        def case(fac, full=full, cur=cur):
            rng = np.random.default_rng(2600)
            a = fac.frame(px16(rng, full, cur))
            b = fac.frame(px16(rng, full, cur)) if op == "interlace" else None
            out = fac.frame(blank(True, full), out=True, cmp="exact" if op == "interlace" else "f16")
            if op == "interlace":
                return cvs.cvs_interlace_fields_f16_dev(out.ref(), a.ref(), b.ref(), fac.stream)
            if op == "soften":
                return cvs.cvs_soften_fields_f16_dev(out.ref(), a.ref(), fac.stream)
            return cvs.cvs_field_to_frame_f16_dev(out.ref(), a.ref(), int(op[-1]), fac.stream)
        cases.append((_name(op, width, height, wname), case))
    return cases


def chroma_key(cvs, width, height, half):
    p = ec.KEY_SETTINGS[0]
    params = _lib.chroma_key((C.c_float * 3)(*p["key"]), p["tolerance"], p["softness"], p["spill"], p["spill_range"], p["flags"])
    cases = []
    for wname, full, cur in windows(width, height):
        def case(fac, full=full, cur=cur):
            src = fac.frame(px(np.random.default_rng(2700), half, full, cur))
            out = fac.frame(blank(half, full), out=True, cmp="f16" if half else "f32")
            entry = cvs.cvs_chroma_key_f16_dev if half else cvs.cvs_chroma_key_f32_dev
            return entry(out.ref(), src.ref(), C.byref(params), fac.stream)
        cases.append((_name("key %s" % ("f16" if half else "f32"), width, height, wname), case))
    return cases


# ------------------------------------------------------------------ matte, transform

def matte(cvs, width, height, half):
    """Choke 16 and a 25-tap feather: the largest halo, 28 rows and columns, on every tile."""
    m = _lib.matte(16, ec.ROUGH25, 0.1, 0.9)
    cases = []
    for wname, full, cur in windows(width, height):
        def case(fac, full=full, cur=cur):
            src = fac.frame(px(np.random.default_rng(2800), half, full, cur))
            out = fac.frame(blank(half, full), out=True, cmp="f16" if half else "f32")
            entry = cvs.cvs_matte_refine_f16_dev if half else cvs.cvs_matte_refine_f32_dev
            return entry(out.ref(), src.ref(), C.byref(m), fac.stream)
        cases.append((_name("matte %s, choke 16, 25 taps" % ("f16" if half else "f32"), width, height, wname), case))
    return cases


def transform(cvs, width, height, half):
    """width x height is the TARGET.  A half-pixel shift from a source of the target's size, and a quarter turn from a source
    of the transposed size, under both filters."""
    tfull = (0, 0, width - 1, height - 1)
    turned = (0, 0, height - 1, width - 1)
    maps = [("half-pixel shift", tfull, (1.0, 0.0, 0.5, 0.0, 1.0, 0.5)),
            ("90 degrees", turned, (0.0, -1.0, float(height - 1), 1.0, 0.0, 0.0))]      # u = height - 1 - y, v = x
    cases = []
    for name, sfull, m in maps:
        for filt in (_lib.TRANSFORM_NEAREST, _lib.TRANSFORM_BILINEAR):
            def case(fac, sfull=sfull, m=m, filt=filt):
                t = _lib.transform(fac.matrix(m), filt)
                src = fac.frame(px(np.random.default_rng(2900), half, sfull))
                out = fac.frame(blank(half, tfull), out=True, cmp="f16" if half else "f32")
                entry = cvs.cvs_transform_f16_dev if half else cvs.cvs_transform_f32_dev
                return entry(out.ref(), src.ref(), C.byref(t), fac.stream)
            cases.append((_name("transform %s, %s, %s" % ("f16" if half else "f32", name, "bilinear" if filt else "nearest"), width, height, "whole"), case))
    return cases


# ------------------------------------------------------------------ blur and unsharp mask

BLUR_TAPS = [3, 13, 15, 4]      # the register window; its widest list; k_blur; an even count: the table kernels (k_fir)


def blur_and_unsharp(cvs, width, height, half, ntaps):
    taps = ec._taps(ntaps)
    cases = []
    for wname, full, cur in windows(width, height):
        def blur(fac, full=full, cur=cur):
            src = fac.frame(px(np.random.default_rng(3000), half, full, cur))
            out = fac.frame(blank(half, full), out=True, cmp="f16" if half else "f32")
            entry = cvs.cvs_fir_blur_f16_dev if half else cvs.cvs_fir_blur_f32_dev
            return entry(out.ref(), src.ref(), f32p(taps), ntaps, fac.stream)

        def unsharp(fac, full=full, cur=cur):
            src = fac.frame(px(np.random.default_rng(3001), half, full, cur))
            out = fac.frame(blank(half, full), out=True, cmp="f16" if half else "f32")
            entry = cvs.cvs_unsharp_mask_f16_dev if half else cvs.cvs_unsharp_mask_f32_dev
            return entry(out.ref(), src.ref(), f32p(taps), ntaps, C.c_float(0.7), C.c_float(0.01), fac.stream)
        cases.append((_name("blur %s, %d taps" % ("f16" if half else "f32", ntaps), width, height, wname), blur))
        if ntaps % 2:               # 3, 13: k_unsharp, the mask fused; 15: the blur, then k_unsharp_combine
            cases.append((_name("unsharp %s, %d taps" % ("f16" if half else "f32", ntaps), width, height, wname), unsharp))
    return cases


# ------------------------------------------------------------------ the bilinear scaler

def scale_bilinear(cvs, width, height, half, factor):
    """width x height is the TARGET; the source has the rows and columns the factor asks for."""
    sw, sh = int(width / factor) + 2, int(height / factor) + 2
    sfull, tfull = (0, 0, sw - 1, sh - 1), (0, 0, width - 1, height - 1)

    def case(fac):
        src = fac.frame(px(np.random.default_rng(3400), half, sfull))
        out = fac.frame(blank(half, tfull), out=True, cmp="f16" if half else "f32")
        entry = cvs.cvs_scale_bilinear_f16_dev if half else cvs.cvs_scale_bilinear_f32_dev
        return entry(out.ref(), fac.point(0, 0), src.ref(), fac.point(0, 0, source=True), ec.v2f(factor, factor), fac.stream)
    return [(_name("scale %s x%r" % ("f16" if half else "f32", factor), width, height, "whole"), case)]


def scale_bilinear_batch(cvs, width, height, half, factor):
    """The batch form of the case above: two frames."""
    sw, sh = int(width / factor) + 2, int(height / factor) + 2
    sfull, tfull = (0, 0, sw - 1, sh - 1), (0, 0, width - 1, height - 1)
    cls = _lib.rgba_frame_f16_t if half else _lib.rgba_frame_f32_t

    def case(fac):
        rng = np.random.default_rng(3401)
        srcs = [fac.frame(px(rng, half, sfull), name="source %d" % k) for k in range(2)]
        outs = [fac.frame(blank(half, tfull), out=True, cmp="f16" if half else "f32", name="target %d" % k) for k in range(2)]
        entry = cvs.cvs_scale_bilinear_f16_batch_dev if half else cvs.cvs_scale_bilinear_f32_batch_dev
        return entry(ec._table(outs, cls), fac.point(0, 0), ec._table(srcs, cls), fac.point(0, 0, source=True), ec.v2f(factor, factor), 2, fac.stream)
    return [(_name("scale batch %s x%r" % ("f16" if half else "f32", factor), width, height, "whole"), case)]


# ------------------------------------------------------------------ Lanczos at 0.5

def lanczos_resample(cvs, width, height):
    """width x height is the TARGET, the source twice as large on both axes; f16 and f32 (run under each of ec.LANCZOS_PINS)."""
    sfull, tfull = (0, 0, 2 * width - 1, 2 * height - 1), (0, 0, width - 1, height - 1)
    cases = []
    for half in (True, False):
        def case(fac, half=half):
            src = fac.frame(px(np.random.default_rng(3200), half, sfull))
            out = fac.frame(blank(half, tfull), out=True, cmp="f16" if half else "f32")
            entry = cvs.cvs_resample_lanczos_f16_dev if half else cvs.cvs_resample_lanczos_f32_dev
            return entry(out.ref(), src.ref(), C.c_float(0.5), C.c_float(0.5), 3, fac.stream)
        cases.append((_name("lanczos %s x0.5" % ("f16" if half else "f32"), width, height, "whole"), case))
    return cases


def blur_lanczos(cvs, width, height):
    """Blur (5 taps) + Lanczos at 0.5: a single call and a batch of two."""
    taps = ec._taps(5)
    sfull, tfull = (0, 0, 2 * width - 1, 2 * height - 1), (0, 0, width - 1, height - 1)

    def single(fac):
        src = fac.frame(px16(np.random.default_rng(3300), sfull))
        out = fac.frame(blank(True, tfull), out=True, cmp="f16")
        return cvs.cvs_blur_lanczos_f16_dev(out.ref(), src.ref(), f32p(taps), 5, C.c_float(0.5), C.c_float(0.5), 3, fac.stream)

    def batch(fac):
        rng = np.random.default_rng(3301)
        srcs = [fac.frame(px16(rng, sfull), name="source %d" % k) for k in range(2)]
        outs = [fac.frame(blank(True, tfull), out=True, cmp="f16", name="target %d" % k) for k in range(2)]
        return cvs.cvs_blur_lanczos_f16_batch_dev(ec._table(outs), ec._table(srcs), 2, f32p(taps), 5, C.c_float(0.5), C.c_float(0.5), 3, fac.stream)
    return [(_name("blur + lanczos x0.5", width, height, "whole"), single), (_name("blur + lanczos batch x0.5", width, height, "whole"), batch)]


# ------------------------------------------------------------------ coded planes, display bytes, the 3D LUT, the scopes

def mpeg2(cvs, width, height):
    """A raster as tall and as wide as the frame, as far as MPEG-2 allows one: an even width, a height that is a multiple of 4
    (two columns and four rows at least).  Reconstruction with both flag sets, subsampling of both windows."""
    rw, rh = max(2, width & ~1), max(4, height & ~3)
    strides, lines = [rw, rw // 2, rw // 2], [rh, rh // 2, rh // 2]
    planes = [np.random.default_rng(3600 + k).integers(0, 256, (n, s), dtype=np.uint8) for k, (n, s) in enumerate(zip(lines, strides))]
    full = (0, 0, width - 1, height - 1)
    cases = []
    for flags in (0, _lib.YCC_PROGRESSIVE | _lib.YCC_REC709):
        def reconstruct(fac, flags=flags):
            ptrs = [fac.buffer(p, "plane", name="plane %d" % k) for k, p in enumerate(planes)]
            out = fac.frame(blank(True, full), out=True, cmp="f16")
            return cvs.cvs_reconstruct_mpeg2_dev(out.ref(), C.byref(ec._image(ptrs, strides, lines)), rw, rh, flags, fac.stream)
        cases.append((_name("MPEG-2 reconstruct, flags %d" % flags, width, height, "whole"), reconstruct))
    for wname, _full, cur in windows(width, height):
        def subsample(fac, cur=cur):
            frame = fac.frame(px16(np.random.default_rng(3601), full, cur))
            ptrs = [fac.buffer(np.full((n, s), ec.PAD, np.uint8), "plane", out=True, name="plane %d" % k) for k, (n, s) in enumerate(zip(lines, strides))]
            return cvs.cvs_subsample_mpeg2_dev(C.byref(ec._image(ptrs, strides, lines)), frame.ref(), rw, rh, fac.stream)
        cases.append((_name("MPEG-2 subsample", width, height, wname), subsample))
    return cases


def display_bytes(cvs, width, height, pre):
    cases = []
    for wname, full, cur in windows(width, height):
        n = (cur[2] - cur[0] + 1) * (cur[3] - cur[1] + 1) * 4

        def make(call, what, full=full, cur=cur, n=n, wname=wname):
            def case(fac):
                frame = fac.frame(ec.all_codes(full, cur))
                out = fac.buffer(np.full(n, ec.PAD, np.uint8), "bytes", out=True, name="byte target")
                return call(out, frame, fac.stream)
            return (_name(what, width, height, wname), case)
        for mode in (_lib.DISPLAY_RGBA8, _lib.DISPLAY_ARGB32_PREMUL):
            cases.append(make(lambda out, f, s, mode=mode: cvs.cvs_frame_to_bytes_dev(out, f.ref(), pre, mode, s), "frame to bytes, mode %d" % mode))
        cases.append(make(lambda out, f, s: cvs.cvs_frame_to_rgba8_intent_dev(out, f.ref(), pre, C.c_float(1.25), s), "frame to rgba8, intent 1.25"))
    return cases


def lut3d(cvs, width, height, half, size):
    """N = 17: the lattice in LDS; N = 33: through the caches, on the row-stream grid (stream_common.hpp)."""
    from tests import lut3d_model as lm
    p = _lib.lut3d(size)
    cases = []
    for wname, full, cur in windows(width, height):
        def case(fac, full=full, cur=cur):
            src = fac.frame(px(np.random.default_rng(3700), half, full, cur))
            out = fac.frame(blank(half, full), out=True, cmp="f16" if half else "f32")
            lattice = fac.buffer(lm.packed(lm.distinct(size, size)), "f32", name="lattice")
            entry = cvs.cvs_lut3d_f16_dev if half else cvs.cvs_lut3d_f32_dev
            return entry(out.ref(), src.ref(), lattice, C.byref(p), fac.stream)
        cases.append((_name("lut3d %s N=%d" % ("f16" if half else "f32", size), width, height, wname), case))
    return cases


SCOPE_COLUMNS = 7


def _scope_count(kind):
    return {_lib.SCOPE_HISTOGRAM: 5 * 256, _lib.SCOPE_WAVEFORM: SCOPE_COLUMNS * 256}[kind]


def scope_counts(cvs, width, height, kind):
    """The region is the window; through the exporter's table without the transparent pixels, and through the widget's."""
    cases = []
    for wname, full, cur in windows(width, height):
        for widget in (False, True):
            def case(fac, full=full, cur=cur, widget=widget):
                frame = fac.frame(ec.all_codes(full, cur))
                table = fac.buffer(np.full(_scope_count(kind) * 4, ec.PAD, np.uint8), "bytes", out=True, name="count table")
                p = _lib.scope(kind, fac.box(*cur), columns=SCOPE_COLUMNS, pre_lut=_lib.LUT_LINEAR_TO_SRGB if widget else _lib.LUT_NONE,
                               rendering_intent=1.25 if widget else 0.0, flags=0 if widget else _lib.SCOPE_SKIP_TRANSPARENT)
                return cvs.cvs_scope_counts_f16_dev(table, frame.ref(), C.byref(p), fac.stream)
            cases.append((_name("scope counts, kind %d, %s" % (kind, "widget" if widget else "export"), width, height, wname), case))
    return cases


def scope_render(cvs, width, height):
    """A waveform picture (7 x 256: a place is at most 12 288 x 256, whatever the target) over the target's last rows and
    columns, overhanging it below and on the right."""
    full = (0, 0, width - 1, height - 1)
    x0, y0 = (width - 5 if width > SCOPE_COLUMNS else -2), height - 100

    def render(fac):
        n = _scope_count(_lib.SCOPE_WAVEFORM)
        counters = (np.arange(n, dtype=np.uint64) * 2654435761 % 41).astype(np.uint32)
        table = fac.buffer(counters, "bytes", name="count table")
        target = fac.frame(blank(True, full), out=True, name="scope picture")
        place = fac.box(x0, y0, x0 + SCOPE_COLUMNS - 1, y0 + 255)
        p = _lib.scope(_lib.SCOPE_WAVEFORM, fac.box(0, 0, 0, 0), columns=SCOPE_COLUMNS)
        return cvs.cvs_scope_render_f16_dev(target.ref(), C.byref(place), table, C.byref(p), C.c_float(1.0 / 16.0), fac.stream)
    return [(_name("scope render, waveform", width, height, "last rows"), render)]


# ------------------------------------------------------------------ blur + over in a batch, the workspace stack

def blur_over_batch(cvs, width, height):
    taps = ec.synth.gaussian_taps(9, 1.5)
    full = (0, 0, width - 1, height - 1)

    def batch(fac):
        rng = np.random.default_rng(3150)
        srcs = [fac.frame(px16(rng, full), name="blur source %d" % k) for k in range(2)]
        ovs = [fac.frame(px16(rng, full), name="overlay of frame %d" % k) for k in range(2)]
        outs = [fac.frame(blank(True, full), out=True, cmp="f16", name="blur output %d" % k) for k in range(2)]
        return cvs.cvs_blur_over_f16_batch_dev(ec._table(outs), ec._table(srcs), f32p(taps), 9, ec._table(ovs), 1, 2, fac.stream)
    return [(_name("blur over batch, 9 taps", width, height, "whole"), batch)]


def workspace_stack(cvs, width, height):
    """entry_cases.workspace_stack at this extent: three device-resident layers (z order 0, 7, 3), the upper two ragged."""
    full = (0, 0, width - 1, height - 1)
    wins = [full] + _ragged(width, height)
    cases = []
    for half_native, half_target in ((True, True), (True, False), (False, True)):
        def case(fac, half_native=half_native, half_target=half_target):
            rng = np.random.default_rng(3800)
            layers = [fac.frame(px16(rng, full, w), name="layer %d" % k) for k, w in enumerate(wins)]
            out = fac.frame(blank(half_target, full, full), out=True, cmp="f16" if half_target else "f32", name="pulled frame")
            sources = [ec._device_source(cvs, l, half_native) for l in layers]
            ws = cvs.workspace_create()
            try:
                for (src, _keep), z in zip(sources, (0, 7, 3)):
                    cvs.workspace_add_item(ws, C.cast(C.pointer(src), C.c_void_p), 0, 10, 0, z, None)
                vs = ec.video_source()
                cvs.workspace_as_video_source(ws, C.byref(vs))
                d = _lib.rgba_frame_dev(out.ptr, ec.FORMAT_F16 if half_target else ec.FORMAT_F32, out.c.full_window, out.c.full_window, fac.stream)
                cvs.video_get_frame_dev(C.byref(vs), 4, C.byref(d))
                out.c.current_window = d.current_window
            finally:
                cvs.workspace_free(ws)
            return 0
        cases.append((_name("workspace stack, %s sources, pulled as %s" % ("half-native" if half_native else "two-format", "f16" if half_target else "f32"),
                            width, height, "ragged"), case))
    return cases


# ------------------------------------------------------------------ the extension headers: the row-stream pair

def _held(codes, full, cur):
    return HostFrame(full, np.uint16, codes, cur)


@functools.lru_cache(maxsize=1)
def _thirds(full):
    """(a case is run several times on the same pictures -- the reference side, both poisons -- and four million rows take a second to draw)"""
    return _read_only(dm.thirds(np.random.default_rng(4100), full, dc.THRESHOLD, dc.SOFTNESS))


@functools.lru_cache(maxsize=1)
def _sequence(full):
    return _read_only(tpm.sequence(np.random.default_rng(4200), full, tc.THRESHOLD, tc.SOFTNESS))


def _read_only(arrays):
    for a in arrays:
        a.setflags(write=False)
    return tuple(arrays)


def deinterlace_adaptive(cvs, width, height):
    """tests/deinterlace_model.py's thirds (at one or two columns: the third whose neighbours straddle the ramp), so that with the
    catalogue's nonzero softness the blend runs beside both copies.  Per window field 0 between two neighbours and field 1 with
    the previous frame alone (a clip's last frame); on the whole buffer also field 1 between two."""
    cases = []
    for wname, full, cur in windows(width, height):
        for field, which in [(0, "both"), (1, "prev")] + ([(1, "both")] if wname == "whole" else []):
            def case(fac, full=full, cur=cur, field=field, which=which):
                prev, now, nxt = (_held(codes, full, cur) for codes in _thirds(full))
                a = fac.frame(prev)
                b = fac.frame(now)
                c = fac.frame(nxt) if which == "both" else None
                out = fac.frame(blank(True, full), out=True, cmp="f16")
                p = _lib.deinterlace_adaptive(field, dc.THRESHOLD, dc.SOFTNESS)
                return cvs.cvs_deinterlace_adaptive_f16_dev(out.ref(), a.ref(), b.ref(), c.ref() if c else None, C.byref(p), fac.stream)
            cases.append((_name("adaptive deinterlace, field %d, neighbours %s" % (field, which), width, height, wname), case))
    return cases


def temporal(cvs, width, height, radius):
    """tests/temporal_model.py's sequence; radius 1: the two near neighbours, radius 2: all four, every channel, on the ramp."""
    which = tc.WHICH["near" if radius == 1 else "all"]
    cases = []
    for wname, full, cur in windows(width, height):
        def case(fac, full=full, cur=cur):
            prev2, prev1, now, next1, next2 = (_held(codes, full, cur) for codes in _sequence(full))
            frames = [fac.frame(f) if on else None for f, on in zip((prev2, prev1), which[:2])]
            frames.append(fac.frame(now))
            frames += [fac.frame(f) if on else None for f, on in zip((next1, next2), which[2:])]
            out = fac.frame(blank(True, full), out=True, cmp="f16")
            p = _lib.temporal_denoise(tc.THRESHOLD, tc.SOFTNESS, tpm.ALL)
            refs = [f.ref() if f else None for f in frames]
            return cvs.cvs_temporal_denoise_f16_dev(out.ref(), refs[0], refs[1], refs[2], refs[3], refs[4], C.byref(p), fac.stream)
        cases.append((_name("temporal denoise, radius %d" % radius, width, height, wname), case))
    return cases


# ------------------------------------------------------------------ the corner pin

PIN_REACH = 20000           # rows between the map's origin and its vanishing line, where the target has them


def pin_map(width, height, near):
    """(h, target origin, source origin, source buffer) of a true perspective for a target of width x height (h6, h7 != 0: a
    parallelogram would give the affine kernel's bytes).  With x, y counted from the target origin and D = the reach,

        w = 1 + x / (8 * source width) - y / D

    so the vanishing line w = 0 lies D rows below the origin, which is placed so that the line crosses a tall target 20 rows above
    its last row (of 524 320 rows: inside the launcher's second band, which starts at row 524 280); a target of a few rows has the
    line four rows below it.  One map cannot vary from row to row both far from its line and next to it (v is a Moebius function
    of y: its slope falls with 1 / w^2), so there are two:

        far    u = (x + y / 1024 + 1/4) / w;  v = (2 - 0.4 y) / w.  Above the origin v climbs towards 0.4 D, the source's height,
               and differs from row to row for some 400 000 rows: a row of the first band put in another's place shows.  The D rows
               between the origin and the line fall outside the source, the rows beyond the line have w <= 0: both zero.
        near   u = 1/4 + x / w;  v = 4 + c / w with c D = the source's height less 8: k rows above the line the middle column
               samples source row 4 + c D / k -- 404, 425, ... 4004, 8004 in the second band's first 20 rows -- and the rows
               beyond it are zero: the second band holds drawn and undrawn rows, every drawn one different.

    The source is as wide as the target and 64 columns more, so u runs off it on both sides of a wide target."""
    reach = max(8, min(PIN_REACH, height // 2))
    line = height - 20 if height >= 64 else height + 4
    sw, sh = width + 64, int(0.4 * reach) + 8
    h6, h7 = 1.0 / (8.0 * sw), -1.0 / reach
    if near:
        u0, v0, c = 0.25, 4.0, (sh - 8.0) / reach
        h = (1.0 + u0 * h6, u0 * h7, u0, v0 * h6, v0 * h7, v0 + c, h6, h7, 1.0)
    else:
        h = (1.0, 1.0 / 1024.0, 0.25, 0.0, -0.4, 2.0, h6, h7, 1.0)
    return h, (width // 2, line - reach), (sw // 2, 0), (0, 0, sw - 1, sh - 1)


def perspective(cvs, width, height, half):
    """width x height is the TARGET.  A bilinear and a nearest case of each of pin_map's two maps; the origins go through fac.box,
    as tests/perspective_cases.py params() takes them."""
    tfull = (0, 0, width - 1, height - 1)
    cases = []
    for near in (False, True):
        h, to, so, sfull = pin_map(width, height, near)
        for filt in (_lib.TRANSFORM_BILINEAR, _lib.TRANSFORM_NEAREST):
            def case(fac, h=h, to=to, so=so, sfull=sfull, filt=filt):
                t, s = fac.box(to[0], to[1], to[0], to[1]), fac.box(so[0], so[1], so[0], so[1])
                p = _lib.perspective(h, (t.min.x, t.min.y), (s.min.x, s.min.y), filt)
                src = fac.frame(px(np.random.default_rng(4300), half, sfull))
                out = fac.frame(blank(half, tfull), out=True, cmp="f16" if half else "f32")
                entry = cvs.cvs_perspective_f16_dev if half else cvs.cvs_perspective_f32_dev
                return entry(out.ref(), src.ref(), C.byref(p), fac.stream)
            cases.append((_name("perspective %s, %s map, %s" % ("f16" if half else "f32", "near" if near else "far", "bilinear" if filt else "nearest"),
                                width, height, "whole"), case))
    return cases


# ------------------------------------------------------------------ the 4:2:2 and 4:2:0 edges

# width x height of the RASTER; the frame is the raster's window or the inset one.  Where the 128 KiB transfer table lives is
# table_placement.hpp's: gathered through L2 up to kGatherUpTo pixels, staged into LDS above.  Every raster here but the last of
# each list lies below that line and runs the gathered form; the last, of two columns, is the first two-column row in the LDS form
# (tests/test_extents_cpu.py test_the_tallest_raster_alone_is_above_the_table_line reads the constant and holds the lists to this).
YCC422_RASTERS = [(2, 65535), (2, 65536), (4, 70001), (70002, 3), (131074, 2), (2, 4194305)]      # any height is legal
YCC420_RASTERS = [(2, 65534), (2, 65536), (4, 70002), (70002, 4), (131074, 2), (2, 4194306)]      # even heights
YCC_FEW = [(2, 65536), (131074, 2)]


def ycc422(cvs, width, height, layout):
    """Both directions; the raster's own window with the least strides, and the inset window with padded ones."""
    strides, lines = y422m.least(layout, width, height)
    cases = []
    for n, (wname, full, cur) in enumerate(windows(width, height)):
        frame = full if wname == "whole" else cur
        padded = [s + p for s, p in zip(strides, y422.PADS[layout][n])]
        for direction in ("reconstruct", "subsample"):
            spec = dict(direction=direction, layout=layout, matrix="601" if n else "709", width=width, height=height, strides=padded, lines=lines,
                        full=frame, seed=4400 + n)
            cases.append((_name(y422.name(spec), width, height, wname), y422.make_case(cvs, spec)))
    return cases


def ycc420(cvs, width, height, layout):
    """Both directions.  Below 2^19 rows: the raster's window at left siting, the inset window with padded strides at centre siting
    (the import keeps a lane for the column on the left: runs of 62 columns) and full range, the raster's window at top-left siting
    without a transfer table.  At the tallest raster, where the table is in LDS: centre siting with the table, top-left without."""
    strides, lines = y420m.least(layout, width, height)
    wins = windows(width, height)
    whole, inset = wins[0][1], wins[-1][2]
    if len(wins) == 1:
        forms = [("whole", whole, 0, "center", "studio", "709", "709"), ("whole", whole, 0, "topleft", "studio", "2020", "none")]
    else:
        forms = [("whole", whole, 0, "left", "studio", "709", "709"), ("inset", inset, 1, "center", "full", "601", "709"),
                 ("whole", whole, 0, "topleft", "studio", "2020", "none")]
    cases = []
    for n, (wname, frame, pad, siting, range_, matrix, transfer) in enumerate(forms):
        padded = [s + p for s, p in zip(strides, y420.PADS[layout][pad])]
        for direction in ("reconstruct", "subsample"):
            spec = dict(direction=direction, layout=layout, siting=siting, range=range_, matrix=matrix, transfer=transfer, width=width, height=height,
                        strides=padded, lines=lines, full=frame, seed=4500 + n)
            cases.append((_name(y420.name(spec), width, height, wname), y420.make_case(cvs, spec)))
    return cases


# ------------------------------------------------------------------ the median, the primary, the secondaries

# Thin groups over the operands of tests/median_cases.py, primary_cases.py and secondary_cases.py: what puts the entries under the
# headers' completeness check at 65 536 rows and 70 001 columns.  Their widest and tallest windows (131 073 columns, 4 194 305
# rows) stay where they are, in the extent tests of their harness modules.
THIN = [(2, 65536), (70001, 3)]


def median(cvs, width, height):
    cases = []
    for wname, full, cur in windows(width, height):
        for half, radius, threshold, channels in ((True, 2, mdm.THRESHOLD, "rgba"), (False, 1, 0.0, "ga")):
            def case(fac, full=full, cur=cur, half=half, radius=radius, threshold=threshold, channels=channels):
                src = fac.frame(mdc.source(np.random.default_rng(4600), half, full, cur))
                out = fac.frame(blank(half, full), out=True, cmp="f16" if half else "f32")
                p = _lib.median(radius, threshold, mdm.mask_of(channels))
                entry = cvs.cvs_median_f16_dev if half else cvs.cvs_median_f32_dev
                return entry(out.ref(), src.ref(), C.byref(p), fac.stream)
            cases.append((_name("median %s, radius %d" % ("f16" if half else "f32", radius), width, height, wname), case))
    return cases


def primary(cvs, width, height):
    """Out of place in both formats (curves, matrix, curves; curves alone twice), and the half frame in place."""
    cases = []
    for wname, full, cur in windows(width, height):
        for half, stages, in_place in ((True, prc.STAGES[0], False), (False, prc.STAGES[6], False), (True, prc.STAGES[4], True)):
            def case(fac, full=full, cur=cur, half=half, stages=stages, in_place=in_place):
                cmp = "f16" if half else "f32"
                src = fac.frame(px(np.random.default_rng(4700), half, full, cur), out=in_place, cmp=cmp, in_place=in_place)
                out = src if in_place else fac.frame(blank(half, full), out=True, cmp=cmp)
                pre, post = prc._tables(fac, stages)
                p = prc._params(stages)
                return prc._entry(cvs, half)(out.ref(), src.ref(), C.byref(p), pre, post, fac.stream)
            cases.append((_name("primary %s%s" % ("f16" if half else "f32", ", in place" if in_place else ""), width, height, wname), case))
    return cases


def secondaries(cvs, width, height):
    """The qualifier on all three axes with a key frame of its own, and the mix through a matte's luma, in both formats; every
    input's current window narrowed its own way (tests/secondary_cases.py _narrowed)."""
    cases = []
    for wname, full, cur in windows(width, height):
        for half in (True, False):
            cmp, fmt = ("f16", "f16") if half else ("f32", "f32")

            def qualify(fac, full=full, cur=cur, half=half, cmp=cmp):
                rng = np.random.default_rng(4800)
                src = fac.frame(sec.picture(rng, half, full, cur))
                key = fac.frame(sec.picture(rng, half, full, sec._narrowed(cur, 1)))
                out = fac.frame(blank(half, full), out=True, cmp=cmp)
                p = sec.params(sec.QUALIFIERS[7])
                return sec._qualify(cvs, half)(out.ref(), src.ref(), key.ref(), C.byref(p), fac.stream)

            def mix(fac, full=full, cur=cur, half=half, cmp=cmp):
                rng = np.random.default_rng(4850)
                ins = [fac.frame(sec.picture(rng, half, full, w)) for w in (cur, sec._narrowed(cur, 1), sec._narrowed(cur, 2))]
                out = fac.frame(blank(half, full), out=True, cmp=cmp)
                p = _lib.matte_mix(True, False)
                return sec._mix(cvs, half)(out.ref(), ins[0].ref(), ins[1].ref(), ins[2].ref(), C.byref(p), fac.stream)
            cases += [(_name("qualify %s" % fmt, width, height, wname), qualify), (_name("matte mix %s" % fmt, width, height, wname), mix)]
    return cases


# ------------------------------------------------------------------ every group at every extent

def _groups():
    """(id, FIR path pin, builder(cvs, width, height), extents, halo): `halo` is how many rows beyond a band of rows the rows
    of that band depend on -- 0 for a pointwise group -- or None where a row depends on rows far from it."""
    auto = _lib.FIR_PATH_AUTO
    both = AT_16_BITS + WIDE
    g = [("copies_and_conversions", auto, copies_and_conversions, both, 0), ("attenuate_in_place", auto, attenuate_in_place, both, 0),
         ("solid_fills", auto, solid_fills, both, 0)]
    g += [("colour_matrix[%d-%d]" % (pre, post), auto, lambda cvs, w, h, pre=pre, post=post: colour_matrix(cvs, w, h, pre, post), both, 0)
          for pre, post in ec.COLOUR_MATRIX_TABLES]
    # the mixers choose their regions from the windows' corners (video_mix.c:137,265), the weave addresses its second field
    # linearly: neither is a function of a band of rows alone
    g += [("mixers_f32", auto, mixers_f32, both, None), ("weave_fields", auto, weave_fields, both + WEAVE_ROWS, None)]
    g += [("mix_cross_f16", auto, mix_cross_f16, both, None), ("chain", auto, chain, both, None), ("blur_over", auto, blur_over, both, None)]
    g += [("field_conversions[%s]" % op, auto, lambda cvs, w, h, op=op: field_conversions(cvs, w, h, op), both + STREAM_ROWS, 2) for op in ec.FIELD_OPS]
    g += [("chroma_key[f16]", auto, lambda cvs, w, h: chroma_key(cvs, w, h, True), both + STREAM_ROWS, 0),
          ("chroma_key[f32]", auto, lambda cvs, w, h: chroma_key(cvs, w, h, False), both, 0)]
    g += [("matte[%s]" % ("f16" if half else "f32"), auto, lambda cvs, w, h, half=half: matte(cvs, w, h, half), both + (MATTE_ROWS if half else MATTE_ROWS[-1:]), 28)
          for half in (True, False)]
    g += [("transform[%s]" % ("f16" if half else "f32"), auto, lambda cvs, w, h, half=half: transform(cvs, w, h, half), both + (TRANSFORM_ROWS if half else TRANSFORM_ROWS[-1:]), None)
          for half in (True, False)]
    g += [("blur_and_unsharp[%s-%d]" % ("f16" if half else "f32", n), auto, lambda cvs, w, h, half=half, n=n: blur_and_unsharp(cvs, w, h, half, n), both, n // 2)
          for half in (True, False) for n in BLUR_TAPS]
    g += [("scale_bilinear[f16-2.0-tiles]", ec.PINS["tiles"], lambda cvs, w, h: scale_bilinear(cvs, w, h, True, 2.0), AT_16_BITS + [(70001, 3)] + SCALER_ROWS, None),
          ("scale_bilinear[f16-2.0-strips]", ec.PINS["strips"], lambda cvs, w, h: scale_bilinear(cvs, w, h, True, 2.0), AT_16_BITS + [(70001, 3)], None),
          ("scale_bilinear[f32-2.0]", auto, lambda cvs, w, h: scale_bilinear(cvs, w, h, False, 2.0), AT_16_BITS + [(70001, 3)], None),
          ("scale_bilinear[f16-0.5]", auto, lambda cvs, w, h: scale_bilinear(cvs, w, h, True, 0.5), AT_16_BITS + [(70001, 3)], None),
          ("scale_bilinear[f32-0.5]", auto, lambda cvs, w, h: scale_bilinear(cvs, w, h, False, 0.5), AT_16_BITS + [(70001, 3)], None)]
    resampled = AT_16_BITS + [(70001, 3)]
    g += [("scale_bilinear_batch[%s-%r]" % ("f16" if half else "f32", f), auto, lambda cvs, w, h, half=half, f=f: scale_bilinear_batch(cvs, w, h, half, f), resampled, None)
          for half in (True, False) for f in (2.0, 0.5)]
    g += [("lanczos_resample[%s]" % pin, ec.PINS[pin], lanczos_resample, resampled, None) for pin in ec.LANCZOS_PINS]
    g += [("blur_lanczos", auto, blur_lanczos, resampled, None)]
    g += [("blur_over_batch", auto, blur_over_batch, both, None), ("workspace_stack", auto, workspace_stack, both, None), ("mpeg2", auto, mpeg2, both, None)]
    g += [("display_bytes[%d]" % pre, auto, lambda cvs, w, h, pre=pre: display_bytes(cvs, w, h, pre), both, None) for pre in ec.DISPLAY_TABLES]
    g += [("lut3d[f16-17]", auto, lambda cvs, w, h: lut3d(cvs, w, h, True, 17), both, 0), ("lut3d[f32-17]", auto, lambda cvs, w, h: lut3d(cvs, w, h, False, 17), both, 0),
          ("lut3d[f16-33]", auto, lambda cvs, w, h: lut3d(cvs, w, h, True, 33), both + STREAM_ROWS, 0), ("lut3d[f32-33]", auto, lambda cvs, w, h: lut3d(cvs, w, h, False, 33), both, 0)]
    g += [("scope_counts[%d]" % kind, auto, lambda cvs, w, h, kind=kind: scope_counts(cvs, w, h, kind), both, None) for kind in (_lib.SCOPE_HISTOGRAM, _lib.SCOPE_WAVEFORM)]
    g += [("scope_render", auto, scope_render, both, None)]
    # the extension headers.  Halos, read from the models: a made row of the deinterlacer takes the rows above and below it, and
    # its weight -- like the denoise's -- the 3 x 3 differences around the pixel (deinterlace_model.neighbourhood): 1 row.  The
    # 4:2:0 import reads chroma rows c - 1 and c + 1 for luma rows 2c and 2c + 1 (ycc420_model.vertical), the export luma row
    # 2c - 1 (filter_chroma): 2 rows.  The 4:2:2 edges work along a row: 0.  The corner pin reads the source wherever h says.
    g += [("deinterlace_adaptive", auto, deinterlace_adaptive, both + STREAM_ROWS, 1),
          ("temporal[1]", auto, lambda cvs, w, h: temporal(cvs, w, h, 1), both, 1),
          ("temporal[2]", auto, lambda cvs, w, h: temporal(cvs, w, h, 2), both + STREAM_ROWS, 1)]
    g += [("perspective[%s]" % ("f16" if half else "f32"), auto, lambda cvs, w, h, half=half: perspective(cvs, w, h, half), both + (TRANSFORM_ROWS if half else TRANSFORM_ROWS[-1:]), None)
          for half in (True, False)]
    g += [("ycc422[%s]" % layout, auto, lambda cvs, w, h, layout=layout: ycc422(cvs, w, h, layout), YCC422_RASTERS if layout in ("v210", "planar8") else YCC_FEW, 0)
          for layout in y422.LAYOUT_NAMES]
    g += [("ycc420[%s]" % layout, auto, lambda cvs, w, h, layout=layout: ycc420(cvs, w, h, layout), YCC420_RASTERS if layout in ("nv12", "planar10") else YCC_FEW, 2)
          for layout in y420.LAYOUT_NAMES]
    g += [("median", auto, median, THIN, 2), ("primary", auto, primary, THIN, 0), ("secondaries", auto, secondaries, THIN, 0)]
    return g


GROUPS = _groups()
