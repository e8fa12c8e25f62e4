"""The CPU oracle against a build of the reference's own src/cprocess (oracle/ref_build.py -> oracle/_ref/), bit for bit,
in both flavours: the gcc reference against liboracle.so, the clang (contracting) reference against liboracle_fma.so.
Only what tests/util.py canon_f16 / canon_f32 fold is folded; whole buffers and the reported windows are compared.

Skips where the reference was never built (no reference tree on that machine).  Where the two disagree the reference is
right and oracle/*.c is what gets fixed.  Entry points with no CPU implementation in the reference (gain/offset, FIR blur,
the Lanczos resampler beyond its taps, the general matrix, key, unsharp, fields, MPEG-2) have no case here: DESIGN.md A.
"""
import numpy as np
import pytest

import oracle
from canvas_amd.abi import HostFrame
from tests import reference_cases as rc
from tests.util import canon_f16, canon_f32

FLAVOURS = ["gcc", "fma"]

if oracle.ref("gcc") is None or oracle.ref("fma") is None:
    pytest.skip("the reference's own code is not built here (oracle/ref_build.py)", allow_module_level=True)


@pytest.fixture(params=FLAVOURS)
def pair(request, orc):
    """(reference build, oracle build) of one flavour."""
    with orc.flavour(request.param):
        yield rc.ref_abi(orc.ref(request.param)), rc.OrcAbi(orc)


def _same(a, b, what):
    (ca, wa), (cb, wb) = a, b
    assert wa == wb, "%s: window %r (reference) != %r (oracle)" % (what, wa, wb)
    assert ca.shape == cb.shape, what
    if not np.array_equal(ca, cb):
        bad = np.argwhere(ca != cb)
        i = tuple(bad[0])
        raise AssertionError("%s: %d of %d codes differ; first at %s: reference 0x%x, oracle 0x%x" % (what, len(bad), ca.size, i, ca[i], cb[i]))


# ------------------------------------------------------------------ half conversion

def test_h2f_all_codes(pair):
    ref, orc = pair
    a, b = ref.h2f(rc.ALL_CODES), orc.h2f(rc.ALL_CODES)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))         # payloads included: both are table look-ups


def test_f2h_probe_set_and_fast_variants(pair):
    ref, orc = pair
    for i, p in enumerate(rc.f2h_probes(orc.h2f)):
        assert np.array_equal(ref.f2h(p), orc.f2h(p)), "probe set %d" % i
    nan = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0x7F802000, 0x7FFFFFFF], np.uint32).view(np.float32)
    assert np.array_equal(ref.f2h(nan), orc.f2h(nan))                    # integer code on both sides: NaN bits are pinned too
    # the _fast pair is exponent re-biasing in integers: defined (if not meaningful) for every input
    a, b = ref.h2f(rc.ALL_CODES, fast=True), orc.h2f(rc.ALL_CODES, fast=True)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    for p in rc.f2h_probes(orc.h2f):
        assert np.array_equal(ref.f2h(p, fast=True), orc.f2h(p, fast=True))


# ------------------------------------------------------------------ tables

@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_transfer_tables_all_codes(pair, which):
    ref, orc = pair
    a, b = ref.table(which), orc.table(which)
    bad = np.flatnonzero(canon_f16(a) != canon_f16(b))
    assert bad.size == 0, "table %d: %d codes differ, first 0x%04x: reference 0x%04x oracle 0x%04x" % (which, bad.size, bad[0], a[bad[0]], b[bad[0]])


def test_gamma45_ramp(pair):
    ref, orc = pair
    a, b = ref.ramp(), orc.ramp()
    ok = ((rc.ALL_CODES & 0x7FFF) <= 0x7C00) & (rc.ALL_CODES < 0x8000)   # a NaN or a negative float has no defined byte in C
    assert np.array_equal(a[ok], b[ok])


# ------------------------------------------------------------------ taps

@pytest.mark.parametrize("sub,offset", rc.TAP_GRID)
def test_fir_taps(pair, sub, offset):
    ref, orc = pair
    for kind, a, b in (("triangle", ref.triangle(sub, offset), orc.triangle(sub, offset)),
                       ("lanczos", ref.lanczos(sub, 3, offset), orc.lanczos(sub, 3, offset))):
        assert a[1:] == b[1:], (kind, "width, centre", a[1:], b[1:])
        assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), (kind, sub, offset, a[0], b[0])


@pytest.mark.parametrize("sub,size", [(0.5, 3), (0.5, 2), (0.3, 4), (1.0, 1), (2.5, 3)])
def test_lanczos_taps_other_sizes(pair, sub, size):
    """The grid of test_oracle_pins.test_lanczos_taps (sub 0.5, size 3) and the kernel sizes around it."""
    ref, orc = pair
    a, b = ref.lanczos(sub, size, 0.0), orc.lanczos(sub, size, 0.0)
    assert a[1:] == b[1:] and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))


# ------------------------------------------------------------------ copies

@pytest.mark.parametrize("out_full,in_full,in_cur", rc.COPY_WINDOWS)
def test_copy_frame_f16(pair, out_full, in_full, in_cur):
    ref, orc = pair
    res = []
    for impl in (ref, orc):
        rng = np.random.default_rng(1)
        src, out = rc.lively_f16(rng, in_full, in_cur), rc.lively_f16(rng, out_full, out_full)
        impl.copy_f16(out, src)
        res.append((out.array.copy(), rc.win_of(out)))              # a copy: not one bit may change, NaN payloads included
    _same(res[0], res[1], "copy f16")


@pytest.mark.parametrize("out_full,in_full,in_cur", rc.COPY_WINDOWS)
@pytest.mark.parametrize("alpha", [1.0, 0.4, 0.0, 1.5, -2.0])
def test_copy_frame_alpha_f32(pair, out_full, in_full, in_cur, alpha):
    ref, orc = pair
    res = []
    for impl in (ref, orc):
        rng = np.random.default_rng(2)
        src, out = rc.lively_f32(rng, in_full, in_cur), rc.lively_f32(rng, out_full, out_full)
        impl.copy_alpha(out, src, alpha)
        res.append((canon_f32(out.array), rc.win_of(out)))
    _same(res[0], res[1], "copy alpha")


# ------------------------------------------------------------------ mixes

@pytest.mark.parametrize("i", range(len(rc.MIX_WINDOWS)))
@pytest.mark.parametrize("mix", rc.MIXES)
def test_mix_over(pair, i, mix):
    ref, orc = pair
    for windows, full in ((rc.MIX_WINDOWS, rc.MIX_FULL), (rc.BIG_WINDOWS, rc.BIG_FULL)):
        _same(rc.over_case(ref, i, mix, windows, full), rc.over_case(orc, i, mix, windows, full), "over %r mix %g" % (windows[i], mix))


@pytest.mark.parametrize("i", range(len(rc.MIX_WINDOWS)))
@pytest.mark.parametrize("mix", rc.MIXES)
def test_mix_cross(pair, i, mix):
    ref, orc = pair
    for windows, full in ((rc.MIX_WINDOWS, rc.MIX_FULL), (rc.BIG_WINDOWS, rc.BIG_FULL)):
        _same(rc.cross_case(ref, i, mix, windows, full), rc.cross_case(orc, i, mix, windows, full), "cross %r mix %g" % (windows[i], mix))


@pytest.mark.parametrize("i", range(len(rc.MIX_WINDOWS)))
def test_mix_cross_in_place(pair, i):
    ref, orc = pair
    res = []
    for impl in (ref, orc):
        rng = np.random.default_rng(3000 + i)
        a, b = rc.lively_f32(rng, rc.MIX_FULL, rc.MIX_WINDOWS[i][0]), rc.lively_f32(rng, rc.MIX_FULL, rc.MIX_WINDOWS[i][1])
        impl.cross(a, a, b, 0.3)
        res.append((canon_f32(a.array), rc.win_of(a)))
    _same(res[0], res[1], "cross in place %r" % (rc.MIX_WINDOWS[i],))


# ------------------------------------------------------------------ scaler

def _scale(impl, tfull, sfull, scur, tp, sp, fac, src):
    frame = HostFrame(sfull, np.float32, src.copy(), scur)
    out = HostFrame(tfull, np.float32, fill=rc.SENTINEL_F32)
    impl.scale(out, tp, frame, sp, fac)
    return canon_f32(out.array), rc.win_of(out)


def test_scaler_on_the_model_setups(pair):
    ref, orc = pair
    rng = np.random.default_rng(305)
    undefined = 0                                 # see rc.scale_defined_in_reference: the reference itself overflows there
    for tfull, sfull, scur, tp, sp, fac in rc.scaler_setups(rng):
        src = rng.uniform(-0.5, 1.5, (sfull[3] - sfull[1] + 1, sfull[2] - sfull[0] + 1, 4)).astype(np.float32)
        args = (tfull, sfull, scur, tp, sp, fac, src)
        if not rc.scale_defined_in_reference(ref, *args[:6]):
            undefined += 1
            continue
        _same(_scale(ref, *args), _scale(orc, *args), "scale %r" % (args[:6],))
    assert undefined <= 6, undefined              # the set-ups stay what they are: nearly all of them are defined calls


def test_scaler_random_geometry_sweep(pair):
    """Free factors and points (the set-ups above draw them from short lists): 150 geometries, sources with an inset
    window, factors from 1/5 to 5 on each axis independently."""
    ref, orc = pair
    rng = np.random.default_rng(20251)
    compared = 0
    for _ in range(150):
        sw, sh, tw, th = (int(v) for v in rng.integers(3, 40, 4))
        sfull = (int(rng.integers(-5, 5)), int(rng.integers(-5, 5)))
        sfull += (sfull[0] + sw - 1, sfull[1] + sh - 1)
        tfull = (int(rng.integers(-5, 5)), int(rng.integers(-5, 5)))
        tfull += (tfull[0] + tw - 1, tfull[1] + th - 1)
        ax, bx = sorted(int(v) for v in rng.integers(sfull[0], sfull[2] + 1, 2))
        ay, by = sorted(int(v) for v in rng.integers(sfull[1], sfull[3] + 1, 2))
        fac = tuple(float(np.float32(np.exp(rng.uniform(np.log(0.2), np.log(5.0))))) for _ in range(2))
        tp = tuple(float(np.float32(v)) for v in rng.uniform(-3, 8, 2))
        sp = tuple(float(np.float32(v)) for v in rng.uniform(-3, 8, 2))
        src = rng.uniform(-0.5, 1.5, (sh, sw, 4)).astype(np.float32)
        args = (tfull, sfull, (ax, ay, bx, by), tp, sp, fac, src)
        if not rc.scale_defined_in_reference(ref, *args[:6]):
            continue
        compared += 1
        _same(_scale(ref, *args), _scale(orc, *args), "scale %r" % (args[:6],))
    assert compared >= 100, compared


@pytest.mark.parametrize("fac", rc.SCALE_FACTORS)
def test_scaler_recorded_cases(pair, fac):
    ref, orc = pair
    _same(rc.scale_case(ref, fac), rc.scale_case(orc, fac), "scale %r" % (fac,))
    _same(rc.scale_case_f16(ref, fac), rc.scale_case_f16(orc, fac), "scale f16 %r" % (fac,))


def test_scaler_wide_target(pair):
    ref, orc = pair
    _same(rc.wide_case(ref), rc.wide_case(orc), "wide")


# ------------------------------------------------------------------ colour

@pytest.mark.parametrize("full,cur", [(rc.COLOUR_FULL, rc.COLOUR_WINDOW), ((0, 0, 40, 20), (0, 0, 40, 20)), ((-3, -2, 37, 18), (5, 5, 5, 5)),
                                      ((0, 0, 40, 20), (1, 3, 39, 3)), ((0, 0, 40, 20), (0, 0, -1, -1))])
@pytest.mark.parametrize("which", ["xyz", "srgb"])
def test_named_colour_functions(pair, full, cur, which):
    ref, orc = pair
    res = []
    for impl in (ref, orc):
        f = rc.lively_f16(np.random.default_rng(5), full, cur)
        (impl.to_xyz if which == "xyz" else impl.to_srgb)(f)
        res.append((canon_f16(f.array), rc.win_of(f)))
    _same(res[0], res[1], "colour %s %r" % (which, cur))


# ------------------------------------------------------------------ DV, workspace

def test_dv_both_directions(pair):
    ref, orc = pair
    a, b = rc.dv_cases(ref), rc.dv_cases(orc)
    for name in a:
        _same(a[name], b[name], name)


def test_workspace_three_solids(pair):
    ref, orc = pair
    _same(rc.workspace_case(ref), rc.workspace_case(orc), "workspace")
    for frame_index in (0, 9, 10):                                   # the ends of the items' span, and past it: empty
        res = []
        for impl in (ref, orc):
            out = HostFrame((0, 0, 63, 35), np.float32, fill=rc.SENTINEL_F32)
            impl.workspace(rc.workspace_layers(), frame_index, out)
            res.append((canon_f32(out.array), rc.win_of(out)))
        _same(res[0], res[1], "workspace frame %d" % frame_index)
