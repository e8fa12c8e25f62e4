"""The secondaries' catalogue of device-entry calls, in the form of tests/entry_cases.py and tests/primary_cases.py: a case is a
function case(fac) that makes ONE call of cvs_qualify_f16_dev / _f32_dev or cvs_matte_mix_f16_dev / _f32_dev
(include/canvas_secondary.h) on operands it takes from a factory, in the same order every time, on the stream fac.stream, and
returns the entry's return code.  So the harnesses that run the catalogue -- frames packed into a guarded arena, a stream that
records and replays, windows far from the origin -- run these calls with no harness code of their own
(tests/test_secondary_harness_gpu.py), and tests/test_secondary_cpu.py holds the cases to the header without a GPU.

Every case's description is also what tests/test_secondary_gpu.py needs to compute the model's answer: CASES[what] holds it."""
import ctypes as C

import numpy as np

from canvas_amd import _lib
from canvas_amd.abi import HostFrame
from tests import secondary_model as sm
from tests.entry_cases import _ANY, DISPLAY_GEOMETRIES, SPECIALS16, SPECIALS32, _box, _stream_geometries, all_codes, blank

ENTRIES = ("cvs_matte_mix_f16_dev", "cvs_matte_mix_f32_dev", "cvs_qualify_f16_dev", "cvs_qualify_f32_dev")
WIDTHS = [1, 2, 129, 130]
HEIGHTS = [1, 9]
# per-pixel maps: far from the origin they give the origin's bytes (tests/entry_cases.py FAR_CLASSES: "equivariant", any offset
# within CVS_MAX_COORD)
FAR_RULE = _ANY
INF = float("inf")
ALL = dict(hue=(350.0, 40.0, 20.0), saturation=(0.2, INF, 0.1, 0.0), luma=(0.1, 0.9, 0.05, 0.1))
# between them: each axis alone and all three together; a hue range that wraps through 0 (center 350, width 40); width 360; hard
# and soft edges on each side; high = +inf; invert and show-matte; no axis at all
QUALIFIERS = [
    sm.Qualifier(hue=(120.0, 60.0, 30.0)),
    sm.Qualifier(hue=(350.0, 40.0, 0.0)),
    sm.Qualifier(hue=(200.0, 360.0, 0.0)),
    sm.Qualifier(saturation=(0.3, 0.8, 0.1, 0.2)),
    sm.Qualifier(saturation=(0.25, 1.0, 0.0, 0.0)),
    sm.Qualifier(luma=(0.25, INF, 0.125, 0.0)),
    sm.Qualifier(luma=(0.2, 0.7, 0.0, 0.25)),
    sm.Qualifier(**ALL),
    sm.Qualifier(invert=True, **ALL),
    sm.Qualifier(hue=(-30.0, 90.0, 15.0), show_matte=True),
    sm.Qualifier(invert=True, show_matte=True, **ALL),
    sm.Qualifier(hue=(350.0, 40.0, 20.0), luma=(0.5, 0.5, 0.25, 0.25), invert=True),
    sm.Qualifier(),
]
KEYS = ["distinct", "absent", "source"]
MIXES = [(False, False), (True, False), (False, True), (True, True)]         # (luma, invert)
# what the model needs of every case: CASES[what] = dict(op=..., half=..., frames in the order the case asks for them, ...)
CASES = {}


def picture(rng, half, full, cur=None):
    """Colours spread over [-0.125, 1.125] (every hue, saturation and luma), alphas over [0, 1] with exact 0s and 1s among them;
    greys, pixels with two equal largest channels and pure primaries; and the special codes, NaN and Inf among them."""
    h, w = _box(full)
    a = rng.uniform(-0.125, 1.125, (h, w, 4)).astype(np.float32)
    a[..., 3] = np.clip(rng.uniform(-0.25, 1.25, (h, w)), 0.0, 1.0)
    kind = rng.integers(0, 40, (h, w))
    a[kind == 0, 1] = a[kind == 0, 0]                                   # r == g
    a[kind == 1, 2] = a[kind == 1, 1]                                   # g == b
    grey = kind == 2
    a[grey, 0] = a[grey, 1] = a[grey, 2]
    primaries = np.array([[1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 1, 1], [0, 0, 1], [1, 0, 1], [0, 0, 0]], np.float32)
    pure = kind == 3
    a[pure, :3] = primaries[rng.integers(0, len(primaries), int(pure.sum()))]
    if half:
        with np.errstate(over="ignore"):
            codes = a.astype(np.float16).view(np.uint16).copy()
        hit = rng.uniform(size=codes.shape) < 0.02
        codes[hit] = SPECIALS16[rng.integers(0, len(SPECIALS16), int(hit.sum()))]
        return HostFrame(full, np.uint16, codes, full if cur is None else cur)
    hit = rng.uniform(size=a.shape) < 0.01
    a[hit] = SPECIALS32[rng.integers(0, len(SPECIALS32), int(hit.sum()))]
    return HostFrame(full, np.float32, a, full if cur is None else cur)


def params(q):
    return _lib.qualifier(q.hue, q.saturation, q.luma, q.invert, q.show_matte)


def _narrowed(cur, n):
    """another input's current window: one column off the right (n odd) or the left (n even) where there are more than two, and a
    row off the top (n odd) or the bottom where there are more than two: the entries work on the intersection"""
    x0, y0, x1, y1 = cur
    if x1 - x0 >= 2:
        x0, x1 = (x0, x1 - 1) if n % 2 else (x0 + 1, x1)
    if y1 - y0 >= 2:
        y0, y1 = (y0 + 1, y1) if n % 2 else (y0, y1 - 1)
    return (x0, y0, x1, y1)


def _wider(full, n):
    """another input's buffer: every other case one column more on the left, so that its pairs sit on the other parity"""
    return (full[0] - 1, full[1], full[2], full[3]) if n % 2 else full


def _qualify(cvs, half):
    return cvs.cvs_qualify_f16_dev if half else cvs.cvs_qualify_f32_dev


def _mix(cvs, half):
    return cvs.cvs_matte_mix_f16_dev if half else cvs.cvs_matte_mix_f32_dev


def qualify(cvs, half):
    """Streams of 1, 2, 129 and 130 columns, 1 and 9 rows, over the stream geometries; the qualifiers and the three key modes in
    turn; out of place, and -- every other case -- in place on the source and, with a distinct key frame, on the key; for halfs
    also key frames that hold every half code."""
    cases, n = [], 0
    cmp = "f16" if half else "f32"
    fmt = "f16" if half else "f32"
    for width in WIDTHS:
        for height in HEIGHTS:
            for g, (sfull, scur, tfull) in enumerate(_stream_geometries(width, height)):
                q = QUALIFIERS[n % len(QUALIFIERS)]
                key = KEYS[(n // 2) % len(KEYS)]
                kfull, kcur = _wider(sfull, n), _narrowed(scur, n)
                seed = 2600 + n
                p = params(q)
                for place in (["out", "source", "key"] if g % 2 == 0 else ["out"]):
                    if place == "key" and key != "distinct":
                        continue
                    what = "qualify %s %dx%d %s key %s %r %r" % (fmt, width, height, place, key, q, (sfull, scur, tfull))

                    def case(fac, place=place, key=key, sfull=sfull, scur=scur, tfull=tfull, kfull=kfull, kcur=kcur, seed=seed, p=p):
                        rng = np.random.default_rng(seed)
                        src = fac.frame(picture(rng, half, sfull, scur), out=place == "source", cmp=cmp, in_place=place == "source")
                        k = fac.frame(picture(rng, half, kfull, kcur), out=place == "key", cmp=cmp, in_place=place == "key") if key == "distinct" else None
                        out = {"out": None, "source": src, "key": k}[place]
                        if out is None:
                            out = fac.frame(blank(half, tfull), out=True, cmp=cmp)
                        kref = {"absent": None, "source": src.ref(), "distinct": None if k is None else k.ref()}[key]
                        return _qualify(cvs, half)(out.ref(), src.ref(), kref, C.byref(p), fac.stream)
                    CASES[what] = dict(op="qualify", half=half, place=place, key=key, q=q, seed=seed, sfull=sfull, scur=scur, tfull=tfull, kfull=kfull, kcur=kcur)
                    cases.append((what, case))
                n += 1
    if half:
        for k, (full, cur) in enumerate(DISPLAY_GEOMETRIES[1:]):
            q = QUALIFIERS[(7 + k) % len(QUALIFIERS)]
            p = params(q)
            what = "qualify all codes %r %r" % (q, (full, cur))

            def codes(fac, full=full, cur=cur, p=p, k=k):
                src = fac.frame(picture(np.random.default_rng(2900 + k), True, full, full))
                key = fac.frame(all_codes(full, cur))
                out = fac.frame(blank(True, full), out=True, cmp="f16")
                return cvs.cvs_qualify_f16_dev(out.ref(), src.ref(), key.ref(), C.byref(p), fac.stream)
            CASES[what] = dict(op="qualify codes", half=True, q=q, seed=2900 + k, full=full, cur=cur)
            cases.append((what, codes))
    return cases


def matte_mix(cvs, half):
    """The same streams; by alpha and by luma, plain and inverted, in turn; three inputs whose buffers and current windows
    differ; out of place, and -- every other case -- in place on a, on b and on the matte; for halfs also mattes that hold
    every half code."""
    cases, n = [], 0
    cmp = "f16" if half else "f32"
    fmt = "f16" if half else "f32"
    for width in WIDTHS:
        for height in HEIGHTS:
            for g, (sfull, scur, tfull) in enumerate(_stream_geometries(width, height)):
                luma, invert = MIXES[n % len(MIXES)]
                fulls = [sfull, _wider(sfull, n), sfull]
                curs = [scur, _narrowed(scur, n), _narrowed(scur, n + 1)]
                seed = 3300 + n
                p = _lib.matte_mix(luma, invert)
                for place in (["out", "a", "b", "matte"] if g % 2 == 0 else ["out"]):
                    what = "mix %s %dx%d %s luma %r invert %r %r" % (fmt, width, height, place, luma, invert, (sfull, scur, tfull))

                    def case(fac, place=place, fulls=fulls, curs=curs, tfull=tfull, seed=seed, p=p):
                        rng = np.random.default_rng(seed)
                        ins = [fac.frame(picture(rng, half, full, cur), out=place == name, cmp=cmp, in_place=place == name)
                               for name, full, cur in zip(("a", "b", "matte"), fulls, curs)]
                        out = dict(zip(("a", "b", "matte"), ins)).get(place)
                        if out is None:
                            out = fac.frame(blank(half, tfull), out=True, cmp=cmp)
                        return _mix(cvs, half)(out.ref(), ins[0].ref(), ins[1].ref(), ins[2].ref(), C.byref(p), fac.stream)
                    CASES[what] = dict(op="mix", half=half, place=place, luma=luma, invert=invert, seed=seed, fulls=fulls, curs=curs, tfull=tfull)
                    cases.append((what, case))
                n += 1
    if half:
        for k, (full, cur) in enumerate(DISPLAY_GEOMETRIES[1:]):
            luma, invert = MIXES[k % len(MIXES)]
            p = _lib.matte_mix(luma, invert)
            what = "mix all codes luma %r invert %r %r" % (luma, invert, (full, cur))

            def codes(fac, full=full, cur=cur, p=p, k=k):
                rng = np.random.default_rng(3600 + k)
                a, b = fac.frame(picture(rng, True, full, full)), fac.frame(picture(rng, True, full, full))
                matte = fac.frame(all_codes(full, cur))
                out = fac.frame(blank(True, full), out=True, cmp="f16")
                return cvs.cvs_matte_mix_f16_dev(out.ref(), a.ref(), b.ref(), matte.ref(), C.byref(p), fac.stream)
            CASES[what] = dict(op="mix codes", half=True, luma=luma, invert=invert, seed=3600 + k, full=full, cur=cur)
            cases.append((what, codes))
    return cases


GROUPS = [("%s[%s]" % (name, fmt), lambda cvs, build=build, half=half: build(cvs, half))
          for name, build in (("qualify", qualify), ("matte_mix", matte_mix)) for fmt, half in (("f16", True), ("f32", False))]


def expected(what):
    """The model's answer to a case: (the written frame's pixels after the call, its window or None)"""
    d = CASES[what]
    half = d["half"]
    rng = np.random.default_rng(d["seed"])
    if d["op"] == "qualify":
        src = picture(rng, half, d["sfull"], d["scur"]).array
        key = picture(rng, half, d["kfull"], d["kcur"]).array if d["key"] == "distinct" else None
        before, tfull = {"out": (blank(half, d["tfull"]).array, d["tfull"]), "source": (src, d["sfull"]), "key": (key, d["kfull"])}[d["place"]]
        if d["key"] == "distinct":
            return sm.expected_qualify(before, tfull, src, d["sfull"], d["scur"], d["q"], key, d["kfull"], d["kcur"])
        return sm.expected_qualify(before, tfull, src, d["sfull"], d["scur"], d["q"])
    if d["op"] == "mix":
        ins = [picture(rng, half, full, cur).array for full, cur in zip(d["fulls"], d["curs"])]
        at = {"a": 0, "b": 1, "matte": 2}.get(d["place"])
        before, tfull = (blank(half, d["tfull"]).array, d["tfull"]) if at is None else (ins[at], d["fulls"][at])
        args = [v for trio in zip(ins, d["fulls"], d["curs"]) for v in trio]
        return sm.expected_mix(before, tfull, *args, luma=d["luma"], invert=d["invert"])
    full, cur = d["full"], d["cur"]
    if d["op"] == "qualify codes":
        src = picture(rng, True, full, full).array
        return sm.expected_qualify(blank(True, full).array, full, src, full, full, d["q"], all_codes(full, cur).array, full, cur)
    a, b = picture(rng, True, full, full).array, picture(rng, True, full, full).array
    return sm.expected_mix(blank(True, full).array, full, a, full, full, b, full, full, all_codes(full, cur).array, full, cur, luma=d["luma"], invert=d["invert"])
