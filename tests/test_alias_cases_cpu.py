"""The policy table of tests/alias_cases.py held to the five headers, and its catalogue held to the table, without a GPU.

  the header walk      every pair of frame operands of every device entry the headers declare is in ALIAS_POLICY, with a class
                       that fits what the prototype says of the two operands, or the entry is in EXEMPT with a reason
  the header block     the entries include/canvas_hip.h lists per class are exactly the table's
  the catalogue        run on operands that exist as descriptions only, against a stand-in that notes what it is handed: every
                       pair is exercised in both sharing forms, its operands do arrive with equal data, full_window and
                       current_window, and every call is handed the factory's stream
  the reference side   what tests/test_aliasing_gpu.py expects of an "in place" or "shared" case -- the call on DISTINCT host
                       operands through the reference side -- reports a window with pixels and changes at least half of them:
                       an entry that left its buffer alone, or copied it, could not pass
  the refusals         the oracle's own function, called on ONE host buffer as both operands, gives other pixels than on
                       distinct operands where its loops read what they have written (the weave); the reference's blur and
                       resamplers go through a whole intermediate frame and do not, so for them the one-launch form the
                       kernels have is modelled: the refusal is the operation's, not a matter of taste"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from canvas_amd import _lib
from tests import alias_cases as ac
from tests import entry_cases as ec
from tests import reference_library as rl
from tests.test_entry_cases_cpu import HostOnly, _walk

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
HEADERS = ["canvas_hip.h", "canvas_scope.h", "canvas_lut3d.h", "canvas_perspective.h", "canvas_deinterlace.h"]
# flat arrays: the operands are the arrays `count` measures
NOT_AN_OPERAND = {("cvs_half_lookup_dev", "table_dev"): "a table of 65536 codes, whatever `count` is"}


def _text(name):
    return open(os.path.join(INCLUDE, name)).read()


def prototypes():
    """entry -> [(parameter name, type text)] for every cvs_*_dev function of the five headers whose last parameter is a stream"""
    found = {}
    for header in HEADERS:
        text = re.sub(r"/\*.*?\*/", " ", _text(header), flags=re.S)
        for name, params in re.findall(r"CVS_EXPORT\s+int\s+(cvs_\w+_dev)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
            parts = [" ".join(p.split()) for p in params.split(",")]
            if parts[-1].split()[0] != "cvs_stream_t":
                continue
            assert name not in found, name
            found[name] = [(re.search(r"(\w+)(\[\d*\])?$", p).group(1), p) for p in parts]
    return found


def operands(entry, params):
    """[(name, argument index, element type, written, several)] of the entry's frame operands; of its flat arrays where it takes no frame"""
    out = []
    for k, (name, text) in enumerate(params):
        m = re.search(r"rgba_frame_(f16|f32)", text)
        if m:
            several = text.count("*") == 2
            out.append((name, k, m.group(1), not text.startswith("const"), several))
        elif "cvs_chain_job" in text:
            out += [("out", k, "f16", True, False), ("layers", k, "f16", False, True)]
    if not out and any(text.startswith("size_t") for _n, text in params):
        for k, (name, text) in enumerate(params):
            m = re.match(r"(const )?(half|float) \*", text)
            if m and (entry, name) not in NOT_AN_OPERAND:
                out.append((name, k, m.group(2), not m.group(1), False))
    return out


def pairs_of(entry, params):
    """{(first, second): the classes the prototype allows}: a written operand against a read one of its type; two read ones"""
    ops = operands(entry, params)
    pairs = {}
    for i, (a, _ka, ta, wa, sa) in enumerate(ops):
        for j, (b, _kb, tb, wb, _sb) in enumerate(ops):
            if ta != tb or wb:
                continue
            if wa and i != j:
                pairs[(a, b)] = (ac.IN_PLACE, ac.REFUSED)
            elif not wa and (i < j or (i == j and sa)):
                pairs[(a, b)] = (ac.SHARED,)
    return pairs


def test_the_header_walk_finds_the_entries_and_their_operands():
    protos = prototypes()
    assert len(protos) >= 55, sorted(protos)                    # 48 of canvas_hip.h and 7 of the extension headers when this was written
    ops = lambda e: [(o[0], o[2], o[3], o[4]) for o in operands(e, protos[e])]
    assert ops("cvs_mix_over_f32_dev") == [("out", "f32", True, False), ("b", "f32", False, False)]
    assert ops("cvs_blur_over_f16_batch_dev") == [("outs", "f16", True, True), ("sources", "f16", False, True), ("overlays", "f16", False, True)]
    assert ops("cvs_chain_color_over_f16_dev") == [("out", "f16", True, False), ("layers", "f16", False, True)]
    assert ops("cvs_half_lookup_dev") == [("out", "half", True, False), ("in", "half", False, False)]
    assert ops("cvs_half_to_float_dev") == [("out", "float", True, False), ("in", "half", False, False)]
    assert ops("cvs_subsample_dv_dev") == [("frame", "f16", True, False)]
    assert ops("cvs_lut3d_f32_dev") == [("target", "f32", True, False), ("source", "f32", False, False)]
    assert pairs_of("cvs_deinterlace_adaptive_f16_dev", protos["cvs_deinterlace_adaptive_f16_dev"]).keys() == {
        ("out", "prev"), ("out", "cur"), ("out", "next"), ("prev", "cur"), ("prev", "next"), ("cur", "next")}


def test_every_pair_of_every_entry_has_a_policy_or_the_entry_is_exempt_for_a_reason():
    protos = prototypes()
    both = sorted(set(ac.ALIAS_POLICY) & set(ac.EXEMPT))
    assert not both, "in the policy table and exempt at once: %r" % both
    stale = sorted((set(ac.ALIAS_POLICY) | set(ac.EXEMPT)) - set(protos))
    assert not stale, "named by the tables, declared by no header: %r" % stale
    for entry, params in sorted(protos.items()):
        pairs = pairs_of(entry, params)
        if not pairs:
            assert entry in ac.EXEMPT, "%s has no pair of operands that could share a buffer and EXEMPT does not say why" % entry
            assert isinstance(ac.EXEMPT[entry], str) and len(ac.EXEMPT[entry].split()) >= 3, entry
            continue
        assert entry in ac.ALIAS_POLICY, "%s: %r have no policy" % (entry, sorted(pairs))
        policy = ac.ALIAS_POLICY[entry]
        assert set(policy) == set(pairs), "%s: the table has %r, the prototype %r" % (entry, sorted(policy), sorted(pairs))
        for p, allowed in pairs.items():
            assert policy[p] in allowed, "%s %r: %r, the prototype allows %r" % (entry, p, policy[p], allowed)
    for key, reason in ac.IDENTITY.items():
        assert ac.ALIAS_POLICY[key[0]][key[1]] == ac.IN_PLACE and len(reason.split()) >= 3
    named = [c.what for _gid, c in _all_cases(Noting()) if c.identity]
    assert len(named) == len(ac.GEOMETRIES) + 2, named          # the copy at each geometry; the one-layer plain chain, out == its layer


def header_block():
    """{class: {(entry, pair)}} as the block "Operands that share a buffer" of include/canvas_hip.h lists them"""
    text = _text("canvas_hip.h")
    block = re.search(r"/\* Operands that share a buffer.*?\*/", text, flags=re.S).group(0)
    listed = {}
    sections = re.split(r"\n \*   (in place|refused|shared):\n", block)
    for cls, body in zip(sections[1::2], sections[2::2]):
        body = body.split("\n * Every other device entry")[0]
        found = set()
        for entry, tail in re.findall(r"(cvs_\w+_dev)((?: \(\w+, \w+\))+)", body):
            found |= {(entry, (a, b)) for a, b in re.findall(r"\((\w+), (\w+)\)", tail)}
        assert cls not in listed
        listed[cls] = found
        assert re.sub(r"(cvs_\w+_dev)((?: \(\w+, \w+\))+)", "", body).strip(" *;\n/") == "", "the %s list holds something that is no entry: %r" % (cls, body)
    return listed


def test_the_header_block_lists_exactly_the_table():
    listed = header_block()
    assert set(listed) == {ac.IN_PLACE, ac.REFUSED, ac.SHARED}
    for cls in listed:
        table = {(e, p) for e, pairs in ac.ALIAS_POLICY.items() for p, c in pairs.items() if c == cls}
        assert listed[cls] == table, "%s: only in the header %r, only in the table %r" % (cls, sorted(listed[cls] - table), sorted(table - listed[cls]))
    block = re.search(r"/\* Operands that share a buffer.*?\*/", _text("canvas_hip.h"), flags=re.S).group(0)
    for wording in ac.WORDINGS:
        assert wording in " ".join(block.replace("\n *", " ").split()), wording
    for header in HEADERS[1:]:
        assert "Operands that share a buffer" in _text(header), "%s does not point to the block" % header


# ------------------------------------------------------------------ the catalogue's shape

class Noting:
    """Stands in for the library: every function returns 0 and is noted with its arguments and the frames found in them."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            seen = []
            for k, a in enumerate(args):
                _walk(a, k, seen, 0)
            self.calls.append((name, args, [(k, v) for k, kind, v in seen if kind == "frame"]))
            return 0
        return call


def _all_cases(lib):
    return [(gid, case) for gid, build in ac.GROUPS for case in build(lib)]


def _slots(entry, name, protos, args, frames):
    """what arrives as operand `name`: [(data, full_window, current_window)], or [address] for a flat array"""
    for oname, k, _type, _written, _several in operands(entry, protos[entry]):
        if oname != name:
            continue
        got = [v for kk, v in frames if kk == k]
        if "cvs_chain_job" in protos[entry][k][1]:
            return got[:1] if name == "out" else got[1:]
        return got if got else [args[k]]
    raise AssertionError("%s has no operand %r" % (entry, name))


def test_the_catalogue_exercises_every_pair_in_both_forms_on_operands_that_do_share():
    protos = prototypes()
    lib = Noting()
    stream = 0x5EED
    seen = {}
    names = set()
    for gid, case in _all_cases(lib):
        assert case.what not in names, case.what
        names.add(case.what)
        assert case.policy == ac.ALIAS_POLICY[case.entry][case.pair]
        specs = {}
        for form in ("distinct",) + ac.FORMS:
            before = len(lib.calls)
            fac = HostOnly(lib, stream)
            assert case(fac, form) == 0
            assert len(lib.calls) == before + 1, "%s, %s: not ONE call" % (case.what, form)
            name, args, frames = lib.calls[-1]
            assert name == case.entry, "%s calls %s" % (case.what, name)
            assert args[-1] == stream, "%s, %s: the entry is not handed the factory's stream" % (case.what, form)
            first, second = (_slots(case.entry, n, protos, args, frames) for n in case.pair)
            if case.pair[0] == case.pair[1]:                       # two positions of one table
                common = [v for v in set(first) if first.count(v) > 1]
            else:
                common = [v for v in first if v in second]
            if form == "distinct":
                datas = [v[0] if isinstance(v, tuple) else v for v in first + second]
                assert not common and (case.pair[0] == case.pair[1] or len(set(datas)) == len(datas)), "%s: the distinct form shares" % case.what
            else:
                assert common, "%s, %s: %r and %r arrive as %r and %r" % (case.what, form, case.pair[0], case.pair[1], first, second)
                seen.setdefault((case.entry, case.pair), set()).add(form)
            specs[form] = [(o.cls, o.name, o.out, o.cmp, o.nbytes) for o in fac.objects if not o.name.startswith(ac.DISTINCT)]
            assert any(o.out for o in fac.objects), case.what
            if form != "distinct":
                assert not any(o.name.startswith(ac.DISTINCT) for o in fac.objects)
        assert specs["distinct"] == specs["one struct"] == specs["two structs"], "%s: the forms are not one case" % case.what
    for entry, pairs in ac.ALIAS_POLICY.items():
        for p in pairs:
            assert seen.get((entry, p)) == set(ac.FORMS), "%s %r is run in %r" % (entry, p, seen.get((entry, p)))


def test_every_pair_is_run_on_a_whole_buffer_and_on_a_window_inside_one_from_an_odd_column():
    lib = Noting()
    whole, inside = set(), set()
    for _gid, case in _all_cases(lib):
        fac = HostOnly(lib, 1)
        case(fac, "one struct")
        for _k, (data, full, cur) in lib.calls[-1][2]:
            if cur == full:
                whole.add((case.entry, case.pair))
            if cur[0] > full[0] and cur[1] > full[1] and cur[2] < full[2] and cur[3] < full[3] and cur[0] % 2 == 1:
                inside.add((case.entry, case.pair))
            assert full[2] - full[0] < 300 and full[3] - full[1] < 41, case.what
    # the weave's second field is allocated for the frame's window: operands that share a buffer have the whole buffer as window
    only_whole = {("cvs_weave_fields_f16_dev", ("frame", "other"))}
    flat = {("cvs_half_lookup_dev", ("out", "in"))}
    every = {(e, p) for e, pairs in ac.ALIAS_POLICY.items() for p in pairs}
    assert every - whole == flat, sorted(every - whole - flat)
    assert every - inside == flat | only_whole, sorted(every - inside - flat - only_whole)


# ------------------------------------------------------------------ the reference side alone

class Remembering(rl.OnHostWithBuffers):
    """OnHostWithBuffers that keeps what every operand held when it was made."""

    def _make_frame(self, o, host):
        rl.OnHostWithBuffers._make_frame(self, o, host)
        o.initial = o.frame.array.copy()

    def _make_buffer(self, o, data):
        rl.OnHostWithBuffers._make_buffer(self, o, data)
        o.initial = o.array.copy()


def _changed(o):
    """(pixels of the reported window, those that differ from what the buffer held before): elements, for a flat array"""
    if o.frame is None:
        a, b = o.array.view(np.uint16), o.initial.view(np.uint16)
        return a.size, int((a != b).sum())
    w, full = o.frame.current_window, o.frame.full_window
    if w.is_empty():
        return 0, 0
    ys, xs = slice(w.min.y - full.min.y, w.max.y - full.min.y + 1), slice(w.min.x - full.min.x, w.max.x - full.min.x + 1)
    raw = lambda a: np.ascontiguousarray(a[ys, xs]).view(np.uint8).reshape(a[ys, xs].shape[0], a[ys, xs].shape[1], -1)
    differ = (raw(o.frame.array) != raw(o.initial)).any(axis=2)
    return differ.size, int(differ.sum())


GROUP_IDS = [g[0] for g in ac.GROUPS]


@pytest.mark.parametrize("gid", GROUP_IDS)
def test_the_reference_alone_reports_a_window_and_changes_half_of_it(gid):
    build = dict(ac.GROUPS)[gid]
    for case in build(ac.Reference()):
        if case.policy == ac.REFUSED:
            continue
        fac = Remembering(None)
        assert case(fac, "distinct") == 0
        for o in fac.objects:
            if not o.out:
                held = o.frame.array if o.frame is not None else o.array
                assert np.array_equal(held.view(np.uint8), o.initial.view(np.uint8)), "%s: the reference wrote %s" % (case.what, o.name)
                continue
            pixels, changed = _changed(o)
            assert pixels > 0, "%s: %s reports no window" % (case.what, o.name)
            if case.identity:
                assert changed == 0, "%s: %s is no longer its input" % (case.what, o.name)
            else:
                assert 2 * changed >= pixels, "%s: only %d of %d pixels of %s differ from what it held" % (case.what, changed, pixels, o.name)


# ------------------------------------------------------------------ earning each refusal

def _oracle_in_place():
    """entry -> ([cases whose truly in-place result differs from the distinct call's], [cases where it does not]) for the
    refused entries of reference_library.ORACLE, under no pin"""
    lib = rl.OracleAsLibrary()
    out = {}
    for _gid, build in ac.GROUPS:
        for case in build(lib):
            if case.policy != ac.REFUSED or case.entry not in rl.ORACLE or case.pin is not None:
                continue
            apart, together = rl.OnHost(None), rl.OnHost(None)
            assert case(apart, "distinct") == 0 and case(together, "one struct") == 0
            want, got = apart.objects[0], together.objects[0]
            assert want.out and got.out and want.name == got.name
            w, full = want.frame.current_window, want.frame.full_window
            assert not w.is_empty(), case.what
            ys, xs = slice(w.min.y - full.min.y, w.max.y - full.min.y + 1), slice(w.min.x - full.min.x, w.max.x - full.min.x + 1)
            a, b = np.ascontiguousarray(want.frame.array[ys, xs]), np.ascontiguousarray(got.frame.array[ys, xs])
            same = np.array_equal(a.view(np.uint8), b.view(np.uint8)) and w.tuple() == got.frame.current_window.tuple()
            out.setdefault(case.entry, ([], []))[1 if same else 0].append(case.what)
    return out


def test_the_oracle_called_truly_in_place():
    """The reference's own loops on ONE host buffer as both operands against the same call on distinct operands.

    The weave reads its second field min.x pixels before the pixel it writes (Pulldown23RemovalFilter.c:101): in place, from an
    odd first column, it gives other pixels -- the refusal is the operation's.  The oracle's blur, Lanczos resampler and scaler
    CAN be called this way and give the distinct call's pixels: they run two passes through a whole intermediate frame, so
    nothing is read after the target is first written.  The kernels have no such frame between the passes; their case is
    test_one_launch_of_a_gather_in_place_reads_what_its_neighbours_wrote below.  The other refused entries (matte, warps, field
    conversions, deinterlace) have no oracle function; each gathers the rows or columns around a pixel in one launch, which is
    the same argument."""
    found = _oracle_in_place()
    assert set(found) == {"cvs_fir_blur_f32_dev", "cvs_resample_lanczos_f32_dev", "cvs_scale_bilinear_f32_dev", "cvs_weave_fields_f16_dev"}
    differs, same = found["cvs_weave_fields_f16_dev"]
    assert differs and all("odd column" in what for what in differs) and all("odd column" not in what for what in same), (differs, same)
    for entry in ("cvs_fir_blur_f32_dev", "cvs_resample_lanczos_f32_dev", "cvs_scale_bilinear_f32_dev"):
        assert not found[entry][0] and found[entry][1], "%s: the oracle no longer goes through a whole intermediate frame: %r" % (entry, found[entry][0])


def _blur_by_workgroups(source, target, taps, strip, segment):
    """kernels/blur_kernel.hpp:9-19 as a schedule: one workgroup per strip of `strip` columns and segment of `segment` rows,
    one after the other; each reads its pixels and the NT-1 halo columns and rows around them from `source` when it runs, forms
    the separable sum in float32 (taps outside the buffer skipped) and stores its pixels into `target`."""
    h, w = source.shape[:2]
    c = len(taps) // 2
    for y0 in range(0, h, segment):
        for x0 in range(0, w, strip):
            y1, x1 = min(y0 + segment, h), min(x0 + strip, w)
            ya, yb, xa, xb = max(y0 - c, 0), min(y1 + c, h), max(x0 - c, 0), min(x1 + c, w)
            tile = source[ya:yb, xa:xb].copy()
            rows = np.zeros((yb - ya, x1 - x0, 4), np.float32)
            for k, t in enumerate(taps):
                for x in range(x0, x1):
                    sx = x - c + k
                    if 0 <= sx < w:
                        rows[:, x - x0] += np.float32(t) * tile[:, sx - xa]
            res = np.zeros((y1 - y0, x1 - x0, 4), np.float32)
            for k, t in enumerate(taps):
                for y in range(y0, y1):
                    sy = y - c + k
                    if 0 <= sy < h:
                        res[y - y0] += np.float32(t) * rows[sy - ya]
            target[y0:y1, x0:x1] = res


def test_one_launch_of_a_gather_in_place_reads_what_its_neighbours_wrote():
    """Why the entries of host/scale.c refuse a target that is the source's buffer.  k_blur, like every one-launch kernel behind
    them, has no frame between its passes: a workgroup reads halo columns and rows that belong to its neighbours.  With the
    target in the source's buffer, a neighbour that ran earlier has stored over them.  On a frame one workgroup covers the
    result is right -- which is why a small test would pass by luck, and why the order of the workgroups, which nothing pins
    on a device, decides the rest."""
    rng = np.random.default_rng(5000)
    taps = ec._taps(9)
    src = rng.uniform(0.0, 1.0, (24, 40, 4)).astype(np.float32)
    want = np.empty_like(src)
    _blur_by_workgroups(src, want, taps, 16, 8)
    one = src.copy()
    _blur_by_workgroups(one, one, taps, 64, 32)                      # one workgroup: in place, and right
    assert np.array_equal(one, want)
    many = src.copy()
    _blur_by_workgroups(many, many, taps, 16, 8)
    wrong = (many != want).any(axis=2)
    assert wrong.any() and not wrong[:8, :12].any(), "the first workgroup's own pixels, away from its neighbours, are right"
    # every later workgroup has pixels within four columns or rows of an earlier one's
    assert wrong[8:, :].any() and wrong[:, 16:].any()
