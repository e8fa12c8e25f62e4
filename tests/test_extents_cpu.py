"""What tests/test_extents_gpu.py takes for granted, established without a GPU (DESIGN.md "Extents"): the expectations it
applies to windows taller or wider than a picture are what the reference side computes there, and the reference side has no
extent problem of its own up to the sizes used.

Every case of tests/extent_cases.py runs on tests/reference_library.py alone: reported windows inside their buffers, inputs
unwritten, the target no longer the sentinel anywhere in the reported window (the reference found its source at that extent).
Then rows [a, b] of the tall result are compared with the same case run on that band of rows alone, grown by the group's halo.
Last, the catalogue is held to the headers, as tests/test_entry_cases_cpu.py holds entry_cases.GROUPS."""
import re

import numpy as np
import pytest

from canvas_amd.abi import HostFrame
from tests import entry_cases as ec
from tests import extent_cases as xc
from tests import fields_model as fm
from tests import reference_library as rl
from tests.test_entry_cases_cpu import HEADER, HostOnly, Recorder, declared, header_files

# (group prefix, (width, height)) -> the reference's file and line, where its own `int` code is undefined at that extent and
# the extent is kept out for that group only.  At most one pair in ten, and no group may lose both 65 536 and 70 001 rows.
REFERENCE_UNDEFINED = {}

PAIRS = [(gid, pin, build, extent) for gid, pin, build, extents, _halo in xc.GROUPS for extent in extents
         if (gid.split("[")[0], extent) not in REFERENCE_UNDEFINED]
IDS = ["%s-%dx%d" % (gid, e[0], e[1]) for gid, _p, _b, e in PAIRS]


def reference_run(case, fac=None):
    """The case on the reference side -> (factory, buffers after the call)."""
    fac = fac or rl.OnHostWithBuffers(None)
    assert case(fac) == 0
    return fac, fac.collect()


def check_reference_run(label, fac, hosts, got):
    """hosts: what every operand was made of.  Windows inside buffers; inputs unwritten; outputs written all over their window."""
    for o, h, g in zip(fac.objects, hosts, got):
        if o.frame is None:                                   # a flat buffer: an input unwritten, an output no longer what it held
            assert (g.tobytes() == h.tobytes()) == (not o.out), "%s: %s %s" % (label, o.name, "is as it was" if o.out else "was written")
            continue
        w, full = o.frame.current_window, h.full_window
        assert w.is_empty() or (full.min.x <= w.min.x and w.max.x <= full.max.x and full.min.y <= w.min.y and w.max.y <= full.max.y), \
            "%s: %s reports %r" % (label, o.name, w.tuple())
        if not o.out:
            assert g.tobytes() == h.array.tobytes(), "%s: %s was written" % (label, o.name)
            continue
        assert not w.is_empty(), "%s: %s has an empty window" % (label, o.name)
        inside = g[w.min.y - full.min.y:w.max.y - full.min.y + 1, w.min.x - full.min.x:w.max.x - full.min.x + 1]
        if o.reads:                                           # worked on in place: no sentinel to lose; something must have changed
            before = h.array[w.min.y - full.min.y:w.max.y - full.min.y + 1, w.min.x - full.min.x:w.max.x - full.min.x + 1]
            assert inside.tobytes() != before.tobytes(), "%s: %s is as it was" % (label, o.name)
            continue
        sentinel = ec.SENT16 if g.dtype == np.uint16 else ec.SENT32
        left = np.flatnonzero((inside == sentinel).all(axis=2).any(axis=1))
        assert left.size == 0, "%s: %s keeps the sentinel in %d rows of its window, first row %d" % (label, o.name, left.size, left[0] + w.min.y)


class Keeping(rl.OnHostWithBuffers):
    """OnHost that keeps what every operand was made of."""

    def __init__(self, cvs):
        rl.OnHostWithBuffers.__init__(self, cvs)
        self.hosts = []

    def frame(self, host, **kw):
        self.hosts.append(host)
        return rl.OnHostWithBuffers.frame(self, host, **kw)

    def buffer(self, data, cls, **kw):
        self.hosts.append(np.ascontiguousarray(data).view(np.uint8).reshape(-1).copy())
        return rl.OnHostWithBuffers.buffer(self, data, cls, **kw)


class Band(Keeping):
    """Every frame cut down to rows y0 .. y1 (its windows with it), every box likewise: the same case on a band of rows alone."""

    def __init__(self, cvs, y0, y1):
        Keeping.__init__(self, cvs)
        self.y0, self.y1 = y0, y1

    def _cut(self, b):
        return (b[0], max(b[1], self.y0), b[2], min(b[3], self.y1))

    def frame(self, host, **kw):
        full = host.full_window.tuple()
        part = self._cut(full)
        assert part[1] <= part[3]
        cur = host.current_window.tuple()
        cur = self._cut(cur) if cur[2] >= cur[0] and cur[3] >= cur[1] else cur
        if cur[3] < cur[1]:
            cur = (0, 0, -1, -1)
        cut = HostFrame(part, host.dtype, host.array[part[1] - full[1]:part[3] - full[1] + 1].copy(), cur)
        return Keeping.frame(self, cut, **kw)

    def box(self, x0, y0, x1, y1):
        return ec.Factory.box(self, *self._cut((x0, y0, x1, y1)))


@pytest.mark.parametrize("gid,pin,build,extent", PAIRS, ids=IDS)
def test_the_reference_at_every_extent(gid, pin, build, extent):
    halo = next(g[4] for g in xc.GROUPS if g[0] == gid)
    width, height = extent
    for what, case in build(rl.ReferenceLibrary(), width, height):
        fac, got = reference_run(case, Keeping(None))
        check_reference_run(what, fac, fac.hosts, got)
        if halo is None or height < 4096:
            continue
        # the reference at a large extent is the reference at a small one: two bands, one across row 65 535 where the frame
        # has it, one at the frame's last rows; rows a .. b must not depend on anything but rows a - halo .. b + halo
        for a, b in {(min(65530, height - 40), min(65541, height - 30)), (height - 12, height - 1)}:
            band = Band(None, a - halo, b + halo)
            assert case(band) == 0
            small = band.collect()
            for o, g, s, h in zip(fac.objects, got, small, band.hosts):
                if not o.out or o.frame is None:
                    continue
                top = h.full_window.min.y
                assert g[a:b + 1].tobytes() == s[a - top:b + 1 - top].tobytes(), "%s: rows %d..%d of %s are not those of the band alone" % (what, a, b, o.name)


def test_the_vectorised_field_model_is_the_model():
    """reference_library.field_to_frame restates fields_model.field_to_frame without its Python loop over rows."""
    import oracle
    rng = np.random.default_rng(5)
    for h in (1, 2, 3, 4, 9, 10):
        for y0 in (0, 1, -3):
            cur = ec.px16(rng, (0, 0, 4, h - 1)).array
            for field in (0, 1):
                want = fm.field_to_frame(cur, y0, field, oracle.float_to_half)
                assert rl.field_to_frame(cur, y0, field).tobytes() == want.tobytes(), (h, y0, field)


def test_the_undefined_table_is_within_its_cap():
    total = sum(len(g[3]) for g in xc.GROUPS)
    assert len(REFERENCE_UNDEFINED) * 10 <= total
    for prefix in {p for p, _e in REFERENCE_UNDEFINED}:
        lost = {e for p, e in REFERENCE_UNDEFINED if p == prefix}
        assert not ({(2, 65536), (3, 70001)} <= lost), prefix
    for reason in REFERENCE_UNDEFINED.values():
        assert re.search(r"\.c:\d+", reason), reason


def test_the_tallest_raster_alone_is_above_the_table_line():
    """Which rasters of the edge groups run which table placement, from kernels/table_placement.hpp's own constant: every raster
    but the tallest of each list is gathered through L2, the tallest -- two columns wide -- stages the table into LDS."""
    import os
    text = open(os.path.join(os.path.dirname(os.path.dirname(HEADER)), "canvas_amd", "csrc", "kernels", "table_placement.hpp")).read()
    shift = re.search(r"constexpr long long kGatherUpTo = 1LL << (\d+);", text)
    assert shift and re.search(r"pixels <= kGatherUpTo \? kTableL2 : kTableLds", text)
    line = 1 << int(shift.group(1))
    for rasters in (xc.YCC422_RASTERS, xc.YCC420_RASTERS):
        assert [w * h > line for w, h in rasters] == [False] * (len(rasters) - 1) + [True] and rasters[-1][0] == 2
    assert all(w * h <= line for w, h in xc.YCC_FEW)


def frame_taking_entries(texts=None):
    """Every cvs_*_dev function of every header (include/canvas*.h, found by glob) that takes a frame and a stream."""
    found = set()
    for text in texts if texts is not None else [open(name).read() for name in header_files()]:
        for entry, params in declared(text):
            if "rgba_frame_f" in params or "cvs_chain_job" in params:
                found.add(entry)
    return found


# the edges' rasters have even widths: what reaches them at 70 001 columns and more is a raster of 70 002
AT_EXTENT = {(2, 65536): [(2, 65536)], (70001, 3): [(70001, 3), (70002, 3), (70002, 4)]}


def test_every_frame_taking_entry_is_reached_at_both_extents():
    """At 65 536 rows and at 70 001 columns, by a call the stand-in sees; the DV pair is the only exemption (no extent to vary)."""
    entries = frame_taking_entries()
    assert len(entries) >= 47 and "cvs_scope_counts_f16_dev" in entries and "cvs_lut3d_f16_dev" in entries and "cvs_half_lookup_dev" not in entries
    assert len(header_files()) >= 11 and {"cvs_reconstruct_420_dev", "cvs_temporal_denoise_f16_dev", "cvs_qualify_f32_dev"} <= entries
    for extent in ((2, 65536), (70001, 3)):
        rec = Recorder()
        for gid, _pin, build, extents, _halo in xc.GROUPS:
            for at in AT_EXTENT[extent]:
                if at not in extents:
                    continue
                for what, case in build(rec, *at):
                    assert case(HostOnly(rec, 1)) == 0
        reached = {n for n, _ in rec.calls if n.startswith("cvs_") and n.endswith("_dev")}
        assert reached <= entries, sorted(reached - entries)
        assert not reached & set(xc.EXEMPT)
        missing = entries - reached - set(xc.EXEMPT)
        assert not missing, "at %d x %d no extent case calls %r" % (extent[0], extent[1], sorted(missing))
    assert sorted(xc.EXEMPT) == ["cvs_reconstruct_dv_dev", "cvs_subsample_dv_dev"]
    assert "video_get_frame_dev" in {n for n, _ in rec.calls}            # the workspace stack, through the device slot
