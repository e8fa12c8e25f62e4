"""The graph evaluator and generator of tests/graph_model.py, checked without the library: the request windows written into the
evaluator are sufficient (a pull in tiles equals the crop of the whole pull, which fails when any one of them shrinks by a
pixel), the committed seed reaches what tests/test_node_graphs_gpu.py is there for, no graph of it comes out empty or tiny, and
the one pairing the suite has by hand, matte(key(tape)), gives that test's model expression."""
import collections

import numpy as np
import pytest

import oracle
from tests import graph_model as gm
from tests import key_model as km
from tests import matte_model as mm
from tests.models import f2h_rz_model
from tests.test_fields_gpu import Tape as HandTape
from tests.test_matte_gpu import KEY, TAPS5
from tests.test_unsharp_gpu import _tiles
from tests.util import canon_f16, canon_f32


@pytest.fixture(scope="module")
def graphs():
    return gm.graphs()


def _bits(pixels):
    return canon_f16(pixels) if pixels.dtype == np.uint16 else canon_f32(pixels)


def _describe(node):
    return gm.kind(node) + ("(" + ", ".join(_describe(s) for s in node.sources) + ")" if node.sources else "")


def _area(win):
    return 0 if win is None else (win[2] - win[0] + 1) * (win[3] - win[1] + 1)


def test_the_tiles_are_the_suites():
    for full in [(-3, -5, 50, 31), gm.WIDE, (0, 0, 1, 1), (7, -9, 30, 2)]:
        assert gm.tiles(full) == _tiles(full)


@pytest.mark.parametrize("flavour", ["gcc", "fma"])
def test_tiles_equal_the_whole_in_the_model(graphs, flavour):
    """Every graph of the seed, both frames, both formats: the pull over each tile is the crop of the pull over the whole
    window, pixels (zero outside the window) and window.  A node that asked its source for a pixel less than its taps reach
    would differ along the tiles' inner edges."""
    with oracle.flavour(flavour):
        for n, (graph, raster) in enumerate(graphs):
            for full in gm.windows(raster):
                for index in gm.FRAMES:
                    for fmt in (gm.F16, gm.F32):
                        whole, win = gm.pull(graph, index, full, fmt)
                        for tile in _tiles(full):
                            what = "graph %d %s frame %d %s window %r tile %r" % (n, _describe(graph), index, fmt, full, tile)
                            got, twin = gm.pull(graph, index, tile, fmt)
                            assert twin == (None if win is None else gm.um.intersect(win, tile)), what
                            assert np.array_equal(_bits(got), _bits(gm.um.crop(whole, full, tile))), what


def test_the_fixed_chains_are_usable_and_tile_in_the_model():
    full = (-3, -5, 50, 31)
    for name, graph in gm.fixed_chains().items():
        assert gm.usable(graph, gm.RASTER), name
        for fmt in (gm.F16, gm.F32):
            whole, win = gm.pull(graph, 2, full, fmt)
            for tile in _tiles(full):
                got, twin = gm.pull(graph, 2, tile, fmt)
                assert twin == gm.um.intersect(win, tile), (name, tile)
                assert np.array_equal(_bits(got), _bits(gm.um.crop(whole, full, tile))), (name, fmt, tile)
    # what the named cases are there for
    gm.TRACE = []
    try:
        gm.pull(gm.fixed_chains()["matte(transform(tape), choke=-2, feather=gauss9)"], 2, full, gm.F32)
        asked, win = next((asked, win) for node, asked, win in gm.TRACE if isinstance(node, gm.Transform))
    finally:
        gm.TRACE = None
    assert asked == (-9, -11, 56, 37) and all(a < w for a, w in zip(asked[:2], win[:2])) and all(a > w for a, w in zip(asked[2:], win[2:]))


def _statistics(graphs):
    """What the seed covers: per node kind the graphs it occurs in, the adjacent pairs, and per graph whether a half-native
    node sits in mid-chain, whether some node answered with less than it was asked for, and the smallest window pulled."""
    kinds, variants, pairs = collections.Counter(), collections.Counter(), set()
    mid_half, partial, empty, smallest = 0, 0, 0, None
    for graph, raster in graphs:
        nodes = list(gm.walk(graph))
        for k in set(gm.kind(node) for node in nodes):
            kinds[k] += 1
        seen = set()
        for node in nodes:
            for s in node.sources:
                pairs.add((gm.kind(node), gm.kind(s)))
            if any(isinstance(v, gm.Lerp) for v in vars(node).values()):
                seen.add("lerp")
            if isinstance(node, gm.Tape) and node.raster != gm.RASTER:
                seen.add("tape on another raster")
            if isinstance(node, gm.Key):
                seen.add("key, spill" if node.spill else "key, no spill")
                if node.show_matte:
                    seen.add("key, show_matte")
            if isinstance(node, gm.Unsharp):
                seen.add("unsharp, fused taps" if node.taps in gm.FUSED_TAPS else "unsharp, general taps")
            if isinstance(node, gm.Matte):
                if node.choke != 0:
                    seen.add("matte, positive choke" if node.choke > 0 else "matte, negative choke")
                seen.add("matte, feather" if node.feather else "matte, no feather")
            if isinstance(node, gm.Transform):
                seen.add("transform, " + node.filter_name)
                if node.source_rect != raster:
                    seen.add("transform, source_rect inside the raster")
            if isinstance(node, gm.Workspace):
                seen.add("workspace, %d items" % len(node.items))
        for v in seen:
            variants[v] += 1
        # mid-chain: a half-native node that has a source of its own and a node above it
        mid_half += any(s.half_native and s.sources for node in nodes for s in node.sources)
        gm.TRACE = []
        try:
            windows = [gm.pull(graph, index, full, gm.F16)[1] for full in gm.windows(raster) for index in gm.FRAMES]
            partial += any(win != asked for _, asked, win in gm.TRACE)
        finally:
            gm.TRACE = None
        empty += any(win is None for win in windows)
        areas = [_area(win) for win in windows if win is not None]
        smallest = min(areas + ([] if smallest is None else [smallest]))
    return dict(kinds=kinds, variants=variants, pairs=pairs, mid_half=mid_half, partial=partial, empty=empty, smallest=smallest)


def test_the_seed_covers_what_the_gpu_test_is_for(graphs):
    s = _statistics(graphs)
    print("graphs per node kind:", sorted(s["kinds"].items()))
    print("graphs per variant:", sorted(s["variants"].items()))
    print("graphs with a half-native node in mid-chain: %d, with a partial window: %d, with an empty pull: %d, smallest window: %d pixels"
          % (s["mid_half"], s["partial"], s["empty"], s["smallest"]))
    assert len(graphs) == gm.COUNT == 48
    for k in gm.KINDS:
        assert s["kinds"][k] >= 4, (k, s["kinds"][k])
    for v in ("lerp", "tape on another raster", "key, spill", "key, no spill", "key, show_matte", "unsharp, fused taps", "unsharp, general taps",
              "matte, positive choke", "matte, negative choke", "matte, feather", "matte, no feather", "transform, bilinear", "transform, nearest",
              "transform, source_rect inside the raster", "workspace, 2 items", "workspace, 3 items"):
        assert s["variants"][v] >= 1, v
    for upper in gm.PAIR_KINDS:
        for lower in gm.SPATIAL:
            assert (upper, lower) in s["pairs"], "%s directly over %s" % (upper, lower)
    assert 3 * s["mid_half"] >= len(graphs), s["mid_half"]
    assert 3 * s["partial"] >= len(graphs), s["partial"]


def test_no_graph_of_the_seed_hides_behind_an_empty_or_tiny_window(graphs):
    """At most one graph in eight may come out empty at a frame the GPU test pulls, and no window pulled has fewer than 64
    pixels: an empty answer would agree with anything."""
    s = _statistics(graphs)
    assert 8 * s["empty"] <= len(graphs), s["empty"]
    assert s["smallest"] >= 64, s["smallest"]


def test_a_mixer_that_reads_outside_a_window_is_refused():
    """A layer whose window starts right of the ground's and above the ground's left edge value (min.y <= the ground's min.x):
    the reference's `left` selector takes the layer for the left strip, pixels nothing defines; the evaluator says so."""
    ground = gm.Solid((0.5, 0.5, 0.5, 1.0), None)
    layer = gm.Solid((0.25, 0.75, 0.5, 0.5), (10, -4, 20, 10))
    with pytest.raises(gm.Undefined):
        gm.pull(gm.Workspace([dict(source=ground), dict(source=layer)]), 0, (-3, -5, 50, 31), gm.F32)
    pixels, win = gm.pull(gm.Workspace([dict(source=ground), dict(source=layer)]), 0, (-6, -5, 50, 31), gm.F32)      # -6 < -4: the ground
    assert win == (-6, -5, 50, 31) and not np.isnan(pixels).any()


def test_matte_over_key_is_the_expression_the_suite_has_by_hand():
    """tests/test_matte_gpu.py test_node_over_the_keyer_equals_the_two_entries_by_hand, its parameters, tape, frame and
    windows: the refine of the model's key over the whole raster, cropped; the f16 pull that truncated (the keyer is not
    half-native, so the matte's f16 pull is its f32 render truncated once)."""
    hand = HandTape()
    tape = gm.Tape(gm.RASTER, pictures=hand.picture)
    p = dict(choke=1, feather=TAPS5, black=0.05, white=0.95)
    assert list(gm.FEATHERS["taps5"]) == TAPS5
    graph = gm.Matte(gm.Key(tape, KEY["key"], KEY["tolerance"], KEY["softness"], KEY["spill"], KEY["spill_range"]), 1, "taps5", 0.05, 0.95)
    codes = hand.picture(4)
    want = mm.refine_pixels(km.key_f32(km.widen(codes), **KEY), **p)
    for full in ((10, 3, 30, 20), (-3, -5, 50, 31), (20, 10, 45, 28)):
        win = km.intersect(full, gm.RASTER)
        got32, w32 = gm.pull(graph, 4, full, gm.F32)
        got16, w16 = gm.pull(graph, 4, full, gm.F16)
        assert w32 == win and w16 == win
        assert np.array_equal(canon_f32(km.crop(got32, full, win)), canon_f32(mm.crop(want, gm.RASTER, win))), full
        assert np.array_equal(canon_f16(km.crop(got16, full, win)), canon_f16(f2h_rz_model(mm.crop(want, gm.RASTER, win)))), full
    # straight over the half-native tape, pulled as f16: the half model on the tape's codes
    direct = gm.Matte(tape, -2, "gauss9", show_matte=True)
    for full in ((10, 3, 30, 20), (-3, -5, 50, 31)):
        win = km.intersect(full, gm.RASTER)
        got16, w16 = gm.pull(direct, 4, full, gm.F16)
        assert w16 == win
        assert np.array_equal(canon_f16(km.crop(got16, full, win)),
                              canon_f16(mm.crop(mm.refine_pixels(codes, -2, gm.FEATHERS["gauss9"], show_matte=True), gm.RASTER, win))), full
