"""Every device entry recorded into a graph and replayed (include/canvas_hip.h "HIP graphs"; DESIGN.md "Recorded graphs").

The contract of cvs_graph_begin / _end / _launch / _destroy covers every cvs_*_dev entry: frame pointers and parameters are
baked in, frame CONTENTS are read at replay time, scratch blocks and cached tables stay with the graph until it is destroyed.
Here each case of the catalogue (tests/entry_cases.py) is held to it on one explicit stream, never the thread's own:

  the call is made directly on a twin, and on a second twin whose inputs are rolled by one pixel: the expected results;
  it is made once on a third twin (the warm run the contract asks for), whose buffers are then put back as they were;
  it is recorded on that twin's operands: same return code and windows, and NOTHING may have run -- every buffer still holds
      its initial bytes (work that went to another stream, or ran at once, shows here and is missing from every replay);
  the graph is replayed: every output equals the direct call's byte for byte, every input is unwritten;
  the same call is made directly on the same stream in between (the graph's scratch must not be handed out again);
  the rolled inputs are uploaded and the graph is replayed: every output equals the rolled twin's;
  it is launched twice in a row: a replay does not depend on the one before it.

A call that refuses records an empty graph, whose replay must leave every buffer alone.  Then the state behind the contract:
the display tables' and the tap tables' holds, a capture that takes more scratch blocks than a graph can hold, a graph
destroyed from another device context, and a scratch block that another stream parked.

Both arithmetic flavours, set here (tests/conftest.py parametrises two other modules only)."""
import ctypes as C

import numpy as np
import pytest

from canvas_amd import _lib
from canvas_amd.abi import HostFrame, box2i
from canvas_amd.device import DeviceFrame
from tests import entry_cases as ec
from tests.util import assert_same_f16, f32p, same_window

pytestmark = pytest.mark.gpu

GRAPH_BLOCKS = 64             # runtime.c: scratch blocks, and cached tables, one graph can hold
AXIS_CACHE = 128              # fir_tables.c: tap tables cached per context
DISP_CACHE = 8                # display.c: byte tables cached per context


@pytest.fixture(scope="module", params=["separate", "contracted"])
def flavour(request, cvs):
    before = cvs.cvs_set_arithmetic(_lib.ARITH_CONTRACTED if request.param == "contracted" else _lib.ARITH_SEPARATE)
    yield request.param
    cvs.cvs_set_arithmetic(before if before >= 0 else _lib.ARITH_SEPARATE)
    cvs.cvs_fir_path_override(_lib.FIR_PATH_AUTO)


@pytest.fixture(scope="module")
def stream(cvs):
    s = cvs.cvs_stream_create()
    assert s, _lib.last_error()
    yield s
    _lib.check(cvs.cvs_stream_sync(s))
    cvs.cvs_stream_destroy(s)


# ------------------------------------------------------------------ the three factories

class Kept(ec.Twin):
    """The twin, remembering what each object held when it was made."""

    def _initial(self, o, raw):
        return raw

    def _make_frame(self, o, host):
        raw = self._initial(o, np.ascontiguousarray(host.array).reshape(-1, 4).view(np.uint8))         # one row per pixel
        o.initial = raw.reshape(-1).copy()
        ec.Twin._make_frame(self, o, HostFrame(host.full_window, host.dtype, o.initial.view(host.dtype), host.current_window))

    def _make_buffer(self, o, data):
        o.initial = self._initial(o, data.reshape(-1, 1)).reshape(-1).copy()
        ec.Twin._make_buffer(self, o, o.initial)

    def put(self, contents, only=lambda o: True):
        """contents[k] into object k, at once (nothing may be running on the objects)."""
        for o, raw in zip(self.objects, contents):
            if o.nbytes and only(o):
                _lib.check(self.cvs.cvs_memcpy_h2d(o.ptr, raw.ctypes.data, o.nbytes, None), "h2d")


class Rolled(Kept):
    """Everything the call reads holds other contents: pixels rolled by one position (through the whole buffer, so along x),
    planes and flat arrays by one byte."""

    def _initial(self, o, raw):
        return np.roll(raw, 1, axis=0) if o.reads else raw


class Replay(ec.Factory):
    """Hands out the operands of an earlier twin again, in order, each frame's window put back to what the case starts from.
    Nothing happens on the device."""

    def __init__(self, twin):
        ec.Factory.__init__(self, twin.cvs, twin.stream)
        self.twin = twin

    def _earlier(self, o):
        t = self.twin.objects[len(self.objects) - 1]
        assert (t.cls, t.nbytes, t.out, t.name) == (o.cls, o.nbytes, o.out, o.name), "the case is not the same case"
        return t

    def _make_frame(self, o, host):
        t = self._earlier(o)
        t.frame.c.current_window = box2i.of(*host.current_window.tuple())
        o.frame, o.ptr = t.frame, t.ptr

    def _make_buffer(self, o, data):
        o.ptr = self._earlier(o).ptr


def _windows(fac):
    return [None if o.frame is None else box2i.of(*o.frame.current_window.tuple()) for o in fac.objects]


def _same(label, objects, got, want, which="outputs"):
    for o, g, w in zip(objects, got, want):
        if (which == "outputs") != bool(o.out) and which != "all":
            continue
        if not np.array_equal(g, w):
            bad = np.flatnonzero(g != w)
            raise AssertionError("%s: %s (%s) differs in %d of %d bytes, first at byte %d: 0x%02x, expected 0x%02x" % (
                label, o.name, "output" if o.out else "input", bad.size, g.size, bad[0], g[bad[0]], w[bad[0]]))


def record(cvs, stream, call):
    """call() between cvs_graph_begin and cvs_graph_end on `stream`; -> (what call returned, the graph, or None)."""
    _lib.check(cvs.cvs_graph_begin(stream), "cvs_graph_begin")
    try:
        result = call()
    finally:
        graph = cvs.cvs_graph_end(stream)
    return result, graph


def run_case(cvs, stream, what, case):
    twins = []

    def twin(cls):
        twins.append(cls(cvs, stream))
        return twins[-1]
    graph = None
    try:
        # 1. what the call gives, on the catalogue's contents and on rolled ones
        a = twin(Kept)
        want_rc, want, want_windows = case(a), a.collect(), _windows(a)
        r = twin(Rolled)
        rolled_rc, want_rolled = case(r), r.collect()
        assert rolled_rc == want_rc and all(same_window(x, y) for x, y in zip(_windows(r), want_windows) if x is not None), what + ": the rolled twin is another call"
        # 2. the warm run, then every buffer as it was
        g = twin(Kept)
        assert case(g) == want_rc
        _lib.check(cvs.cvs_stream_sync(stream))
        initial = [o.initial for o in g.objects]
        g.put(initial)
        # 3. recorded: the same answer, and nothing has run
        rc, graph = record(cvs, stream, lambda: case(Replay(g)))
        assert graph, "%s: cvs_graph_end gave no graph: %s" % (what, _lib.last_error())
        assert rc == want_rc, "%s: returned %r while recording, %r when called directly (%s)" % (what, rc, want_rc, _lib.last_error())
        for o, w, ww in zip(g.objects, _windows(g), want_windows):
            assert w is None or same_window(w, ww), "%s: %s reports window %r while recording, %r when called directly" % (what, o.name, w.tuple(), ww.tuple())
        _same(what + ", after recording (nothing may have run)", g.objects, g.collect(), initial, "all")
        # 4. replayed on the contents it was recorded over
        _lib.check(cvs.cvs_graph_launch(graph, stream), "cvs_graph_launch")
        got = g.collect()
        _same(what + ", first replay", g.objects, got, want)
        _same(what + ", first replay", g.objects, got, initial, "inputs")
        # 5. the stream used directly in between: the graph's scratch is not handed out again
        d = twin(Kept)
        assert case(d) == want_rc
        _same(what + ", called directly between two replays", d.objects, d.collect(), want)
        # 6. replayed on new contents
        g.put([o.initial for o in r.objects])
        _lib.check(cvs.cvs_graph_launch(graph, stream), "cvs_graph_launch")
        _same(what + ", replay on rolled inputs", g.objects, g.collect(), want_rolled, "all")
        # 7. twice in a row: a replay does not depend on the one before it (what is worked on in place is put back in between)
        in_place = lambda o: o.out and o.reads
        for _ in range(2):
            if any(in_place(o) for o in g.objects):
                _lib.check(cvs.cvs_stream_sync(stream))
                g.put([o.initial for o in r.objects], in_place)
            _lib.check(cvs.cvs_graph_launch(graph, stream), "cvs_graph_launch")
        _same(what + ", two replays in a row", g.objects, g.collect(), want_rolled, "all")
    finally:
        cvs.cvs_stream_sync(stream)
        if graph:
            cvs.cvs_graph_destroy(graph)
        for t in twins:
            t.free()


@pytest.mark.parametrize("group", ec.GROUPS, ids=[g[0] for g in ec.GROUPS])
def test_recorded_and_replayed(cvs, flavour, stream, group):
    _gid, pin, build = group
    cvs.cvs_fir_path_override(pin)
    try:
        for what, case in build(cvs):
            run_case(cvs, stream, what, case)
    finally:
        cvs.cvs_fir_path_override(_lib.FIR_PATH_AUTO)


# ------------------------------------------------------------------ the state behind the contract

def _free_bytes(cvs):
    f, t = C.c_size_t(), C.c_size_t()
    _lib.check(cvs.cvs_mem_info(C.byref(f), C.byref(t)))
    return f.value


def _intent_bytes(cvs, frame, out, intent, stream):
    """cvs_frame_to_rgba8_intent_dev of the 64 x 64 frame into `out`: (return code, the bytes `out` holds afterwards)."""
    rc = cvs.cvs_frame_to_rgba8_intent_dev(out, frame.ref(), _lib.LUT_NONE, C.c_float(intent), stream)
    _lib.check(cvs.cvs_stream_sync(stream))
    got = np.empty((64, 64), np.uint32)
    _lib.check(cvs.cvs_memcpy_d2h(got.ctypes.data, out, got.nbytes, None))
    return rc, got


def _oracle_intent(orc, host, intent):
    want = np.zeros((64, 64), np.uint32)
    orc.lib().orc_frame_to_rgba8_intent(want.ctypes.data_as(C.POINTER(C.c_uint32)), host.ref(), None, C.c_float(intent))
    return want


def test_a_graph_holds_its_display_table(cvs, orc, flavour, stream):
    """display.c keeps 8 byte tables and REWRITES an evicted slot in place: a graph whose table were not held would replay with
    another intent's bytes.  And with every slot held by a graph there is no slot for a ninth table: the call says so and
    writes nothing."""
    host = ec.all_codes((0, 0, 63, 63), (0, 0, 63, 63))
    frame = DeviceFrame.from_host(host)
    out = cvs.cvs_malloc(64 * 64 * 4)
    pad = np.full((64, 64), 0xA5A5A5A5, np.uint32)
    graphs = []
    try:
        rc, before = _intent_bytes(cvs, frame, out, 2.0, stream)                       # warm; the direct result before the churn
        assert rc == 0 and np.array_equal(before, _oracle_intent(orc, host, 2.0))
        rc, graph = record(cvs, stream, lambda: cvs.cvs_frame_to_rgba8_intent_dev(out, frame.ref(), _lib.LUT_NONE, C.c_float(2.0), stream))
        assert graph and rc == 0, _lib.last_error()
        graphs.append(graph)
        for k in range(12):                                                            # tests/test_gpu_parity.py test_display_table_cache_evicts_and_rebuilds
            rc, got = _intent_bytes(cvs, frame, out, 0.5 + 0.1 * k, stream)
            assert rc == 0 and np.array_equal(got, _oracle_intent(orc, host, 0.5 + 0.1 * k)), k
        _lib.check(cvs.cvs_memcpy_h2d(out, pad.ctypes.data, pad.nbytes, None))
        _lib.check(cvs.cvs_graph_launch(graph, stream))
        _lib.check(cvs.cvs_stream_sync(stream))
        got = np.empty((64, 64), np.uint32)
        _lib.check(cvs.cvs_memcpy_d2h(got.ctypes.data, out, got.nbytes, None))
        assert np.array_equal(got, before), "the replay read another table: %d of %d pixels differ" % ((got != before).sum(), got.size)
        # eight graphs, eight intents: every slot is held
        for k in range(1, DISP_CACHE):
            intent = 2.0 + 0.25 * k
            assert _intent_bytes(cvs, frame, out, intent, stream)[0] == 0
            rc, graph = record(cvs, stream, lambda: cvs.cvs_frame_to_rgba8_intent_dev(out, frame.ref(), _lib.LUT_NONE, C.c_float(intent), stream))
            assert graph and rc == 0, _lib.last_error()
            graphs.append(graph)
        _lib.check(cvs.cvs_memcpy_h2d(out, pad.ctypes.data, pad.nbytes, None))
        cvs.cvs_clear_last_error()
        rc, got = _intent_bytes(cvs, frame, out, 0.33, stream)
        assert rc != 0 and "every cache slot belongs to a captured graph" in _lib.last_error(), (rc, _lib.last_error())
        assert np.array_equal(got, pad), "the refused call wrote its target"
        cvs.cvs_graph_destroy(graphs.pop())
        rc, got = _intent_bytes(cvs, frame, out, 0.33, stream)
        assert rc == 0 and np.array_equal(got, _oracle_intent(orc, host, 0.33)), _lib.last_error()
    finally:
        cvs.cvs_stream_sync(stream)
        for graph in graphs:
            cvs.cvs_graph_destroy(graph)
        cvs.cvs_free(out)
        frame.free()


def test_graphs_hold_their_tap_tables_until_destroyed(cvs, orc, flavour, stream):
    """The pins of fir_tables.c, through exhaustion only (an evicted tap table is freed, not rewritten: churning the cache under a
    graph is not something to try on a device).  Pinned to the table kernels a Lanczos call reads two cached tables; 32 calls
    at factors of their own are the 64 holds one graph takes, two such graphs hold all 128 slots of the cache.  Every graph
    replays to the direct results; a call at a new factor then finds no slot, says so and writes nothing; after one graph is
    destroyed it goes through."""
    sfull = (0, 0, 31, 17)
    src_host = ec.px16(np.random.default_rng(2100), sfull)
    src = DeviceFrame.from_host(src_host)
    per_graph = GRAPH_BLOCKS // 2
    ngraphs = AXIS_CACHE // GRAPH_BLOCKS
    factors = [(0.40 + 0.011 * k, 0.45 + 0.013 * k) for k in range(per_graph * ngraphs + 1)]      # all different, on both axes
    sizes = [(max(1, int(32 * fx)), max(1, int(18 * fy))) for fx, fy in factors]
    outs = [DeviceFrame((0, 0, w - 1, h - 1), np.uint16) for w, h in sizes]
    blanks = [ec.blank(True, (0, 0, w - 1, h - 1)).array for w, h in sizes]

    def lanczos(k):
        return cvs.cvs_resample_lanczos_f16_dev(outs[k].ref(), src.ref(), C.c_float(factors[k][0]), C.c_float(factors[k][1]), 3, stream)
    graphs = []
    cvs.cvs_fir_path_override(_lib.FIR_PATH_TABLES | _lib.FIR_PATH_HV)
    try:
        direct = []
        for k in range(per_graph * ngraphs):                                             # warm, and the direct results
            _lib.check(lanczos(k), "lanczos %d" % k)
            _lib.check(cvs.cvs_stream_sync(stream))
            direct.append(outs[k].download().array)
            outs[k].upload(blanks[k])
        _assert_oracle_lanczos(orc, src_host, direct[0], sizes[0], factors[0])
        for gi in range(ngraphs):
            ks = range(gi * per_graph, (gi + 1) * per_graph)
            rcs, graph = record(cvs, stream, lambda: [lanczos(k) for k in ks])
            assert graph, "graph %d: %s" % (gi, _lib.last_error())
            graphs.append(graph)
            assert rcs == [0] * per_graph
        for gi, graph in enumerate(graphs):
            _lib.check(cvs.cvs_graph_launch(graph, stream))
            _lib.check(cvs.cvs_stream_sync(stream))
            for k in range(gi * per_graph, (gi + 1) * per_graph):
                assert np.array_equal(outs[k].download().array, direct[k]), "graph %d, call %d" % (gi, k)
        # every slot is held: no room for the two tables of a new factor
        last = per_graph * ngraphs
        outs[last].upload(blanks[last])
        cvs.cvs_clear_last_error()
        rc = lanczos(last)
        _lib.check(cvs.cvs_stream_sync(stream))
        assert rc != 0 and "every cache slot is held" in _lib.last_error(), (rc, _lib.last_error())
        assert np.array_equal(outs[last].download().array, blanks[last]), "the refused call wrote its target"
        cvs.cvs_graph_destroy(graphs.pop())
        _lib.check(lanczos(last), "lanczos at a new factor, one graph destroyed")
        _lib.check(cvs.cvs_stream_sync(stream))
        _assert_oracle_lanczos(orc, src_host, outs[last].download().array, sizes[last], factors[last])
    finally:
        cvs.cvs_fir_path_override(_lib.FIR_PATH_AUTO)
        cvs.cvs_stream_sync(stream)
        for graph in graphs:
            cvs.cvs_graph_destroy(graph)
        for f in outs + [src]:
            f.free()


def _assert_oracle_lanczos(orc, src16, got, tsize, factors):
    """`got`, a whole target buffer, holds the oracle's pixels inside the window the oracle reports."""
    src32 = HostFrame(src16.full_window, np.float32, orc.half_to_float(src16.array), src16.current_window)
    small = HostFrame((0, 0, tsize[0] - 1, tsize[1] - 1), np.float32)
    orc.lib().orc_resample_lanczos_f32(small.ref(), src32.ref(), C.c_float(factors[0]), C.c_float(factors[1]), 3)
    x0, y0, x1, y1 = small.current_window.tuple()
    assert x1 >= x0 and y1 >= y0
    assert_same_f16(got[y0:y1 + 1, x0:x1 + 1], orc.float_to_half(small.array)[y0:y1 + 1, x0:x1 + 1], "lanczos x%r against the oracle" % (factors,))


BIG = 1024                                  # a 1024 x 1024 f32 scratch frame: 16 MiB
BIG_BLOCK = BIG * BIG * 16


def _big_unsharp(cvs):
    """cvs_unsharp_mask_f16_dev with 15 taps (no one-launch form: the blur goes into ONE pooled f32 frame of the window's size)
    on a 1024 x 1024 frame: (call(stream) -> return code, the target frame, every frame to free)."""
    full = (0, 0, BIG - 1, BIG - 1)
    tile = ec.px16(np.random.default_rng(2200), (0, 0, 127, 127)).array
    src = DeviceFrame.from_host(HostFrame(full, np.uint16, np.tile(tile, (BIG // 128, BIG // 128, 1))))
    out = DeviceFrame(full, np.uint16)
    taps = ec._taps(15)

    def call(stream):
        return cvs.cvs_unsharp_mask_f16_dev(out.ref(), src.ref(), f32p(taps), 15, C.c_float(0.7), C.c_float(0.01), stream)
    return call, out, [src, out]


def test_a_capture_with_too_many_scratch_blocks_gives_them_all_back(cvs, flavour, stream):
    """A graph holds at most GRAPH_BLOCKS scratch blocks.  A capture that takes 8 more fails -- and must lose none of them: the
    thread can record again at once, the entry works as before, and after a trim the device has its memory back to within one
    block (a condition, not a measurement: the eight blocks past the 64th are eight times that)."""
    call, out, frames = _big_unsharp(cvs)
    count = GRAPH_BLOCKS + 8
    try:
        _lib.check(call(stream))                                                       # warm
        _lib.check(cvs.cvs_stream_sync(stream))
        want = out.download().array
        cvs.cvs_pool_trim()
        before = _free_bytes(cvs)
        # one parked block per recorded call, so that the capture allocates nothing
        blocks = [cvs.cvs_pool_malloc(BIG_BLOCK, stream) for _ in range(count)]
        assert all(blocks), _lib.last_error()
        for b in blocks:
            cvs.cvs_pool_free(b, stream)
        _lib.check(cvs.cvs_stream_sync(stream))
        assert before - _free_bytes(cvs) >= count * BIG_BLOCK
        cvs.cvs_clear_last_error()
        rcs, graph = record(cvs, stream, lambda: [call(stream) for _ in range(count)])
        if graph:
            cvs.cvs_graph_destroy(graph)
        assert rcs == [0] * count
        assert not graph and "scratch blocks" in _lib.last_error(), _lib.last_error()
        rc, graph = record(cvs, stream, lambda: 0)                                     # the thread is not left capturing
        assert graph, _lib.last_error()
        cvs.cvs_graph_destroy(graph)
        out.upload(np.zeros_like(want))
        _lib.check(call(stream))
        _lib.check(cvs.cvs_stream_sync(stream))
        assert np.array_equal(out.download().array, want)
        cvs.cvs_pool_trim()
        after = _free_bytes(cvs)
        assert before - after <= BIG_BLOCK, "%d bytes (%.1f blocks of %d) did not come back" % (before - after, (before - after) / BIG_BLOCK, BIG_BLOCK)
    finally:
        cvs.cvs_stream_sync(stream)
        for f in frames:
            f.free()
        cvs.cvs_pool_trim()


def test_a_graph_destroyed_from_another_context_parks_its_blocks_where_they_came_from(cvs, flavour):
    """A graph recorded in a second context on device 0 and destroyed by a thread bound to the home context: its scratch block
    belongs to the RECORDING context's pool.  So the destroy frees nothing (the block is parked there), and a trim in the
    recording context gives at least the block back.  Launching from the home context runs the graph in its own, too."""
    home = cvs.cvs_current_context()
    other = cvs.cvs_context_open(0)
    assert other >= 0 and other != home, _lib.last_error()
    frames, graph, s = [], None, None
    try:
        assert cvs.cvs_set_context(other) == home
        s = cvs.cvs_stream_create()
        call, out, frames = _big_unsharp(cvs)
        _lib.check(call(s))                                                            # warm
        _lib.check(cvs.cvs_stream_sync(s))
        want = out.download().array
        rc, graph = record(cvs, s, lambda: call(s))
        assert graph and rc == 0, _lib.last_error()
        out.upload(np.zeros_like(want))
        _lib.check(cvs.cvs_graph_launch(graph, s))
        _lib.check(cvs.cvs_stream_sync(s))
        assert np.array_equal(out.download().array, want)
        cvs.cvs_pool_trim()                                                            # nothing of this context is parked now
        assert cvs.cvs_set_context(home) == other
        out.upload(np.zeros_like(want))                                                # (device 0 either way)
        _lib.check(cvs.cvs_graph_launch(graph, s))
        assert cvs.cvs_current_context() == home
        held = _free_bytes(cvs)                                                        # (waits for nothing: the destroy does)
        cvs.cvs_graph_destroy(graph)
        graph = None
        assert cvs.cvs_current_context() == home
        destroyed = _free_bytes(cvs)
        assert np.array_equal(out.download().array, want), "the graph launched from the home context"
        # (the runtime's own memory for the instantiated graph does come back at the destroy: 2 MiB seen; the block is 16)
        assert destroyed < held + BIG_BLOCK // 2, "cvs_graph_destroy gave %d bytes back to the driver: the block was not parked" % (destroyed - held)
        cvs.cvs_pool_trim()                                                            # the home context's pool: not there
        assert _free_bytes(cvs) < held + BIG_BLOCK // 2
        assert cvs.cvs_set_context(other) == home
        cvs.cvs_pool_trim()
        assert _free_bytes(cvs) >= destroyed + BIG_BLOCK, "the block is not in the recording context's pool"
    finally:
        cvs.cvs_set_context(other)
        if graph:
            cvs.cvs_graph_destroy(graph)
        for f in frames:
            f.free()
        if s:
            cvs.cvs_stream_destroy(s)
        cvs.cvs_pool_trim()
        cvs.cvs_set_context(-1)
    assert cvs.cvs_current_context() == home


def test_a_capture_takes_a_block_that_another_stream_parked(cvs, flavour, stream):
    """Warmed on one stream, recorded on another: the pool hands the capture a block whose event belongs to the first stream,
    which a capturing stream cannot wait for on the device -- the host waits instead (cvs_pool_malloc)."""
    call, out, frames = _big_unsharp(cvs)
    first = cvs.cvs_stream_create()
    graph = None
    try:
        cvs.cvs_pool_trim()
        _lib.check(call(first))                                                        # the only parked block of this size is `first`'s
        _lib.check(cvs.cvs_stream_sync(first))
        want = out.download().array
        out.upload(np.zeros_like(want))
        before = _free_bytes(cvs)
        rc, graph = record(cvs, stream, lambda: call(stream))
        assert graph and rc == 0, _lib.last_error()
        assert before - _free_bytes(cvs) < BIG_BLOCK, "the capture allocated a block of its own"
        _lib.check(cvs.cvs_stream_sync(stream))
        assert not out.download().array.any(), "recording ran the call"
        _lib.check(cvs.cvs_graph_launch(graph, stream))
        _lib.check(cvs.cvs_stream_sync(stream))
        assert np.array_equal(out.download().array, want)
    finally:
        cvs.cvs_stream_sync(stream)
        if graph:
            cvs.cvs_graph_destroy(graph)
        cvs.cvs_stream_destroy(first)
        for f in frames:
            f.free()
        cvs.cvs_pool_trim()
