"""One ledger over every header, without a GPU: every device entry any include/canvas*.h declares is run by each of the five
harnesses, or is exempt from it for a reason that is a property of the entry.

  placement       frames packed into a guarded arena at every residue (tests/test_placement_gpu.py)
  replay          recorded into a graph and replayed (tests/test_graph_replay_gpu.py)
  far windows     windows far from the origin (tests/test_far_windows_gpu.py)
  extents         windows taller or wider than a picture (tests/test_extents_gpu.py)
  shared buffers  operands that share a buffer (tests/test_aliasing_gpu.py)

The first three run the catalogue of tests/entry_cases.py and, through a module tests/test_<family>_harness_gpu.py each, the
catalogue of every tests/<family>_cases.py, found by glob; the fourth runs tests/extent_cases.py, the fifth tests/alias_cases.py.
What a catalogue CALLS is established as tests/test_entry_cases_cpu.py establishes it: its cases are run on operands that exist as
descriptions only, against a stand-in that notes the calls.  Tests that are functions of a harness module and in no catalogue are
listed in IN_HARNESS; the ledger holds each to its module, which must import without a GPU.

The headers are found, not listed: a header added tomorrow is in the ledger at once, and so are its entries, missing under
every heading until something runs them."""
import glob
import importlib
import os

from tests import alias_cases as ac
from tests import entry_cases as ec
from tests import extent_cases as xc
from tests.test_entry_cases_cpu import NOT_RECORDED, HostOnly, Recorder, device_entries, header_files

HEADINGS = ("placement", "replay", "far windows", "extents", "shared buffers")
HERE = os.path.dirname(os.path.abspath(__file__))
# heading -> the test of a family's harness module that runs the family's catalogue (a name, or the start of one)
HARNESS_TESTS = {"placement": "test_packed_into_a_guarded_arena", "replay": "test_recorded_and_replayed", "far windows": "test_far_"}

_FLAT = "a flat array of `count` elements: it has no window to make tall or wide"
_CODED = "its other operand is coded planes of bytes, no frame: no two operands of one type"
# heading -> entry -> the property of the ENTRY that keeps it out of that harness (at least four words)
EXEMPT = {
    "placement": {}, "replay": dict(NOT_RECORDED), "far windows": {},
    "extents": dict(xc.EXEMPT, cvs_half_lookup_dev=_FLAT, cvs_half_to_float_dev=_FLAT, cvs_half_to_float_fast_dev=_FLAT, cvs_float_to_half_dev=_FLAT,
                    cvs_float_to_half_fast_dev=_FLAT),
    # (tests/alias_cases.py's own exemptions are that catalogue's, held to the prototypes by tests/test_alias_cases_cpu.py)
    "shared buffers": dict({e: (r if len(r.split()) >= 4 else r + ": nothing to share a buffer with") for e, r in ac.EXEMPT.items()},
                           cvs_reconstruct_422_dev=_CODED, cvs_subsample_422_dev=_CODED, cvs_reconstruct_420_dev=_CODED, cvs_subsample_420_dev=_CODED),
}
# (heading, entry) -> (module, function): tests written by hand inside a harness or GPU module, which no catalogue knows
_MEDIAN, _PRIMARY, _SECONDARY = "tests.test_median_harness_gpu", "tests.test_primary_harness_gpu", "tests.test_secondary_harness_gpu"
TALLEST, WIDEST = "test_a_window_of_4194305_rows", "test_a_window_of_131073_columns"
IN_HARNESS = {
    # 4 194 305 rows, and beside it in the same module 131 073 columns (WIDEST), of the f16 entries; the catalogue of
    # tests/extent_cases.py reaches these entries, the f32 ones too, at 65 536 rows and 70 001 columns
    ("extents", "cvs_median_f16_dev"): (_MEDIAN, TALLEST), ("extents", "cvs_primary_f16_dev"): (_PRIMARY, TALLEST),
    ("extents", "cvs_qualify_f16_dev"): (_SECONDARY, TALLEST), ("extents", "cvs_matte_mix_f16_dev"): (_SECONDARY, TALLEST),
}
IN_HARNESS.update({
    ("shared buffers", "cvs_median_f16_dev"): (_MEDIAN, "test_the_target_as_the_source_is_refused_and_leaves_no_trace"),
    ("shared buffers", "cvs_median_f32_dev"): (_MEDIAN, "test_the_target_as_the_source_is_refused_and_leaves_no_trace"),
    ("shared buffers", "cvs_temporal_denoise_f16_dev"): ("tests.test_temporal_harness_gpu", "test_the_output_as_a_present_input_is_refused_and_leaves_no_trace"),
    # the in-place cases of tests/primary_cases.py and tests/secondary_cases.py against the same call out of place
    ("shared buffers", "cvs_primary_f16_dev"): ("tests.test_primary_gpu", "test_widths_rows_and_placements"),
    ("shared buffers", "cvs_primary_f32_dev"): ("tests.test_primary_gpu", "test_widths_rows_and_placements"),
    ("shared buffers", "cvs_qualify_f16_dev"): ("tests.test_secondary_gpu", "test_in_place_equals_out_of_place_on_every_permitted_pair"),
    ("shared buffers", "cvs_qualify_f32_dev"): ("tests.test_secondary_gpu", "test_in_place_equals_out_of_place_on_every_permitted_pair"),
    ("shared buffers", "cvs_matte_mix_f16_dev"): ("tests.test_secondary_gpu", "test_in_place_equals_out_of_place_on_every_permitted_pair"),
    ("shared buffers", "cvs_matte_mix_f32_dev"): ("tests.test_secondary_gpu", "test_in_place_equals_out_of_place_on_every_permitted_pair"),
})


def _called(cases):
    """The device entries the cases call, each run once on a factory that only keeps descriptions"""
    rec = Recorder()
    for case in cases(rec):
        assert case(HostOnly(rec, 1)) == 0
    return {n for n, _ in rec.calls if n.startswith("cvs_") and n.endswith("_dev")}


def family_catalogues():
    """{family: module} of every tests/<family>_cases.py that defines GROUPS, but the three catalogues with harnesses of their own"""
    found = {}
    for path in sorted(glob.glob(os.path.join(HERE, "*_cases.py"))):
        family = os.path.basename(path)[:-len("_cases.py")]
        if family in ("entry", "extent", "alias"):
            continue
        module = importlib.import_module("tests.%s_cases" % family)
        if hasattr(module, "GROUPS"):
            found[family] = module
    return found


_memo = {}


def _once(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def called_by_the_catalogues():
    """{heading: {entry}} for the first three headings: entry_cases.GROUPS, and each family's catalogue where the family's harness
    module has the heading's test"""
    def make():
        base = _called(lambda rec: [case for _gid, _pin, build in ec.GROUPS for _what, case in build(rec)])
        out = {heading: set(base) for heading in HARNESS_TESTS}
        for family, module in family_catalogues().items():
            harness = importlib.import_module("tests.test_%s_harness_gpu" % family)          # (imports without a GPU)
            entries = _called(lambda rec: [case for _gid, build in module.GROUPS for _what, case in build(rec)])
            assert entries == set(module.ENTRIES), family
            for heading, test in HARNESS_TESTS.items():
                if any(name.startswith(test) and callable(getattr(harness, name)) for name in dir(harness)):
                    out[heading] |= entries
        return out
    return _once("catalogues", make)


def called_by_extent_group(gid, build, extents):
    """at the group's first extent"""
    return _once(("extent", gid), lambda: _called(lambda rec: [case for _what, case in build(rec, *extents[0])]))


def called_by_the_alias_catalogue():
    def make():
        rec = Recorder()
        for _gid, build in ac.GROUPS:
            for case in build(rec):
                assert case(HostOnly(rec, 1), "one struct") == 0
        return {n for n, _ in rec.calls if n.startswith("cvs_") and n.endswith("_dev")}
    return _once("alias", make)


def in_harness(heading, entry):
    """The hand-written test of IN_HARNESS for (heading, entry), if its module has it"""
    if (heading, entry) not in IN_HARNESS:
        return False
    module, function = IN_HARNESS[(heading, entry)]
    return callable(getattr(importlib.import_module(module), function, None))


def ledger(texts, extent_groups):
    """{heading: the entries the header texts declare that the heading's harness neither runs nor is exempt from}"""
    entries = set(device_entries(texts))
    run = dict(called_by_the_catalogues())
    run["extents"] = set().union(*[called_by_extent_group(gid, build, extents) for gid, _pin, build, extents, _halo in extent_groups])
    run["shared buffers"] = called_by_the_alias_catalogue()
    missing = {}
    for heading in HEADINGS:
        missing[heading] = sorted(e for e in entries if e not in run[heading] and e not in EXEMPT[heading] and not in_harness(heading, e))
    return missing


def _header_texts():
    return [open(name).read() for name in header_files()]


def test_every_entry_of_every_header_is_run_or_exempt_under_every_heading():
    texts = _header_texts()
    entries = device_entries(texts)
    assert len(header_files()) >= 11 and len(entries) >= 68, (header_files(), sorted(entries))       # 48 of canvas_hip.h and 20 of the ten extension headers
    assert {"cvs_reconstruct_420_dev", "cvs_temporal_denoise_f16_dev", "cvs_matte_mix_f32_dev", "cvs_scope_render_f16_dev"} <= set(entries)
    missing = ledger(texts, xc.GROUPS)
    assert not any(missing.values()), "device entries without a run or a reasoned exemption: %r" % {h: m for h, m in missing.items() if m}


def test_the_exemptions_and_the_table_are_in_order():
    entries = set(device_entries(_header_texts()))
    run = dict(called_by_the_catalogues())
    run["extents"] = set().union(*[called_by_extent_group(g[0], g[2], g[3]) for g in xc.GROUPS])
    run["shared buffers"] = called_by_the_alias_catalogue()
    for heading in HEADINGS:
        stale = sorted(set(EXEMPT[heading]) - entries)
        assert not stale, "%s: exempt, declared by no header: %r" % (heading, stale)
        both = sorted(set(EXEMPT[heading]) & run[heading])
        assert not both, "%s: run by the catalogue and exempt at once: %r" % (heading, both)
        for entry, reason in EXEMPT[heading].items():
            assert isinstance(reason, str) and len(reason.split()) >= 4, "%s / %s: the reason must name a property of the entry" % (heading, entry)
    for (heading, entry), (module, function) in IN_HARNESS.items():
        assert heading in HEADINGS and entry in entries, (heading, entry)
        assert callable(getattr(importlib.import_module(module), function, None)), "%s has no %s" % (module, function)
        if function == TALLEST:
            assert callable(getattr(importlib.import_module(module), WIDEST, None)), "%s has no %s" % (module, WIDEST)
    # every family with a catalogue has the module that runs it through all three harnesses
    for family in family_catalogues():
        harness = importlib.import_module("tests.test_%s_harness_gpu" % family)
        for test in HARNESS_TESTS.values():
            assert any(name.startswith(test) for name in dir(harness)), "tests/test_%s_harness_gpu.py has no %s*" % (family, test)


def test_an_entry_whose_extent_group_is_removed_is_named():
    """Teeth: without its group in the extent catalogue, the deinterlacer has no extent run, and nothing else goes missing."""
    fewer = [g for g in xc.GROUPS if g[0] != "deinterlace_adaptive"]
    assert len(fewer) == len(xc.GROUPS) - 1
    missing = ledger(_header_texts(), fewer)
    assert missing["extents"] == ["cvs_deinterlace_adaptive_f16_dev"]
    assert not any(m for heading, m in missing.items() if heading != "extents")
    # an entry with a hand-written extent test still needs the catalogue at 65 536 rows and 70 001 columns: that is
    # tests/test_extents_cpu.py test_every_frame_taking_entry_is_reached_at_both_extents, which reads the same headers


def test_an_invented_entry_is_missing_under_every_heading():
    """Teeth: a header that declares one more entry, which nothing runs."""
    invented = "CVS_EXPORT int cvs_new_thing_f16_dev(rgba_frame_f16 *target, const rgba_frame_f16 *source, cvs_stream_t s);\n"
    missing = ledger(_header_texts() + ["/* a header of tomorrow */\n" + invented], xc.GROUPS)
    assert missing == {heading: ["cvs_new_thing_f16_dev"] for heading in HEADINGS}
