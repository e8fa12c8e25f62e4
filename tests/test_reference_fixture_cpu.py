"""tests/golden/reference_built.npz is what the reference's own code produces today, and its two flavours can be told apart.
CPU only.  The first test needs the reference built (oracle/ref_build.py) and skips elsewhere; the others read the file."""
import os
import sys

import numpy as np
import pytest

import oracle
from tests import reference_cases as rc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))


@pytest.fixture(scope="module")
def fixture():
    return rc.load_fixture()


@pytest.mark.parametrize("flavour", ["gcc", "fma"])
def test_fixture_is_what_the_reference_produces_today(fixture, flavour):
    lib = oracle.ref(flavour)
    if lib is None:
        pytest.skip("the reference's own code is not built here (oracle/ref_build.py)")
    import json
    import make_reference_golden
    now = make_reference_golden.record(rc.ref_abi(lib))
    index, raw = fixture[flavour]
    assert json.loads(str(now.pop("index"))) == index
    assert sorted(k[:-len("/codes")] for k in now) == sorted(raw)
    for k, v in now.items():
        name = k[:-len("/codes")]
        assert v.dtype == raw[name].dtype and np.array_equal(v, raw[name]), name


def test_flavours_differ_in_over_and_bilinear(fixture):
    """Inputs too tame to tell the contracting build from the other would pin nothing about contraction."""
    gcc, fma = fixture["gcc"][0]["cases"], fixture["fma"][0]["cases"]
    assert sorted(gcc) == sorted(fma)
    for family in ("over/", "scale/f32/", "scale/f16/"):
        names = [n for n in gcc if n.startswith(family)]
        assert names and any(gcc[n]["sha"] != fma[n]["sha"] for n in names), family
    # in codes, where both flavours keep them: at least one differs
    for name in ("over/0/0.3", "scale/f32/1.7,0.6"):
        a, b = fixture["gcc"][1][name], fixture["fma"][1][name]
        assert a.shape == b.shape and (a != b).any(), name
    # and what cannot depend on contraction does not: look-ups, integer conversions, copies of table entries
    assert fixture["gcc"][0]["domain"]["h2f"] == fixture["fma"][0]["domain"]["h2f"]
    assert fixture["gcc"][0]["domain"]["f2h"] == fixture["fma"][0]["domain"]["f2h"]


def test_fixture_covers_every_case_and_stays_small(fixture):
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_built.npz")
    assert os.path.getsize(path) < 1000000
    names = set(fixture["gcc"][0]["cases"])
    want = {"%s/%d/%g" % (op, i, m) for op in ("over", "cross") for i in range(13) for m in rc.MIXES}
    want |= {"scale/%s/%g,%g" % ((fmt,) + f) for fmt in ("f32", "f16") for f in rc.SCALE_FACTORS}
    want |= {"scale/wide", "colour/xyz", "colour/srgb", "workspace", "dv/reconstruct", "dv/subsample", "dv/subsample_input_after"}
    want |= {"taps/%s/%g/%g" % (k, s, o) for k in ("tri", "lan") for s, o in rc.TAP_GRID}
    assert names == want
