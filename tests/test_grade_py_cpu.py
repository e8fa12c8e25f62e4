"""fluggo.media.grade without a GPU: the CDL at its nodes against the formula written out, the saturation matrix, lift / gamma /
gain, the monotone cubic through control points, resampling, the 1D `.cube` round trip and its refusals, and that
fluggo.media.cube still refuses a 1D file.  The one test that compares transfer_curves with the library's own half tables needs
the device that builds those tables and is marked gpu."""
import math

import numpy as np
import pytest

from fluggo.media import cube, grade
from tests.models import f2h_rz_model


def test_cdl_at_the_nodes_is_the_formula():
    slope, offset, power = (1.2, 1.0, 0.8), (0.05, 0.0, -0.1), (1.0, 0.9, 2.2)
    for size, domain in ((2, (0.0, 1.0)), (17, (0.0, 1.0)), (1025, (0.0, 1.0)), (33, (-0.5, 1.5)), (9, ((0.0, -1.0, 0.0), (1.0, 1.0, 2.0)))):
        table, matrix = grade.cdl(slope, offset, power, 1.0, size, domain)
        assert len(table) == size and all(len(row) == 3 for row in table)
        lo, hi = grade._domain(domain)
        for i in (0, 1, size // 2, size - 2, size - 1):
            for c in range(3):
                x = lo[c] + i * (hi[c] - lo[c]) / (size - 1) if i < size - 1 else hi[c]
                assert table[i][c] == min(max(x * slope[c] + offset[c], 0.0), 1.0) ** power[c], (size, i, c)
        assert matrix == [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    table, _ = grade.cdl(1.0, 0.0, 1.0, size=5)
    assert table == grade.identity_curves(5) == [[k / 4] * 3 for k in range(5)]
    table, _ = grade.cdl(2.0, -0.5, 1.0, size=5)
    assert [row[0] for row in table] == [0.0, 0.0, 0.5, 1.0, 1.0]                  # clamped before the power
    assert len(grade.cdl(1, 0, 1)[0]) == 1025
    for bad in (dict(slope=-1, offset=0, power=1), dict(slope=1, offset=0, power=0), dict(slope=(1, 1), offset=0, power=1), dict(slope=1, offset=0, power=1, size=1),
                dict(slope=1, offset=0, power=1, size=4098), dict(slope=1, offset=0, power=1, domain=(1.0, 0.0)), dict(slope=1, offset=float("inf"), power=1)):
        with pytest.raises(ValueError):
            grade.cdl(**bad)


def test_saturation_matrix():
    w = grade.REC709_WEIGHTS
    assert grade.saturation_matrix(1.0) == [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    grey = grade.saturation_matrix(0.0)
    assert grey == [w[0], w[1], w[2], 0.0] * 3
    for s in (0.0, 0.5, 1.7):
        m = grade.saturation_matrix(s)
        assert len(m) == 12 and m[3] == m[7] == m[11] == 0.0
        for c in range(3):
            assert math.isclose(sum(m[4 * c:4 * c + 3]), 1.0, abs_tol=1e-15)        # greys stay where they are
        colour = (0.8, 0.3, 0.1)
        luma = sum(w[k] * colour[k] for k in range(3))
        out = [sum(m[4 * c + k] * colour[k] for k in range(3)) for c in range(3)]
        assert all(math.isclose(out[c], luma + s * (colour[c] - luma), abs_tol=1e-15) for c in range(3))
        assert math.isclose(sum(w[k] * out[k] for k in range(3)), luma, abs_tol=1e-15)
    assert grade.saturation_matrix(0.0, (1, 0, 0))[:4] == [1.0, 0.0, 0.0, 0.0]
    assert grade.cdl(1, 0, 1, saturation=0.25)[1] == grade.saturation_matrix(0.25)


def test_lift_gamma_gain():
    assert grade.lift_gamma_gain(0.0, 1.0, 1.0, 5) == grade.identity_curves(5)
    table = grade.lift_gamma_gain((0.1, 0.0, 0.0), (1.0, 2.0, 1.0), (1.0, 1.0, 0.5), 3)
    assert table[0] == [0.1, 0.0, 0.0] and table[2] == [1.0, 1.0, 0.5]
    assert table[1][0] == 0.5 + 0.1 * 0.5 and table[1][1] == 0.5 ** 0.5 and table[1][2] == 0.25
    assert grade.lift_gamma_gain(-0.5, 1.0, 1.0, 3)[0] == [0.0, 0.0, 0.0]           # nothing below black
    with pytest.raises(ValueError):
        grade.lift_gamma_gain(0, 0, 1)


def test_curves_from_points_pass_through_their_points_and_are_monotone():
    rng = np.random.default_rng(5)
    for trial in range(20):
        n = int(rng.integers(2, 8))
        xs = np.sort(rng.choice(np.arange(0, 65), n, replace=False)) / 64.0          # on nodes of a 65-node table
        ys = np.sort(rng.uniform(0, 1, n)) if trial % 2 == 0 else rng.uniform(0, 1, n)
        points = list(zip(xs.tolist(), ys.tolist()))
        table = grade.curves_from_points(points, None, points[::-1], size=65)
        assert len(table) == 65
        for x, y in points:
            i = int(round(x * 64))
            assert math.isclose(table[i][0], y, abs_tol=1e-12) and table[i][1] == i / 64 and math.isclose(table[i][2], y, abs_tol=1e-12)
        column = [row[0] for row in table]
        assert column[0] == ys[0] or xs[0] == 0.0 and math.isclose(column[0], ys[0])   # held flat before the first point
        assert min(column) >= min(ys) - 1e-12 and max(column) <= max(ys) + 1e-12 or trial % 2     # no overshoot for monotone points
        if trial % 2 == 0:
            assert all(b >= a - 1e-15 for a, b in zip(column, column[1:])), (trial, points)
    # two points: the line through them; one: a constant; none: refused; a repeated x: refused
    assert grade.curves_from_points([(0, 0), (1, 1)], [(0, 1), (1, 0)], [(0.5, 0.25)], size=3) == [[0.0, 1.0, 0.25], [0.5, 0.5, 0.25], [1.0, 0.0, 0.25]]
    with pytest.raises(ValueError):
        grade.curves_from_points([], None, None)
    with pytest.raises(ValueError):
        grade.curves_from_points([(0, 0), (0, 1)], None, None)
    # the master goes in front of each channel's curve
    master, red = [(0, 0), (0.5, 0.25), (1, 1)], [(0, 0), (0.25, 0.75), (1, 1)]
    table = grade.curves_from_points(red, None, None, master=master, size=3)
    assert table[1][1] == 0.25 and math.isclose(table[1][0], 0.75) and table[2] == [1.0, 1.0, 1.0]
    # a wider domain: flat beyond the points
    table = grade.curves_from_points([(0, 0.1), (1, 0.9)], None, None, size=5, domain=(-1, 1))
    assert [row[0] for row in table][:3] == [0.1, 0.1, 0.1] and table[4][0] == 0.9 and [row[1] for row in table] == [-1.0, -0.5, 0.0, 0.5, 1.0]


def test_identity_and_resample():
    assert grade.identity_curves(3) == [[0.0] * 3, [0.5] * 3, [1.0] * 3]
    assert grade.identity_curves(2, ((0, -1, 2), (1, 1, 4))) == [[0.0, -1.0, 2.0], [1.0, 1.0, 4.0]]
    big = [[(k / 8192) ** 2 + c for c in range(3)] for k in range(8193)]
    small = grade.resample_curves(big, 4097)
    assert len(small) == 4097 and small[0] == big[0] and small[-1] == big[-1] and small[1] == big[2] and small[2048] == big[4096]
    assert grade.resample_curves(grade.identity_curves(9), 3) == grade.identity_curves(3)
    up = grade.resample_curves([[0, 0, 0], [1, 2, 4]], 5)
    assert up == [[0.0, 0.0, 0.0], [0.25, 0.5, 1.0], [0.5, 1.0, 2.0], [0.75, 1.5, 3.0], [1.0, 2.0, 4.0]]
    for bad in (([[0, 0, 0]], 3), ([[0, 0], [1, 1]], 3), (grade.identity_curves(3), 1), (grade.identity_curves(3), 4098)):
        with pytest.raises(ValueError):
            grade.resample_curves(*bad)


def test_transfer_curves_are_the_functions():
    assert grade.TRANSFERS == ("rec709_to_linear_scene", "rec709_to_linear_display", "linear_to_rec709", "linear_to_srgb")
    for name in grade.TRANSFERS:
        table = grade.transfer_curves(name, 17)
        assert len(table) == 17 and all(row[0] == row[1] == row[2] for row in table)
        assert table[0][0] == 0.0 and math.isclose(table[-1][0], 1.0, abs_tol=1e-12)
        assert all(b[0] > a[0] for a, b in zip(table, table[1:]))
    assert len(grade.transfer_curves("linear_to_rec709")) == 4097
    # the pairs undo each other at the nodes
    there = grade.transfer_curves("linear_to_rec709", 33)
    back = grade._transfer("rec709_to_linear_scene")
    assert all(math.isclose(back(there[i][0]), i / 32, abs_tol=1e-12) for i in range(33))
    assert grade.transfer_curves("linear_to_srgb", 3)[1][0] == 1.055 * 0.5 ** (1 / 2.4) - 0.055
    with pytest.raises(ValueError, match="no such transfer"):
        grade.transfer_curves("log")


NEAR_ULPS = 16          # how close, in f32 steps of the value, a curve's value must lie to a half code for the library's to fall on its other side


def half_code_nodes():
    """(which of the 4097 nodes on [0, 1] are half codes, their codes)"""
    nodes = np.arange(4097, dtype=np.float64) / 4096
    is_code = nodes.astype(np.float16).astype(np.float64) == nodes
    return is_code, nodes[is_code].astype(np.float16).view(np.uint16)


def near_a_half_code(values):
    """Where a value lies within NEAR_ULPS f32 steps of a half code: there, and only there, an f32 evaluation of the same function
    may be truncated to the neighbouring half.  Decided from the Python value alone."""
    v = np.asarray(values, np.float64)
    code = f2h_rz_model(v.astype(np.float32))                            # the half code at or below |v| (towards 0), and the next one
    below, above = code.view(np.float16).astype(np.float64), (code + np.uint16(1)).view(np.float16).astype(np.float64)
    step = np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)
    return np.minimum(np.abs(v - below), np.abs(above - v)) <= NEAR_ULPS * step


def test_the_exemption_of_the_table_comparison_is_narrow():
    """near_a_half_code, on the model alone: it takes a value on a half code and one a few f32 steps beside it, not one a hundred
    steps away; and of the 3073 values per table that the comparison below looks at it exempts at most 90."""
    one = np.float64(np.float16(0.3))
    step = float(np.spacing(np.float32(one)))
    assert near_a_half_code([one, one - 3 * step, one + 3 * step, one + NEAR_ULPS * step]).all()
    assert not near_a_half_code([one + 100 * step, one - 100 * step, 0.3]).any()
    is_code, _ = half_code_nodes()
    assert is_code.sum() == 3073
    for name in grade.TRANSFERS:
        curve = np.array([row[0] for row in grade.transfer_curves(name, 4097)])[is_code]
        # 50, 17, 86 and 9 of the 3073: about 2^-8 of them by chance (2 x 16 steps of 2^-24 in a half step of 2^-11), and the nodes of
        # the linear toes, whose values (x * 4.5 for 73 nodes, x / 4.5, x * 12.92) are or nearly are half codes themselves
        assert near_a_half_code(curve).sum() <= 90, name


@pytest.mark.gpu
def test_transfer_curves_at_half_code_nodes_are_the_librarys_tables(cvs):
    """Wherever a node of the 4097-node table on [0, 1] is a half code (3073 nodes), the curve's value there, brought to a half
    the way the library brings its own tables (rounded to f32, then truncated: tests/models.py f2h_rz_model), EQUALS the entry of
    cvs_lut_host's table for that code -- except where equality is not decidable: the library evaluates the function in f32
    (powf, f32 constants: a few f32 steps from the exact value) and the curve in Python floats, so where the curve's value lies
    within NEAR_ULPS = 16 f32 steps of a half code the two may fall on either side of it and be truncated to neighbouring codes.
    Those nodes are picked from the Python value alone (near_a_half_code); there the codes may differ by one, nowhere else at
    all.  16 steps: the longest chain, ((x + 0.099f) / 1.099f) ^ (1 / 0.45f), has three roundings of half a step and powf's one
    before and after an exponent of 2.2, about 5 steps; 1.099f * powf - 0.099f loses another factor of 2.2 near the knee."""
    from canvas_amd import _lib
    names = {"rec709_to_linear_scene": _lib.LUT_REC709_TO_LINEAR_SCENE, "rec709_to_linear_display": _lib.LUT_REC709_TO_LINEAR_DISPLAY,
             "linear_to_rec709": _lib.LUT_LINEAR_TO_REC709, "linear_to_srgb": _lib.LUT_LINEAR_TO_SRGB}
    is_code, codes = half_code_nodes()
    for name, which in names.items():
        ptr = cvs.cvs_lut_host(which)
        assert ptr, _lib.last_error()
        table = np.ctypeslib.as_array(ptr, shape=(65536,))
        curve = np.array([row[0] for row in grade.transfer_curves(name, 4097)])[is_code]
        mine = f2h_rz_model(curve.astype(np.float32)).astype(np.int64)
        theirs = table[codes].astype(np.int64)
        off = np.abs(mine - theirs)
        near = near_a_half_code(curve)
        print(name, "nodes that are half codes:", int(is_code.sum()), "near a half code:", int(near.sum()), "of those off by one:", int((off[near] == 1).sum()),
              "off elsewhere:", int((off[~near] != 0).sum()))
        assert (off[~near] == 0).all(), (name, codes[~near][off[~near] != 0][:8])
        assert off.max() <= 1, (name, int(off.max()))


def test_cube_1d_round_trip(tmp_path):
    table, _ = grade.cdl((1.1, 1.0, 0.9), (0.01, 0.0, -0.01), (1.0, 1.0, 1.2), size=33)
    text = grade.write_cube_1d(table, (0.0, -0.5, 0.0), (1.0, 1.5, 2.0), title="a grade")
    size, got, lo, hi, title = grade.parse_cube_1d(text)
    assert (size, got, lo, hi, title) == (33, table, (0.0, -0.5, 0.0), (1.0, 1.5, 2.0), "a grade")
    path = tmp_path / "grade.cube"
    path.write_text("# a comment\n\n" + text)
    assert grade.read_cube_1d(str(path)) == (33, table, (0.0, -0.5, 0.0), (1.0, 1.5, 2.0)) == grade.read_cube_1d(path) == grade.read_cube_1d(text)
    assert grade.parse_cube_1d("LUT_1D_SIZE 2\n0 0 0\n1 1 1\n")[1:4] == ([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]], (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    # the constructor arguments of ColorCurves
    from fluggo.media import process
    cv = process.ColorCurves(*grade.read_cube_1d(text))
    assert cv.size == 33 and cv.domain_min == (0.0, -0.5, 0.0) and cv.table == np.array(table, np.float32).tobytes()
    with pytest.raises(ValueError):
        grade.write_cube_1d([[0, 0, 0]])


def test_cube_1d_refusals_name_the_line():
    rows = "".join("%g %g %g\n" % (k, k, k) for k in range(3))
    for text, line, word in (
            ("LUT_1D_SIZE 1\n0 0 0\n", 1, "below 2"),
            ("LUT_1D_SIZE 4098\n", 1, "resample_curves"),
            ("LUT_1D_SIZE 65536\n", 1, "resample_curves"),
            ("LUT_1D_SIZE 3 3\n", 1, "one whole number"),
            ("LUT_1D_SIZE 3\nLUT_1D_SIZE 3\n", 2, "twice"),
            ("LUT_1D_SIZE 3\n" + rows + "3 3 3\n", 5, "more than the 3 rows"),
            ("LUT_1D_SIZE 3\n0 0 0\n1 1 1\n", 3, "2 rows"),
            ("LUT_1D_SIZE 3\n0 0 0\n1 nan 1\n2 2 2\n", 3, "not finite"),
            ("LUT_1D_SIZE 3\n0 0 0\n1 inf 1\n2 2 2\n", 3, "not finite"),
            ("LUT_1D_SIZE 3\n0 0\n", 2, "takes 3 numbers"),
            ("LUT_1D_SIZE 3\n0 0 x\n", 2, "not a number"),
            ("0 0 0\nLUT_1D_SIZE 3\n", 1, "before LUT_1D_SIZE"),
            ("TITLE \"t\"\nLUT_3D_SIZE 2\n", 2, "a 3D table"),
            ("LUT_1D_SIZE 3\nLUT_1D_INPUT_RANGE 0 1\n" + rows, 2, "unknown keyword"),
            ("LUT_1D_SIZE 3\nDOMAIN_MIN 0 0 1\nDOMAIN_MAX 1 1 1\n" + rows, 6, "not below"),
            ("LUT_1D_SIZE 3\nDOMAIN_MIN 0 0\n" + rows, 2, "takes 3 numbers"),
            ("# nothing\n", 0, "no LUT_1D_SIZE")):
        with pytest.raises(cube.CubeError, match=r"line %d: .*%s" % (line, word)):
            grade.parse_cube_1d(text)
    # a larger table is read when asked for, to be brought down
    text = "LUT_1D_SIZE 8193\n" + "".join("%r %r %r\n" % (k / 8192, k / 8192, k / 8192) for k in range(8193))
    size, table = grade.read_cube_1d(text, max_size=None)[:2]
    assert size == 8193 and grade.resample_curves(table, 4097) == grade.identity_curves(4097)


def test_parse_cube_still_refuses_a_1d_file():
    with pytest.raises(cube.CubeError, match="line 1: LUT_1D_SIZE: a 1D table, only 3D tables are read"):
        cube.parse_cube("LUT_1D_SIZE 2\n0 0 0\n1 1 1\n")
    with pytest.raises(cube.CubeError, match="LUT_1D_SIZE"):
        cube.read_cube(grade.write_cube_1d(grade.identity_curves(2)))
