"""Primary grades as values: curve tables and 3 x 4 matrices for `fluggo.media.process.VideoColorCorrectFilter`.

Everything here is plain Python, computed in Python floats.  A curve table is a list of `size` rows `[r, g, b]`, node 0 first: the
rows of a 1D `.cube` file and the `table` argument of `process.ColorCurves`:

    table, matrix = cdl((1.1, 1.0, 0.9), (0.01, 0.0, -0.01), (1.0, 1.0, 1.2), saturation=0.9)
    node = process.VideoColorCorrectFilter(source, pre=process.ColorCurves(len(table), table), matrix=matrix)

A matrix is a list of 12 numbers, three rows of four: out.c = m[4c]*r + m[4c+1]*g + m[4c+2]*b + m[4c+3].  Node i of a table on
the domain (lo, hi) sits on lo + i * (hi - lo) / (size - 1); the filter interpolates linearly between nodes and holds the end
values outside the domain.
"""
import math
import os

from fluggo.media.cube import CubeError, _numbers

MIN_SIZE, MAX_SIZE = 2, 4097
REC709_WEIGHTS = (0.2126, 0.7152, 0.0722)
TRANSFERS = ("rec709_to_linear_scene", "rec709_to_linear_display", "linear_to_rec709", "linear_to_srgb")


def _check_size(size):
    if not isinstance(size, int) or not MIN_SIZE <= size <= MAX_SIZE:
        raise ValueError("size %r, outside %d..%d" % (size, MIN_SIZE, MAX_SIZE))


def _finite(values, what):
    if not all(math.isfinite(v) for v in values):
        raise ValueError("%s must be finite" % what)
    return values


def _three(value, what):
    """a number for all channels, or one per channel -> a tuple of three floats"""
    if isinstance(value, (int, float)):
        return _finite((float(value),) * 3, what)
    out = tuple(float(v) for v in value)
    if len(out) != 3:
        raise ValueError("%s takes a number or three numbers" % what)
    return _finite(out, what)


def _domain(domain):
    """(lo, hi) with numbers or triples -> (lo triple, hi triple)"""
    lo, hi = _three(domain[0], "domain"), _three(domain[1], "domain")
    for c in range(3):
        if not (math.isfinite(lo[c]) and math.isfinite(hi[c]) and lo[c] < hi[c]):
            raise ValueError("domain %g..%g of channel %d must be finite and ascending" % (lo[c], hi[c], c))
    return lo, hi


def _node(lo, hi, i, size):
    return hi if i == size - 1 else lo + i * (hi - lo) / (size - 1)


def curves_from_function(fn, size=1025, domain=(0.0, 1.0)):
    """Samples fn(c, x) -> y, c the channel 0..2, at the nodes of each channel's domain -> the table."""
    _check_size(size)
    lo, hi = _domain(domain)
    table = []
    for i in range(size):
        row = [float(fn(c, _node(lo[c], hi[c], i, size))) for c in range(3)]
        for v in row:
            if not math.isfinite(v):
                raise ValueError("node %d: the function gave a value that is not finite" % i)
        table.append(row)
    return table


def identity_curves(size=2, domain=(0.0, 1.0)):
    """The table that changes nothing inside the domain: every node holds its own position."""
    return curves_from_function(lambda c, x: x, size, domain)


def saturation_matrix(s, weights=REC709_WEIGHTS):
    """out = luma + s * (in - luma), luma = weights . in: 1 changes nothing, 0 gives grey of the same luma."""
    s = float(s)
    w = _three(weights, "weights")
    m = []
    for c in range(3):
        m.extend([(1.0 - s) * w[k] + (s if k == c else 0.0) for k in range(3)] + [0.0])
    return m


def cdl(slope, offset, power, saturation=1.0, size=1025, domain=(0.0, 1.0)):
    """The ASC CDL -> (table, matrix): per channel clamp(x * slope + offset, 0, 1) ** power sampled at the nodes, then the
    Rec.709-weighted saturation matrix.  slope, offset and power are a number or one per channel; slope >= 0, power > 0."""
    slope, offset, power = _three(slope, "slope"), _three(offset, "offset"), _three(power, "power")
    if min(slope) < 0.0 or min(power) <= 0.0:
        raise ValueError("a CDL takes slope >= 0 and power > 0")
    table = curves_from_function(lambda c, x: min(max(x * slope[c] + offset[c], 0.0), 1.0) ** power[c], size, domain)
    return table, saturation_matrix(saturation)


def lift_gamma_gain(lift, gamma, gain, size=1025):
    """Lift / gamma / gain on [0, 1] -> the table: per channel y = gain * (x + lift * (1 - x)), then max(y, 0) ** (1 / gamma).
    lift 0, gamma 1, gain 1 change nothing; each is a number or one per channel; gamma > 0."""
    lift, gamma, gain = _three(lift, "lift"), _three(gamma, "gamma"), _three(gain, "gain")
    if min(gamma) <= 0.0:
        raise ValueError("gamma must be above 0")
    return curves_from_function(lambda c, x: max(gain[c] * (x + lift[c] * (1.0 - x)), 0.0) ** (1.0 / gamma[c]), size, (0.0, 1.0))


def _monotone_cubic(points):
    """Control points [(x, y), ...] -> f(x): the Fritsch-Carlson monotone cubic Hermite spline through them, held flat outside
    the first and the last.  Two points give the line through them, one gives a constant."""
    pts = sorted((float(x), float(y)) for x, y in points)
    if not pts:
        raise ValueError("a curve needs at least one control point")
    xs, ys = [p[0] for p in pts], [p[1] for p in pts]
    for a, b in zip(xs, xs[1:]):
        if not a < b:
            raise ValueError("two control points share x = %g" % b)
    n = len(pts)
    if n == 1:
        return lambda x: ys[0]
    h = [xs[k + 1] - xs[k] for k in range(n - 1)]
    d = [(ys[k + 1] - ys[k]) / h[k] for k in range(n - 1)]
    m = [d[0]] + [0.0 if d[k - 1] * d[k] <= 0.0 else (d[k - 1] + d[k]) / 2.0 for k in range(1, n - 1)] + [d[-1]]
    for k in range(n - 1):
        if d[k] == 0.0:
            m[k] = m[k + 1] = 0.0
            continue
        a, b = m[k] / d[k], m[k + 1] / d[k]
        if a < 0.0:
            m[k] = a = 0.0
        if b < 0.0:
            m[k + 1] = b = 0.0
        r = a * a + b * b
        if r > 9.0:
            t = 3.0 / math.sqrt(r)
            m[k], m[k + 1] = t * a * d[k], t * b * d[k]

    def f(x):
        if x <= xs[0]:
            return ys[0]
        if x >= xs[-1]:
            return ys[-1]
        lo, hi = 0, n - 1
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if xs[mid] <= x:
                lo = mid
            else:
                hi = mid
        if x == xs[lo]:
            return ys[lo]
        t = (x - xs[lo]) / h[lo]
        t2, t3 = t * t, t * t * t
        return ((2 * t3 - 3 * t2 + 1) * ys[lo] + (t3 - 2 * t2 + t) * h[lo] * m[lo] + (-2 * t3 + 3 * t2) * ys[lo + 1] + (t3 - t2) * h[lo] * m[lo + 1])
    return f


def curves_from_points(r, g, b, master=None, size=1025, domain=(0, 1)):
    """Curves through control points -> the table.  r, g, b, master: lists of (x, y), or None for the identity; each becomes a
    monotone cubic (Fritsch-Carlson: no overshoot between points, monotone where the points are) held flat outside its points,
    and `master` is applied in front of each channel's own curve: y = channel(master(x))."""
    fns = [(lambda x: x) if pts is None else _monotone_cubic(pts) for pts in (r, g, b)]
    first = (lambda x: x) if master is None else _monotone_cubic(master)
    return curves_from_function(lambda c, x: fns[c](first(x)), size, domain)


def _transfer(name):
    if name == "rec709_to_linear_scene":
        return lambda x: x / 4.5 if x < 4.5 * 0.018 else ((x + 0.099) / 1.099) ** (1.0 / 0.45)
    if name == "rec709_to_linear_display":
        return lambda x: 0.0 if x < 0.0 else x ** 2.5
    if name == "linear_to_rec709":
        return lambda x: x * 4.5 if x < 0.018 else 1.099 * x ** 0.45 - 0.099
    if name == "linear_to_srgb":
        return lambda x: x * 12.92 if x <= 0.0031308 else 1.055 * x ** (1.0 / 2.4) - 0.055
    raise ValueError("no such transfer function: %r (one of %s)" % (name, ", ".join(TRANSFERS)))


def transfer_curves(name, size=4097, domain=(0.0, 1.0)):
    """One of the library's four transfer functions (TRANSFERS: the tables of cvs_lut_host, in that order) as curves -> the
    table, the same in all three channels.  The default domain is [0, 1]; a wider one takes the function beyond it."""
    fn = _transfer(name)
    return curves_from_function(lambda c, x: fn(x), size, domain)


def resample_curves(table, size):
    """A table of any length >= 2 -> one of `size` nodes on the same domain, by linear interpolation: how a 1D `.cube` with more
    nodes than the filter takes is brought down."""
    _check_size(size)
    rows = [[float(v) for v in row] for row in table]
    n = len(rows)
    if n < 2 or any(len(row) != 3 for row in rows):
        raise ValueError("a table is at least two rows of three numbers")
    out = []
    for i in range(size):
        if i == size - 1:
            out.append(list(rows[-1]))
            continue
        t = i * (n - 1) / (size - 1)
        k = min(int(t), n - 2)
        f = t - k
        out.append([rows[k][c] * (1.0 - f) + rows[k + 1][c] * f for c in range(3)])
    return out


def parse_cube_1d(text, max_size=MAX_SIZE):
    """The text of a 1D `.cube` file -> (size, table, domain_min, domain_max, title).  Reads TITLE, LUT_1D_SIZE, DOMAIN_MIN,
    DOMAIN_MAX, comments (#) and blank lines; refuses LUT_3D_SIZE, unknown keywords, a wrong count of rows and values that are
    not finite, each with its line number.  A size above max_size (4097, the most a ColorCurves takes) is refused; with
    max_size=None any size from 2 is read, for resample_curves to bring down."""
    size, title = None, None
    domain_min, domain_max = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
    table, last = [], 0
    for line_no, raw in enumerate(text.splitlines(), 1):
        line = raw.strip()
        if not line or line.startswith("#"):
            continue
        last = line_no
        words = line.split()
        head = words[0]
        if head == "TITLE":
            title = line[len("TITLE"):].strip().strip('"')
        elif head == "LUT_3D_SIZE":
            raise CubeError("line %d: LUT_3D_SIZE: a 3D table, only 1D tables are read here (fluggo.media.cube.parse_cube reads it)" % line_no)
        elif head == "LUT_1D_SIZE":
            if size is not None:
                raise CubeError("line %d: LUT_1D_SIZE given twice" % line_no)
            if len(words) != 2 or not words[1].isdigit():
                raise CubeError("line %d: LUT_1D_SIZE takes one whole number" % line_no)
            size = int(words[1])
            if size < MIN_SIZE:
                raise CubeError("line %d: LUT_1D_SIZE %d, below %d" % (line_no, size, MIN_SIZE))
            if max_size is not None and size > max_size:
                raise CubeError("line %d: LUT_1D_SIZE %d, above %d: read it with max_size=None and bring it down with resample_curves" % (line_no, size, max_size))
        elif head == "DOMAIN_MIN":
            domain_min = tuple(_numbers(words[1:], 3, line_no, head))
        elif head == "DOMAIN_MAX":
            domain_max = tuple(_numbers(words[1:], 3, line_no, head))
        elif head[0].isupper() and head.replace("_", "").isalnum() and head.upper() == head:     # (inf and nan are numbers, refused as such)
            raise CubeError("line %d: unknown keyword %s" % (line_no, head))
        else:
            if size is None:
                raise CubeError("line %d: a table row before LUT_1D_SIZE" % line_no)
            if len(table) == size:
                raise CubeError("line %d: more than the %d rows of a table of size %d" % (line_no, size, size))
            table.append(_numbers(words, 3, line_no, "a table row"))
    if size is None:
        raise CubeError("line %d: no LUT_1D_SIZE" % last)
    if len(table) != size:
        raise CubeError("line %d: %d rows, a table of size %d has %d" % (last, len(table), size, size))
    for c in range(3):
        if not domain_min[c] < domain_max[c]:
            raise CubeError("line %d: DOMAIN_MIN %g is not below DOMAIN_MAX %g" % (last, domain_min[c], domain_max[c]))
    return size, table, domain_min, domain_max, title


def read_cube_1d(path_or_text, max_size=MAX_SIZE):
    """A 1D `.cube` file, by path or as its text (anything with a line break in it, or that names no file) ->
    (size, table, domain_min, domain_max): the constructor arguments of process.ColorCurves."""
    text = path_or_text
    if isinstance(path_or_text, os.PathLike) or (isinstance(path_or_text, str) and "\n" not in path_or_text and os.path.exists(path_or_text)):
        with open(path_or_text, "r") as f:
            text = f.read()
    return parse_cube_1d(text, max_size)[:4]


def write_cube_1d(table, domain_min=(0.0, 0.0, 0.0), domain_max=(1.0, 1.0, 1.0), title=None):
    """The text of a 1D `.cube` file; floats are written with repr, so read_cube_1d gives the same numbers back."""
    rows = [[float(v) for v in row] for row in table]
    if len(rows) < MIN_SIZE or any(len(row) != 3 for row in rows):
        raise ValueError("a table is at least two rows of three numbers")
    lines = []
    if title is not None:
        lines.append('TITLE "%s"' % title)
    lines.append("LUT_1D_SIZE %d" % len(rows))
    lines.append("DOMAIN_MIN %r %r %r" % tuple(float(v) for v in domain_min))
    lines.append("DOMAIN_MAX %r %r %r" % tuple(float(v) for v in domain_max))
    for row in rows:
        lines.append("%r %r %r" % tuple(row))
    return "\n".join(lines) + "\n"


def secondary(source, graded, hue=None, saturation=None, luma=None, invert=False, choke=0, feather=None):
    """A secondary grade as a graph of `fluggo.media.process` nodes: `graded` where the pixels of `source` fall inside the hue,
    saturation and luma ranges, `source` elsewhere.

        qualified = VideoQualifierFilter(source, hue, saturation, luma, invert=invert)     # source's alpha times the matte
        matte     = VideoMatteFilter(qualified, choke, feather)                              # left out when choke == 0 and feather is None
        out       = VideoMatteMixFilter(source, graded, matte)

    hue is (center, width, softness) in degrees, saturation and luma are (low, high, soft_low, soft_high); None: the axis does not
    qualify.  Returns the last node."""
    from fluggo.media import process
    matte = process.VideoQualifierFilter(source, hue=hue, saturation=saturation, luma=luma, invert=invert)
    if choke != 0 or feather is not None:
        matte = process.VideoMatteFilter(matte, choke=choke, feather=feather)
    return process.VideoMatteMixFilter(source, graded, matte)
