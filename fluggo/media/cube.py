"""3D colour lookup tables as values: reading `.cube` files and baking colour functions into a lattice.

Everything here is plain Python and returns the constructor arguments of `fluggo.media.process.Lut3D`:

    size, table, domain_min, domain_max = read_cube("look.cube")
    lut = process.Lut3D(size, table, domain_min, domain_max)

`table` is a flat list of size**3 * 3 floats, red fastest: the node of lattice index (ir, ig, ib) starts at
3 * (ir + size * (ig + size * ib)), which is the order of a `.cube` file's rows.
"""
import math
import os

MIN_SIZE, MAX_SIZE = 2, 65


class CubeError(ValueError):
    """A `.cube` text that cannot be read; the message names the line."""


def _numbers(words, count, line_no, what):
    if len(words) != count:
        raise CubeError("line %d: %s takes %d numbers, found %d" % (line_no, what, count, len(words)))
    try:
        values = [float(w) for w in words]
    except ValueError:
        raise CubeError("line %d: %s: not a number" % (line_no, what)) from None
    for v in values:
        if not math.isfinite(v):
            raise CubeError("line %d: %s: a value that is not finite" % (line_no, what))
    return values


def parse_cube(text):
    """The text of a `.cube` file -> (size, table, domain_min, domain_max, title).  Reads TITLE, LUT_3D_SIZE, DOMAIN_MIN,
    DOMAIN_MAX, comments (#) and blank lines; refuses LUT_1D_SIZE, unknown keywords, a wrong count of rows and values that are
    not finite, each with its line number."""
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
        elif head == "LUT_1D_SIZE":
            raise CubeError("line %d: LUT_1D_SIZE: a 1D table, only 3D tables are read" % line_no)
        elif head == "LUT_3D_SIZE":
            if size is not None:
                raise CubeError("line %d: LUT_3D_SIZE given twice" % line_no)
            if len(words) != 2 or not words[1].isdigit():
                raise CubeError("line %d: LUT_3D_SIZE takes one whole number" % line_no)
            size = int(words[1])
            if not MIN_SIZE <= size <= MAX_SIZE:
                raise CubeError("line %d: LUT_3D_SIZE %d, outside %d..%d" % (line_no, size, MIN_SIZE, MAX_SIZE))
        elif head == "DOMAIN_MIN":
            domain_min = tuple(_numbers(words[1:], 3, line_no, head))
        elif head == "DOMAIN_MAX":
            domain_max = tuple(_numbers(words[1:], 3, line_no, head))
        elif head[0].isupper() and head.replace("_", "").isalnum() and head.upper() == head:     # (inf and nan are numbers, refused as such)
            raise CubeError("line %d: unknown keyword %s" % (line_no, head))
        else:
            if size is None:
                raise CubeError("line %d: a table row before LUT_3D_SIZE" % line_no)
            if len(table) == size ** 3 * 3:
                raise CubeError("line %d: more than the %d rows of a table of size %d" % (line_no, size ** 3, size))
            table.extend(_numbers(words, 3, line_no, "a table row"))
    if size is None:
        raise CubeError("line %d: no LUT_3D_SIZE" % last)
    if len(table) != size ** 3 * 3:
        raise CubeError("line %d: %d rows, a table of size %d has %d" % (last, len(table) // 3, size, size ** 3))
    for c in range(3):
        if not domain_min[c] < domain_max[c]:
            raise CubeError("line %d: DOMAIN_MIN %g is not below DOMAIN_MAX %g" % (last, domain_min[c], domain_max[c]))
    return size, table, domain_min, domain_max, title


def read_cube(path_or_text):
    """A `.cube` file, by path or as its text (anything with a line break in it, or that names no file) ->
    (size, table, domain_min, domain_max): the constructor arguments of process.Lut3D."""
    text = path_or_text
    if isinstance(path_or_text, os.PathLike) or (isinstance(path_or_text, str) and "\n" not in path_or_text and os.path.exists(path_or_text)):
        with open(path_or_text, "r") as f:
            text = f.read()
    return parse_cube(text)[:4]


def write_cube(size, table, domain_min=(0.0, 0.0, 0.0), domain_max=(1.0, 1.0, 1.0), title=None):
    """The text of a `.cube` file; floats are written with repr, so read_cube gives the same numbers back."""
    if len(table) != size ** 3 * 3:
        raise ValueError("table holds %d values, a lattice of size %d takes %d" % (len(table), size, size ** 3 * 3))
    lines = []
    if title is not None:
        lines.append('TITLE "%s"' % title)
    lines.append("LUT_3D_SIZE %d" % size)
    lines.append("DOMAIN_MIN %r %r %r" % tuple(float(v) for v in domain_min))
    lines.append("DOMAIN_MAX %r %r %r" % tuple(float(v) for v in domain_max))
    for k in range(0, len(table), 3):
        lines.append("%r %r %r" % (float(table[k]), float(table[k + 1]), float(table[k + 2])))
    return "\n".join(lines) + "\n"


def lattice_from_function(fn, size, domain_min=(0.0, 0.0, 0.0), domain_max=(1.0, 1.0, 1.0)):
    """Samples fn(r, g, b) -> (r', g', b') on the lattice: how a CDL, a curve or a saturation change becomes a cube.
    -> (size, table, domain_min, domain_max)"""
    if not MIN_SIZE <= size <= MAX_SIZE:
        raise ValueError("size %d, outside %d..%d" % (size, MIN_SIZE, MAX_SIZE))
    domain_min, domain_max = tuple(float(v) for v in domain_min), tuple(float(v) for v in domain_max)
    axis = [[domain_min[c] + i * (domain_max[c] - domain_min[c]) / (size - 1) for i in range(size)] for c in range(3)]
    table = []
    for b in axis[2]:
        for g in axis[1]:
            for r in axis[0]:
                out = tuple(fn(r, g, b))
                if len(out) != 3:
                    raise ValueError("the colour function must return three numbers")
                table.extend(float(v) for v in out)
    return size, table, domain_min, domain_max


def identity_lattice(size):
    """The lattice on [0, 1] that changes nothing -> (size, table, domain_min, domain_max)"""
    return lattice_from_function(lambda r, g, b: (r, g, b), size)
