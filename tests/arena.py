"""A guarded arena: frames, coded planes and byte targets packed into ONE device allocation at chosen base addresses, every
object with a poisoned guard band on either side, so that an access outside a frame's buffer (which in an editor's ring of
frames is the neighbouring frame) is seen, and so that the base-address term of the launchers' predicates can be flipped.

Two layers.  `Layout` is the arithmetic: where objects go, which bytes are guards, what the poison is, and the check of a
downloaded image; it works on numpy byte arrays and is tested without a GPU (tests/test_arena_cpu.py).  `Arena` puts a Layout
over one cvs_malloc block.

The guard sizes are conditions, not measurements: every placed object has at least `guard` bytes of poison before and after it,
where guard >= 4 KiB and >= two rows of the largest frame of the case, and nothing is ever placed against the end of the
allocation -- a stray access of that extent stays inside memory the test owns and cannot fault.
"""
import ctypes as C

import numpy as np

from canvas_amd.abi import box2i

MODULUS = 256                 # residues are taken modulo this (cvs_malloc blocks start on at least such a boundary)
MIN_GUARD = 4096

# NaN in both pixel formats (half 0xFFFF, float 0xFFFFFFFF) / finite and non-zero in both (half 0x3C00 = 1.0, float 0x3C003C00 = 0.0078...)
POISON_NAN = bytes([0xFF, 0xFF])
POISON_FINITE = bytes([0x00, 0x3C])
POISONS = (("nan", POISON_NAN), ("finite", POISON_FINITE))


def guard_bytes(row_bytes):
    """The guard for a case whose frames' rows are `row_bytes` long (an iterable): >= 4 KiB, >= two rows of the largest."""
    g = max([MIN_GUARD] + [2 * int(r) for r in row_bytes])
    return (g + MODULUS - 1) // MODULUS * MODULUS


def capacity_for(sizes, guard):
    """Bytes that hold objects of these sizes at any residues, with their guards."""
    sizes = [int(n) for n in sizes]
    return sum(sizes) + (len(sizes) + 1) * (guard + MODULUS) + MODULUS


class Placed:
    def __init__(self, name, offset, nbytes, residue):
        self.name, self.offset, self.nbytes, self.residue = name, offset, nbytes, residue
        self.uploaded = None            # bytes of an INPUT object as uploaded (None: an output, free to change)

    @property
    def end(self):
        return self.offset + self.nbytes


class Layout:
    """Where things go in an arena of `capacity` bytes whose first byte has address `base` (only base modulo 256 matters)."""

    def __init__(self, capacity, guard, base=0):
        assert guard >= MIN_GUARD and capacity > 2 * guard
        self.capacity, self.guard, self.base = int(capacity), int(guard), int(base)
        self.objects = []
        self.cursor = 0                 # end of the last object (0: nothing placed)

    def add(self, nbytes, residue, name=None):
        """Place `nbytes` at the first offset >= cursor + guard whose address is `residue` modulo 256, leaving a whole guard
        before the end of the arena.  An empty object still gets an address and its guards."""
        assert 0 <= residue < MODULUS and nbytes >= 0
        off = self.cursor + self.guard
        off += (residue - (self.base + off)) % MODULUS
        if off + nbytes + self.guard > self.capacity:
            raise MemoryError("arena of %d bytes: no room for %d bytes at offset %d with a %d-byte trailing guard" % (
                self.capacity, nbytes, off, self.guard))
        p = Placed(name or "object %d" % len(self.objects), off, int(nbytes), residue)
        self.objects.append(p)
        self.cursor = p.end
        return p

    def guard_mask(self):
        """True for every byte of the arena that belongs to no object."""
        m = np.ones(self.capacity, bool)
        for p in self.objects:
            m[p.offset:p.end] = False
        return m

    def poison_image(self, poison):
        """The whole arena filled with the repeating pattern, phase locked to offset 0."""
        reps = (self.capacity + len(poison) - 1) // len(poison)
        return np.frombuffer(bytes(poison) * reps, np.uint8)[:self.capacity].copy()

    def nearest(self, offset):
        """(object, side) a guard byte is nearest to: side is 'before' or 'after' that object."""
        best = None
        for p in self.objects:
            for side, d in (("before", p.offset - offset), ("after", offset - p.end + 1)):
                if d > 0 and (best is None or d < best[0]):
                    best = (d, p, side)
        assert best is not None, "no objects placed"
        return best[1], best[2], best[0]

    def check(self, image, poison):
        """image: the arena's bytes after the call.  Every guard byte must still hold the poison, every input object what was
        uploaded into it."""
        image = np.ascontiguousarray(image, np.uint8).reshape(-1)
        assert image.size == self.capacity, (image.size, self.capacity)
        bad = np.flatnonzero((image != self.poison_image(poison)) & self.guard_mask())
        if bad.size:
            off = int(bad[0])
            p, side, dist = self.nearest(off)
            raise GuardViolation("%d guard bytes changed; first at arena offset %d (0x%02x, poison 0x%02x): %d bytes %s %r (object at %d..%d)" % (
                bad.size, off, image[off], self.poison_image(poison)[off], dist, side, p.name, p.offset, p.end - 1), off, p, side)
        for p in self.objects:
            if p.uploaded is None:
                continue
            now = image[p.offset:p.end]
            was = np.frombuffer(p.uploaded, np.uint8)
            if not np.array_equal(now, was):
                at = int(np.flatnonzero(now != was)[0])
                raise InputWritten("input %r was written: first at byte %d of %d (0x%02x, was 0x%02x)" % (p.name, at, p.nbytes, now[at], was[at]), p, at)


class GuardViolation(AssertionError):
    def __init__(self, msg, offset, placed, side):
        AssertionError.__init__(self, msg)
        self.offset, self.placed, self.side = offset, placed, side


class InputWritten(AssertionError):
    def __init__(self, msg, placed, at):
        AssertionError.__init__(self, msg)
        self.placed, self.at = placed, at


class Arena:
    """A Layout over one cvs_malloc block.  Poison first (fill), then place and upload, run the call, check()."""

    def __init__(self, lib, capacity, guard):
        from canvas_amd import _lib
        self._lib, self._check_rc = lib, _lib.check
        self.ptr = lib.cvs_malloc(capacity)
        if not self.ptr:
            raise MemoryError("cvs_malloc(%d)" % capacity)
        self.capacity, self.guard = capacity, guard
        self.layout = None
        self.poison = None

    def fill(self, poison):
        """Start a run: forget every placement, fill the whole arena with `poison`."""
        self.layout = Layout(self.capacity, self.guard, self.ptr % MODULUS)
        self.poison = poison
        img = self.layout.poison_image(poison)
        self._check_rc(self._lib.cvs_memcpy_h2d(self.ptr, img.ctypes.data, self.capacity, None), "poison")

    def place_bytes(self, nbytes, residue, name=None):
        """-> (device address, Placed) of `nbytes` at `residue` modulo 256."""
        p = self.layout.add(nbytes, residue, name)
        assert (self.ptr + p.offset) % MODULUS == residue
        return self.ptr + p.offset, p

    def place(self, full_window, dtype, residue, current_window=None, name=None):
        """-> DeviceFrame over `full_window` whose data is at `residue` modulo 256 (its .placed is the Layout's record)."""
        from canvas_amd.device import DeviceFrame
        fw = full_window if isinstance(full_window, box2i) else box2i.of(*full_window)
        nbytes = fw.height * fw.width * 4 * np.dtype(dtype).itemsize
        addr, p = self.place_bytes(nbytes, residue, name)
        f = DeviceFrame(fw, dtype, current_window, ptr=addr)
        f.placed = p
        return f

    def upload(self, placed, data, is_input):
        """Contents of a placed object; an input's are remembered for check()."""
        raw = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        assert raw.size == placed.nbytes, (raw.size, placed.nbytes)
        if raw.size:
            self._check_rc(self._lib.cvs_memcpy_h2d(self.ptr + placed.offset, raw.ctypes.data, raw.size, None), "h2d")
        placed.uploaded = raw.tobytes() if is_input else None

    def download(self):
        """The whole arena, once."""
        self._check_rc(self._lib.cvs_stream_sync(None), "sync")
        img = np.empty(self.capacity, np.uint8)
        self._check_rc(self._lib.cvs_memcpy_d2h(img.ctypes.data, self.ptr, self.capacity, None), "d2h")
        self.image = img
        return img

    def read(self, placed, dtype=np.uint8):
        return self.image[placed.offset:placed.end].copy().view(dtype)

    def check(self):
        self.layout.check(self.image, self.poison)

    def free(self):
        if self.ptr:
            self._lib.cvs_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
