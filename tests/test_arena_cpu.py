"""The guarded arena's own arithmetic, held to account without a GPU (tests/arena.py Layout): placements honour their residues
whatever the base address, guards have the stated size, nothing overlaps, a single changed guard byte is found and attributed
to the right object and side, a changed input byte is found, and an untouched arena passes."""
import numpy as np
import pytest

from tests import arena as ar

SIZES = [0, 1, 8, 24, 1000, 4096, 130 * 9 * 8, 65 * 7 * 16, 480 * 180]
RESIDUES = [0, 8, 24, 136, 16, 48, 144, 1, 2, 3, 7, 4, 12]


def _layout(base, guard=None, sizes=SIZES, residues=RESIDUES):
    guard = guard or ar.guard_bytes([130 * 8])
    lay = ar.Layout(ar.capacity_for(sizes, guard), guard, base)
    for k, n in enumerate(sizes):
        lay.add(n, residues[k % len(residues)], "object-%d" % k)
    return lay


def test_guard_size_is_at_least_4k_and_two_rows_of_the_largest_frame():
    assert ar.guard_bytes([]) == 4096
    assert ar.guard_bytes([130 * 8, 64 * 16]) == 4096
    assert ar.guard_bytes([1100 * 16]) >= 2 * 1100 * 16
    assert ar.guard_bytes([1025 * 8, 300 * 8]) >= 2 * 1025 * 8
    for rows in ([], [1], [2047], [2048], [2049], [17600]):
        g = ar.guard_bytes(rows)
        assert g >= 4096 and g >= 2 * max(rows + [0]) and g % ar.MODULUS == 0


@pytest.mark.parametrize("base", [0, 256, 4096 + 128, 64, 8, 1])
def test_residues_are_honoured_whatever_the_base(base):
    lay = _layout(base)
    for k, p in enumerate(lay.objects):
        assert (base + p.offset) % ar.MODULUS == RESIDUES[k % len(RESIDUES)] == p.residue
        assert p.nbytes == SIZES[k]


@pytest.mark.parametrize("base", [0, 8, 200])
@pytest.mark.parametrize("rows", [[130 * 8], [1100 * 16]])
def test_every_object_has_a_whole_guard_on_both_sides_and_nothing_overlaps(base, rows):
    guard = ar.guard_bytes(rows)
    lay = _layout(base, guard)
    assert lay.objects[0].offset >= guard
    for a, b in zip(lay.objects, lay.objects[1:]):
        assert b.offset - a.end >= guard                     # which also says that they do not overlap, in placement order
    assert lay.capacity - lay.objects[-1].end >= guard      # nothing sits against the end of the allocation
    mask = lay.guard_mask()
    assert mask.sum() == lay.capacity - sum(SIZES)           # objects cover their own bytes once: no two share a byte
    for p in lay.objects:
        assert not mask[p.offset:p.end].any()
        assert mask[p.offset - guard:p.offset].all() and mask[p.end:p.end + guard].all()


def test_an_arena_without_room_for_the_trailing_guard_refuses():
    guard = ar.guard_bytes([])
    lay = ar.Layout(3 * guard, guard)
    lay.add(guard - 300, 0)
    with pytest.raises(MemoryError):
        lay.add(1, 0)                                        # would fit, but not with its guard behind it
    assert len(lay.objects) == 1


@pytest.mark.parametrize("name,poison", ar.POISONS)
def test_the_poisons_are_what_they_claim(name, poison):
    lay = _layout(0)
    img = lay.poison_image(poison)
    assert img.size == lay.capacity
    halfs, floats = img[:64].view(np.uint16), img[:64].view(np.float32)
    if name == "nan":
        assert ((halfs & 0x7C00) == 0x7C00).all() and (halfs & 0x3FF).all() and np.isnan(floats).all()
    else:
        assert (halfs == 0x3C00).all() and np.isfinite(floats).all() and (floats != 0).all()
    # at every residue a frame may take (multiples of 8), a pixel read from the guard is that pattern, not a shifted one
    assert (img[8:16].view(np.uint16) == halfs[0]).all()


@pytest.mark.parametrize("name,poison", ar.POISONS)
def test_an_untouched_arena_passes(name, poison):
    lay = _layout(24)
    img = lay.poison_image(poison)
    rng = np.random.default_rng(1)
    for k, p in enumerate(lay.objects):
        data = rng.integers(0, 256, p.nbytes, dtype=np.uint8)
        img[p.offset:p.end] = data
        if k % 2 == 0:
            p.uploaded = data.tobytes()                      # inputs; the odd ones are outputs, free to hold anything
    lay.check(img, poison)
    for p in lay.objects:                                    # outputs may change
        if p.uploaded is None:
            img[p.offset:p.end] ^= 0x5A
    lay.check(img, poison)


@pytest.mark.parametrize("name,poison", ar.POISONS)
def test_one_changed_guard_byte_anywhere_is_found_and_attributed(name, poison):
    lay = _layout(8)
    clean = lay.poison_image(poison)
    spots = [(0, lay.objects[0], "before"), (lay.capacity - 1, lay.objects[-1], "after")]
    for k, p in enumerate(lay.objects):
        spots.append((p.offset - 1, p, "before"))            # the byte just before its first
        spots.append((p.end, p, "after"))                    # one past its last: the store past the last row
        spots.append((p.end + lay.guard // 2 - 1, p, "after"))
        spots.append((p.offset - lay.guard // 2 + 1, p, "before"))
    for off, p, side in spots:
        img = clean.copy()
        img[off] ^= 0x01                                     # one bit
        with pytest.raises(ar.GuardViolation) as e:
            lay.check(img, poison)
        assert e.value.offset == off and e.value.placed is p and e.value.side == side, (off, p.name, side, str(e.value))
        assert p.name in str(e.value) and side in str(e.value)
    # every guard byte is looked at, not a sample
    rng = np.random.default_rng(2)
    guards = np.flatnonzero(lay.guard_mask())
    for off in rng.choice(guards, 200, replace=False):
        img = clean.copy()
        img[off] = (int(img[off]) + 1) & 0xFF
        with pytest.raises(ar.GuardViolation) as e:
            lay.check(img, poison)
        assert e.value.offset == off


def test_the_first_of_several_changed_guard_bytes_is_reported():
    lay = _layout(0)
    img = lay.poison_image(ar.POISON_NAN)
    a, b = lay.objects[2], lay.objects[5]
    img[b.end + 3] = 0
    img[a.end + 9] = 0
    with pytest.raises(ar.GuardViolation) as e:
        lay.check(img, ar.POISON_NAN)
    assert e.value.offset == a.end + 9 and e.value.placed is a and e.value.side == "after"
    assert "2 guard bytes" in str(e.value)


def test_a_changed_input_byte_is_found():
    lay = _layout(0)
    img = lay.poison_image(ar.POISON_FINITE)
    rng = np.random.default_rng(3)
    for p in lay.objects:
        data = rng.integers(0, 256, p.nbytes, dtype=np.uint8)
        img[p.offset:p.end] = data
        p.uploaded = data.tobytes()
    lay.check(img, ar.POISON_FINITE)
    for p in lay.objects:
        for at in {0, p.nbytes // 2, p.nbytes - 1} if p.nbytes else ():
            bad = img.copy()
            bad[p.offset + at] ^= 0x80
            with pytest.raises(ar.InputWritten) as e:
                lay.check(bad, ar.POISON_FINITE)
            assert e.value.placed is p and e.value.at == at and p.name in str(e.value)


def test_an_object_written_with_the_poison_itself_is_not_mistaken_for_a_guard():
    """An output that happens to hold the poison's bytes is the object's business: only bytes outside objects are guards."""
    lay = _layout(0)
    img = lay.poison_image(ar.POISON_NAN)
    lay.check(img, ar.POISON_NAN)                            # objects never uploaded: still poison, and that is fine
    img[lay.objects[3].offset] = 0
    lay.check(img, ar.POISON_NAN)
