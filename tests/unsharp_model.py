"""Numpy statement of the unsharp mask's contract (DESIGN.md "Unsharp mask"), independent of the kernels.

B comes from outside (the CPU oracle's orc_fir_blur_f32 in the flavour under test, or tests/models.py blur_model); the mask
itself is stated here one f32 operation at a time, the same in both arithmetic flavours:

    for c in r, g, b:   d = s.c - B.c ;  out.c = s.c if fabsf(d) < threshold else s.c + amount * d
    out.a = s.a

`s` is the source pixel; an f16 source is widened exactly, with a signalling NaN coming out quiet (what the device's and
x86's conversion instructions do; numpy's software conversion does not, so it is stated here).  f16 results are truncated
once, by tests/models.py f2h_rz_model."""
import numpy as np

from tests.models import f2h_rz_model

F32 = np.float32


def widen(codes):
    """f16 codes -> f32, exact; NaNs quiet."""
    out = np.ascontiguousarray(codes, np.uint16).view(np.float16).astype(F32)
    bits = out.view(np.uint32)
    bits[np.isnan(out)] |= np.uint32(0x00400000)
    return out


def mask(source, blurred, amount, threshold):
    """source, blurred: (..., 4) f32 arrays of one shape -> the masked pixels, f32."""
    s = np.ascontiguousarray(source, F32)
    b = np.ascontiguousarray(blurred, F32)
    amount, threshold = F32(amount), F32(threshold)
    out = s.copy()
    with np.errstate(all="ignore"):
        for c in range(3):
            d = (s[..., c] - b[..., c]).astype(F32)
            sharp = (s[..., c] + (amount * d).astype(F32)).astype(F32)
            out[..., c] = np.where(np.abs(d) < threshold, s[..., c], sharp)        # a NaN d fails the comparison
    return out


def intersect(a, b):
    w = (max(a[0], b[0]), max(a[1], b[1]), min(a[2], b[2]), min(a[3], b[3]))
    return None if w[2] < w[0] or w[3] < w[1] else w


def crop(array, full, win):
    return array[win[1] - full[1]:win[3] - full[1] + 1, win[0] - full[0]:win[2] - full[0] + 1]


def expected(before, target_full, source, source_full, source_cur, blur, amount, threshold):
    """The target buffer after the call and its window.  before: the target's pixels beforehand (uint16 codes or f32);
    source: pixels over source_full in the same format; blur(source_f32, source_full, source_cur, win) -> B over win, f32.
    Pixels outside the window keep what `before` held."""
    out = before.copy()
    win = None if source_cur is None else intersect(source_cur, target_full)
    if win is None:
        return out, None
    half = before.dtype == np.uint16
    s32 = widen(source) if half else np.ascontiguousarray(source, F32)
    masked = mask(crop(s32, source_full, win), blur(s32, source_full, source_cur, win), amount, threshold)
    crop(out, target_full, win)[...] = f2h_rz_model(masked) if half else masked
    return out, win
