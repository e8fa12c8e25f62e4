"""Records what the reference's OWN code (oracle/ref_build.py -> oracle/_ref/, both flavours) computes on the seeded cases of
tests/reference_cases.py into tests/golden/reference_built.npz.  Run where the reference is built:

    python3 tests/golden/make_reference_golden.py

The GPU tests (tests/test_reference_fixtures_gpu.py) compare the library with this file and nothing else; a CPU test
(tests/test_reference_fixture_cpu.py) holds the file to what oracle.ref() produces today.  Inputs are not stored: every
test regenerates them from the seeds.

Layout, per flavour F in (gcc, fma) and case name N:
    F/index      JSON: {"cases": {N: {"sha": SHA-256 of the canonical codes of the whole target buffer followed by the
                 window, "win": the reported current_window, or (width, centre) for taps, or null}},
                 "domain": {K: SHA-256 of a whole-domain result (h2f, tables, ramp, f2h probe sets)}}
    F/N/codes    the canonical codes themselves (uint16 / uint32 / uint8)                 (the cases keeps_raw() names)
Raw codes are kept for what fits a file of well under 1 MB: random float pixels do not compress, and the 104 mixes on
51 x 26 frames alone are 2.2 MB per flavour.  The over keeps raw codes at mix 0.3 (all 13 window configurations); the cross, the 720 x 480 DV frames, the 1100-wide scaler target and the scaler at (2, 3), which fills all of its 100 x 80
target, are digests only; everything else is raw.  A digest
decides pass / fail just as well; the raw codes are there to say WHERE a difference is.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "tests", "golden", "reference_built.npz")


def keeps_raw(name):
    if name.startswith("cross/"):
        return False
    if name.startswith("over/"):
        return name.endswith("/0.3")
    return not name.startswith("dv/") and name != "scale/wide" and not name.endswith("/2,3")


def record(impl):
    from tests import reference_cases as rc
    out, index = {}, {"cases": {}, "domain": rc.domain_digests(impl)}
    for name, (codes, win) in rc.small_cases(impl).items():
        index["cases"][name] = {"sha": rc.digest(codes, win), "win": None if win is None else [int(v) for v in win]}
        if keeps_raw(name):
            out[name + "/codes"] = codes
    out["index"] = np.array(json.dumps(index, sort_keys=True))
    return out


def main():
    import oracle
    from tests import reference_cases as rc
    data = {}
    for flavour in ("gcc", "fma"):
        lib = oracle.ref(flavour)
        if lib is None:
            raise SystemExit("oracle/_ref is not built: run oracle/ref_build.py where the reference tree is")
        for k, v in record(rc.ref_abi(lib)).items():
            data[flavour + "/" + k] = v
    np.savez_compressed(OUT, **data)
    print("%s: %d entries, %d bytes" % (OUT, len(data), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
