"""Writes tests/golden/cpr_cases.npz: cases for cpr.c's three decoders (tests/cpr_util.py: golden_cases) and what the REFERENCE
returns for them — tests/host_stub/cpr_ref_harness.c linked (-no-pie) with the reference's own object oracle/_ref/full/cpr.o, which
`make -C oracle full` builds.  Run from the repo root in the dev container.

The cases: (a) each of the 58 NL thresholds with latitudes encoded just below and just above it, both parities, both hemispheres;
(b) pairs encoded from true positions, the second fix 0-3 km on — everywhere, the poles, the equator, +-180, airborne and surface;
(c) surface with the reference in each of the four longitude quadrants and at reflat +-45; (d) relative decodes with the reference
0.49 and 0.51 of a cell from the truth, in latitude and in longitude; (e) uniformly random words for the failing codes.
Which codes a function can return: airborne 0 / -1 / -2; relative 0 / -1; surface 0 / -1 — its -2 test (cpr.c:283) cannot fire:
both latitudes come out of [0, 90) and the quadrant step (cpr.c:264-280) moves them to -90, +90 or by -90 once."""
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import cpr_util as cu  # noqa: E402

CODES = {0: (-1, -2), 1: (-1,), 2: (-1,)}

cases = cu.golden_cases()
assert len(cases) <= 20000
with tempfile.TemporaryDirectory() as tmp:
    res = cu.run_ref_harness(cases, tmp)
for fn, codes in CODES.items():
    rc = res["rc"][cases["fn"] == fn]
    share = {c: float((rc == c).mean()) for c in (0,) + codes}
    print(f"fn {fn}: {len(rc)} cases, shares {share}")
    assert set(np.unique(rc)) <= set((0,) + codes)
    assert share[0] >= 0.5, "rc 0 is at least half of the cases"
    for c in codes:
        assert share[c] >= 0.02, f"rc {c} is at least 2 % of the cases"
assert (res["lat"][res["rc"] < 0] == 0).all() and (res["lon"][res["rc"] < 0] == 0).all()
out = cu.GOLDEN
np.savez_compressed(out, cases=np.frombuffer(cases.tobytes(), dtype=np.uint8), lat_bits=res["lat"].view(np.uint64), lon_bits=res["lon"].view(np.uint64),
                    rc=res["rc"].astype(np.int8))
print(out, len(cases), "cases,", os.path.getsize(out), "bytes")
assert os.path.getsize(out) < 1000000
