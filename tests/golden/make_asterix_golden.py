"""Writes tests/golden/asterix_cases.npz: case records for the ASTERIX CAT021 output (tests/asterix_util.py: fuzz_cases, edge_cases,
tie_cases, outside_cases) and what the REFERENCE's own writer, modesSendAsterixOutput, writes for them — tests/host_stub/
asterix_ref_harness.c, which includes the reference's net_io.c and is linked with the objects `make -C oracle full` builds.  Run from
the repo root in the dev container.

Groups: (a) field records of fuzzed frames of every DF / ME type and of Comm-B registers through the oracle's field decode, every item
of the record present in at least 300 of them and absent in as many, with gate-like verdicts, candidate positions, receiver ids and
aircraft state; (b) the edges: every category byte with the aircraft's category 0 and not, every combination of the seven inputs of
I021/090, the I021/040 forms, every FSPEC length, sysTimestamps around midnight and the 32-bit wrap, all 4096 squawks under four
patterns of the other bits, callsigns in and outside the AIS set, both MOPS branches, receiver ids, the integer divisions, the longest
record, random flag combinations; (c) conversion ties: for each scaled item the source values whose product sits on and next to an
integer, zeros of both signs, the ends of the domain; (d) records outside the domain — not given to the harness, their class pinned.

What is stored: the case arrays; `ref_<group>_r<remote>`, the harness's bytes for every record of the group that lies in the domain,
without verdicts (the writer knows none), with mm->remote 0 and 1; `ref_clock_<now_ms>`, the clock cases at other values of the
clock; `cls_*`, the class the library's rules give every record.  Every stream is asserted here to be, byte for byte, what
tests/asterix_util.py's checker writes."""
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import asterix_util as au  # noqa: E402

assert au.have_ref_full(), "needs the reference tree and `make -C oracle full`"
PER_ITEM = 300
sets = {"a": au.fuzz_cases(PER_ITEM, 21), "b": au.edge_cases(22), "c": au.tie_cases(23), "d": au.outside_cases()}
store = {f"{g}_{k}": v for g, c in sets.items() for k, v in c.items()}

with tempfile.TemporaryDirectory() as tmp:
    exe = au.build_ref_harness(tmp)
    items = {}
    for g in ("a", "b", "c"):
        sub = au.in_domain(sets[g])
        for now_ms, remote in au.RUNS:
            got, lens = au.run_ref_harness(exe, sub, now_ms=now_ms, remote=remote, workdir=tmp)
            want = au.asterix_of(sub, now_ms=now_ms, gated=False, remote=bool(remote), want_items=True)
            assert got == want[0] and (lens == want[1]).all(), f"the checker differs from the reference's writer: group {g}, remote {remote}"
            assert (lens >= 7).all() and lens.max() <= au.RECORD_MAX
            store[f"ref_{g}_r{remote}"] = np.frombuffer(got, dtype=np.uint8)
            items[g] = want[4]
    clock = au.clock_cases()
    for now_ms in au.CLOCKS:
        got, lens = au.run_ref_harness(exe, clock, now_ms=now_ms, workdir=tmp)
        assert got == au.asterix_of(clock, now_ms=now_ms, gated=False)[0], f"clock {now_ms}"
        store[f"ref_clock_{now_ms}"] = np.frombuffer(got, dtype=np.uint8)

# ---- coverage, on what the reference wrote -----------------------------------------------------------------------------------------
optional = sorted(set(au.FSPEC_BITS) - {"010", "040", "080", "090", "077"})
for name in optional:
    present = sum(name in it for it in items["a"])
    print(f"  group a: I021/{name} present in {present}, absent in {len(items['a']) - present}")
    assert present >= PER_ITEM and len(items["a"]) - present >= PER_ITEM, name
lens_b = [len(r) for r in au.split_records(store["ref_b_r0"].tobytes())]
assert max(lens_b) == au.RECORD_MAX, "the longest record is reached"
fspec_lens = set()
for r in au.split_records(store["ref_b_r0"].tobytes()):
    k = 3
    while r[k] & 1:
        k += 1
    fspec_lens.add(k - 2)
assert fspec_lens == {4, 5, 6}, fspec_lens
assert store["ref_b_r0"].tobytes() != store["ref_b_r1"].tobytes(), "both MOPS branches"

for g in au.GROUPS:
    c = sets[g]
    store[f"cls_{g}"] = au.asterix_classes(c["fields"], c["positions"], c["verdict"], c["ac_baro_alt"])
assert (store["cls_d"] == au.SKIP).sum() >= 40
np.savez_compressed(au.GOLDEN, **store)
print(au.GOLDEN, {g: len(c["msgs"]) for g, c in sets.items()}, os.path.getsize(au.GOLDEN), "bytes")
assert os.path.getsize(au.GOLDEN) <= os.path.getsize(os.path.join(os.path.dirname(au.GOLDEN), "text_cases.npz")), "no larger than text_cases.npz"
