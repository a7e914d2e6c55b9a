"""Writes tests/golden/text_cases.npz: case records for the two text outputs (tests/sbs_util.py: fuzz_cases, edge_cases, double_cases,
float_cases, raw_cases) and what the REFERENCE's own writers print for them — tests/host_stub/text_ref_harness.c, which includes the
reference's net_io.c and is linked with the objects `make -C oracle full` builds.  Run from the repo root in the dev container.

Groups: (a) field records of fuzzed frames of every DF / ME type through the oracle's field decode, gate-like verdicts; (b) records at
the edges of the domain and outside it, flag combinations no decoder gives; (c) doubles: every exact tie of six decimals up to 180 with
both neighbours, the doubles nearest (k + 0.5) * 1e-6, zeros, subnormals, the ends of the domain; (d) floats k + 0.5 with neighbours;
(e) raw: timestamps around twelve hex digits, every length, every correctedbits.

What is stored: the case arrays; `ref_*`, the harness's bytes — every record of a group that lies in the domain through the reference's
writer, without verdicts (the writer knows none), for both use_gnss settings, the override squawks and the raw flags — asserted here
to be, record for record, what tests/sbs_util.py's references print; `cls_*`, the class the library's rules on top (verdicts, the skip
rule) give every record, so that a stream with verdicts is the reference's lines of exactly the records of class LINE; `want_raw_*`,
the raw streams with verdicts and the network rule.
The coverage conditions below are asserted on the reference's output: each makes up at least 2 % of its group."""
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import sbs_util as su  # noqa: E402

assert su.have_ref_full(), "needs the reference tree and `make -C oracle full`"
sets = {"a": su.fuzz_cases(200, 11), "b": su.edge_cases(12), "c": su.double_cases(13), "d": su.float_cases()}
raw_msgs, raw_verdict = su.raw_cases(14)
store = {f"{g}_{k}": v for g, c in sets.items() for k, v in c.items()}
store["e_msgs"], store["e_verdict"] = raw_msgs, raw_verdict


def split(stream, lens):
    ends = np.cumsum(lens)
    return [stream[int(e - l):int(e)] for e, l in zip(ends, lens)]


def share(what, flags, of):
    s = float(np.mean(flags)) if len(flags) else 0.0
    print(f"  {what}: {s:.3f} of {of}")
    assert s >= 0.02, f"{what} is at least 2 % of {of}"


with tempfile.TemporaryDirectory() as tmp:
    exe = su.build_ref_harness(tmp)
    ref_lines = {}
    for g, c in sets.items():
        sub = su.in_domain(c)
        for gnss in (0, 1):
            got, lens = su.run_ref_harness(exe, "sbs", sub, use_gnss=gnss, workdir=tmp)
            want = su.sbs_reference(sub["msgs"], sub["fields"], su.NOW_MS, positions=sub["positions"], geom_delta=sub["geom_delta"], use_gnss=bool(gnss))
            assert got == want[0] and (lens == want[1]).all(), f"the Python reference differs from the reference's writer: group {g}, use_gnss {gnss}"
            store[f"ref_sbs_{g}_g{gnss}"] = np.frombuffer(got, dtype=np.uint8)
            ref_lines[g, gnss] = split(got, lens)
    sub = su.in_domain(su.override_cases(sets["b"]))
    for o in su.OVERRIDES:
        got, lens = su.run_ref_harness(exe, "sbs", sub, override_squawk=o, workdir=tmp)
        want = su.sbs_reference(sub["msgs"], sub["fields"], su.NOW_MS, positions=sub["positions"], geom_delta=sub["geom_delta"], override_squawk=o)
        assert got == want[0], f"override squawk {o}"
        store[f"ref_sbs_b_o{o}"] = np.frombuffer(got, dtype=np.uint8)
    carried = np.isin(raw_msgs["msgbits"], (16, 56, 112))
    for mlat in (0, 1):
        for verbatim in (0, 1):
            got, lens = su.run_ref_harness(exe, "raw", raw_msgs[carried], mlat=mlat, verbatim=verbatim, workdir=tmp)
            assert got == su.raw_reference(raw_msgs[carried], mlat=bool(mlat), verbatim=bool(verbatim))[0], f"raw, mlat {mlat} verbatim {verbatim}"
            store[f"ref_raw_m{mlat}v{verbatim}"] = np.frombuffer(got, dtype=np.uint8)
            if mlat:
                text = got.decode()
                assert "@1234567890AB" in text and "@100000000000" in text and "@000000000001" in text and "@FFFFFFFFFFFF" in text and "*" in text

# ---- coverage, on what the reference printed --------------------------------------------------------------------------------------
print("group a:")
lines_a = ref_lines["a", 0]
n_a = len(lines_a)
types = np.array([int(l[4:5]) if l else 0 for l in lines_a])
for t in range(1, 9):
    share(f"msgType {t}", types == t, "group a")
sub = su.in_domain(sets["a"])
f = sub["fields"]
no_line = types == 0
es = np.isin(f["msgtype"], (17, 18))
non_icao = (f["addr"] & su.NON_ICAO) != 0
share("no line: non-ICAO address", no_line & non_icao, "group a")
share("no line: unlisted DF", no_line & ~es & ~non_icao, "group a")
share("no line: ME type outside 1-19", no_line & es & ~non_icao, "group a")
print("groups a + b, of the lines:")
for gnss in (0, 1):
    cols = np.array([l.decode("latin-1").rstrip("\r\n").split(",") for g in ("a", "b") for l in ref_lines[g, gnss]
                     if l and l.count(b",") == 21], dtype=object)
    assert len(cols) > 2000
    names = {10: "callsign", 11: "altitude", 12: "ground speed", 13: "heading", 14: "latitude", 15: "longitude", 16: "vertical rate", 17: "squawk",
             18: "alert", 19: "emergency", 20: "SPI", 21: "on ground"}
    for k, name in names.items():
        present = np.array([c[k] != "" for c in cols])
        share(f"use_gnss {gnss}: {name} present", present, "the lines")
        share(f"use_gnss {gnss}: {name} absent", ~present, "the lines")
    for k in (11, 16):
        h = np.array([c[k].endswith("H") for c in cols])
        plain = np.array([c[k] != "" and not c[k].endswith("H") for c in cols])
        if gnss:
            share(f"use_gnss 1: {names[k]} with H", h, "the lines")
        else:
            assert not h.any()
        share(f"use_gnss {gnss}: {names[k]} without H", plain, "the lines")
# the branches behind the altitude's forms: geometric as stored, barometric + geom_delta (H); geometric - geom_delta (plain)
subs = su.concat_cases([su.in_domain(sets["a"]), su.in_domain(sets["b"])])
printed = np.array([bool(l) for g in ("a", "b") for l in ref_lines[g, 0]])
fl, dv = subs["fields"]["flags"], subs["geom_delta"] != su.INT32_MIN
baro, geom = (fl & su.F_BARO_ALT) != 0, (fl & su.F_GEOM_ALT) != 0
share("altitude: geometric as stored", (printed & geom)[printed], "the lines")
share("altitude: barometric + geom_delta", (printed & ~geom & baro & dv)[printed], "the lines")
share("altitude: geometric - geom_delta", (printed & ~baro & geom & dv)[printed], "the lines")
share("altitude: geometric without geom_delta", (printed & ~baro & geom & ~dv)[printed], "the lines")
br, gr = (fl & su.F_BARO_RATE) != 0, (fl & su.F_GEOM_RATE) != 0
share("rate: both", (printed & br & gr)[printed], "the lines")
share("rate: geometric only", (printed & ~br & gr)[printed], "the lines")
share("rate: barometric only", (printed & br & ~gr)[printed], "the lines")

# the library's rules on top of the writers: which records get a line (a stream is then the reference's lines of exactly those), and the raw streams
for g in su.GROUPS:
    store[f"cls_{g}"] = su.sbs_classes(sets[g]["fields"], sets[g]["msgs"]["sysTimestamp"], sets[g]["positions"], sets[g]["verdict"])[0]
for name, stream in su.raw_expectations(raw_msgs, raw_verdict).items():
    store["want_" + name] = np.frombuffer(stream, dtype=np.uint8)
# a stream that equals one already stored (group c and d print the same with either use_gnss, and every record of them is due) is stored once
seen, aliases = {}, []
for name in sorted(k for k in store if k.startswith(("ref_", "want_"))):
    data = store[name].tobytes()
    if data in seen:
        aliases.append(f"{name}={seen[data]}")
        del store[name]
    else:
        seen[data] = name
store["aliases"] = np.array(aliases)
np.savez_compressed(su.GOLDEN, **store)
print(su.GOLDEN, {g: len(c["msgs"]) for g, c in sets.items()}, len(raw_msgs), "raw cases,", os.path.getsize(su.GOLDEN), "bytes")
assert os.path.getsize(su.GOLDEN) < 1000000
