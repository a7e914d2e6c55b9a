"""Writes tests/golden/raw_in_cases.npz: the streams of tests/raw_in_util.py's case groups and, per stream and configuration, what
the REFERENCE's readAscii + processHexMessage left for them (tests/host_stub/raw_in_ref_harness.c, which includes the reference's
net_io.c and runs its decodeModesMessage, CRC tables and ICAO filter): the counts and counters, a class per line, the source line
and mm->signalLevel of every message that was used, the messages' members as struct mgpu_msg.  Group d2 is run behind group d against
the same filter.  The file holds inputs and the reference's recorded results only.  Needs the reference's objects
(`__graft_entry__.build()` where the reference tree exists).
Asserts, with tests/host_stub/raw_in_format_check.cpp, that the parser and the sequential resolver reproduce every record; that the
groups hold what they are for (every class under every configuration, every DF, repaired frames, the Aerobits forms); and for group
(d) that the reference accepts frames of inactive-generation addresses in front of the first growth and rejects them behind it.
    python tests/golden/make_raw_in_golden.py"""
import os
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import raw_in_util as ru  # noqa: E402
import helpers  # noqa: E402


def build_check(tmp, extra=("-O2",), name="raw_in_format_check", src="raw_in_format_check.cpp"):
    exe = os.path.join(tmp, name)
    csrc = os.path.join(helpers.ROOT, "readsb_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-g", "-Wall", "-Werror", "-ffp-contract=off", *extra, "-I" + os.path.join(helpers.ROOT, "include"), "-I" + csrc,
                    os.path.join(helpers.ROOT, "tests", "host_stub", src), os.path.join(csrc, "raw_in_host.cpp"), os.path.join(csrc, "tables.cpp"), "-o", exe, "-lm"],
                   check=True)
    return exe


def run_check(exe, stream, cfg, ops, res, tmp):
    """The parser and the sequential resolver over a stream, compared by the program with the reference's results."""
    names = ("chk_stream.bin", "chk_filter.bin", "chk_head.bin", "chk_class.bin", "chk_line_of.bin", "chk_signal.bin", "chk_msgs.bin")
    paths = [os.path.join(tmp, n) for n in names]
    open(paths[0], "wb").write(stream)
    np.asarray(list(ops), dtype=np.int32).tofile(paths[1])
    np.asarray(res["head"], dtype=np.uint64).tofile(paths[2])
    np.asarray(res["cls"], dtype=np.uint8).tofile(paths[3])
    np.asarray(res["line_of"], dtype=np.uint64).tofile(paths[4])
    np.asarray(res["signal"], dtype=np.float64).tofile(paths[5])
    np.asarray(res["msgs"]).tofile(paths[6])
    r = subprocess.run([exe, paths[0], str(ru.NOW_MS), str(cfg[0]), str(cfg[1]), str(cfg[2]), *paths[1:]], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok ") and "runtime error" not in r.stderr, (cfg, r.stdout[-2000:] + r.stderr[-4000:])
    return r.stdout


def main():
    assert ru.have_ref_full(), "needs oracle/_ref/full (run __graft_entry__.build() where the reference tree exists)"
    groups = ru.build_groups()
    out = {}
    res_of = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = ru.build_ref_harness(tmp)
        chk = build_check(tmp)
        for g, lines in groups.items():
            stream = ru.stream_of(lines)
            out[g + "_stream"] = np.frombuffer(stream, dtype=np.uint8)
            if g != "d2":
                assert 40000 <= len(stream) <= 62000, (g, len(stream))
        for g in ru.CONFIGS:
            if g == "d2":
                continue
            stream = ru.stream_of(groups[g])
            for cfg in ru.CONFIGS[g]:
                streams = [stream] + ([ru.stream_of(groups["d2"])] if g == "d" else [])
                results = ru.run_ref_harness(exe, streams, cfg, tmp, ops=ru.ops_of(g))
                for name, s, res in zip((g, "d2"), streams, results):
                    nlines = len(ru.split_lines(s))
                    assert int(res["head"][0]) == len(s) and int(res["head"][1]) == nlines and len(res["cls"]) == nlines, (name, cfg)
                    if name != "d2":                                              # (the second call starts from the first one's filter: checked on the GPU)
                        print(name, cfg, run_check(chk, s, cfg, ru.ops_of(g), res, tmp).strip(), "counters", res["head"][3:].tolist())
                    k = ru.key(name, cfg)
                    out[k + "_head"], out[k + "_class"], out[k + "_line_of"], out[k + "_signal"], out[k + "_msgs"] = (
                        res["head"], res["cls"], res["line_of"].astype(np.uint32), res["signal"], res["msgs"].view(np.uint8))
                    res_of[k] = res
    # what the groups are for
    for k, res in res_of.items():
        need = {"a": {ru.NONE, ru.ACCEPT, ru.UNKNOWN}, "b": {ru.BAD, ru.ACCEPT, ru.UNKNOWN}, "c": {ru.NONE, ru.ACCEPT, ru.UNKNOWN}, "d": {ru.ACCEPT, ru.UNKNOWN}}[k[0]]
        assert need <= set(res["cls"].tolist()), k
    a0, a1 = res_of[ru.key("a", (1, 1, 0))], res_of[ru.key("a", (1, 1, 1))]
    assert int(a0["head"][4]) == 0 and int(a1["head"][4]) >= 20 and (a1["msgs"]["msgtype"] == 77).sum() == int(a1["head"][4])
    assert (a0["signal"] > 0).sum() >= 50 and len(set(a0["msgs"]["timestamp"].tolist())) >= 30 and (a0["msgs"]["timestamp"] < 0).sum() >= 3
    for cfg in ru.CONFIGS["b"]:
        b = res_of[ru.key("b", cfg)]
        dfs = set(b["msgs"]["msgtype"].tolist())
        assert {0, 4, 5, 11, 16, 17, 18, 20, 21, 24, 31} <= dfs, (cfg, sorted(dfs))
        assert (int(b["head"][8]) > 0) == (cfg[0] >= 1) and (int(b["head"][9]) > 0) == (cfg[0] >= 2), (cfg, b["head"])
    fix_on, fix_off = res_of[ru.key("b", (1, 1, 0))], res_of[ru.key("b", (1, 0, 0))]
    assert int(fix_on["head"][8]) > int(fix_off["head"][8])                      # fixDF17msgtype's repairs count as one corrected bit
    # group (d): the reference accepts frames of inactive-generation addresses in front of L* and rejects them behind it
    lines, lstar, lstar2, probes = ru.group_d()
    d = res_of[ru.key("d", (1, 1, 0))]
    inactive = set(int(x) for x in ru.D_INACTIVE)
    before = [(ln, a) for ln, a, ok in probes if a in inactive and ln < lstar and ok]
    behind = [(ln, a) for ln, a, ok in probes if a in inactive and ln > lstar and not ok]
    assert len(before) >= 20 and len(behind) >= 20 and lstar2 > lstar
    assert all(d["cls"][ln] == ru.ACCEPT for ln, _ in before) and all(d["cls"][ln] == ru.UNKNOWN for ln, _ in behind)
    assert d["cls"][lstar - 1] == ru.ACCEPT and d["cls"][lstar - 2] == ru.ACCEPT and d["cls"][lstar + 1] == ru.UNKNOWN and d["cls"][lstar + 2] == ru.ACCEPT and d["cls"][lstar + 3] == ru.ACCEPT
    for ln, a, ok in probes:                                                     # ... and everywhere what the model of the filter says
        assert d["cls"][ln] == (ru.ACCEPT if ok else ru.UNKNOWN), (ln, hex(a))
    d2 = res_of[ru.key("d2", (1, 1, 0))]
    assert (d2["cls"][: len(ru.D_INACTIVE)] == ru.ACCEPT).sum() == 2 and (d2["cls"][len(ru.D_INACTIVE): -1] == ru.ACCEPT).all() and d2["cls"][-1] == ru.UNKNOWN
    np.savez_compressed(ru.GOLDEN, **out)
    size = os.path.getsize(ru.GOLDEN)
    print(ru.GOLDEN, size, "bytes")
    assert size < 700000


if __name__ == "__main__":
    main()
