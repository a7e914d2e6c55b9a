"""Writes tests/golden/pf_in_cases.npz: the streams of tests/pf_in_util.py's case groups and, per stream and configuration, what the
REFERENCE's readPlanefinder + decodePfMessage left for them (tests/host_stub/pf_in_ref_harness.c, which includes the reference's
net_io.c and runs its decodeModesMessage, CRC tables and ICAO filter): the counts and counters, a class and an offset per handler call,
the handler call and mm->signalLevel of every message that was used, the messages' members as struct mgpu_msg.  Group d2 is run behind
group d against the same filter.  The file holds inputs and the reference's recorded results only.  Needs the reference's objects
(`__graft_entry__.build()` where the reference tree exists).
Asserts, with tests/host_stub/pf_in_format_check.cpp, that the framer, the parser and the sequential walk reproduce every record; that
only group p reads past the end; and that the groups hold what they are for.
    python tests/golden/make_pf_in_golden.py"""
import os
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import pf_in_util as pu  # noqa: E402
import helpers  # noqa: E402


def build_check(tmp, extra=("-O2",), name="pf_in_format_check"):
    exe = os.path.join(tmp, name)
    csrc = os.path.join(helpers.ROOT, "readsb_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-g", "-Wall", "-Werror", "-ffp-contract=off", *extra, "-I" + os.path.join(helpers.ROOT, "include"), "-I" + csrc,
                    os.path.join(helpers.ROOT, "tests", "host_stub", "pf_in_format_check.cpp"), os.path.join(csrc, "pf_in_host.cpp"), os.path.join(csrc, "raw_in_host.cpp"),
                    os.path.join(csrc, "tables.cpp"), "-o", exe, "-lm"], check=True)
    return exe


def run_check(exe, stream, cfg, ops, res, tmp):
    """The sequential walk over a stream, compared by the program with the reference's results."""
    names = ("chk_stream.bin", "chk_filter.bin", "chk_head.bin", "chk_class.bin", "chk_off.bin", "chk_frame_of.bin", "chk_signal.bin", "chk_msgs.bin")
    paths = [os.path.join(tmp, n) for n in names]
    open(paths[0], "wb").write(stream)
    np.asarray(list(ops), dtype=np.int32).tofile(paths[1])
    np.asarray(res["head"], dtype=np.uint64).tofile(paths[2])
    np.asarray(res["cls"], dtype=np.uint8).tofile(paths[3])
    np.asarray(res["off"], dtype=np.uint64).tofile(paths[4])
    np.asarray(res["frame_of"], dtype=np.uint64).tofile(paths[5])
    np.asarray(res["signal"], dtype=np.float64).tofile(paths[6])
    np.asarray(res["msgs"]).tofile(paths[7])
    r = subprocess.run([exe, paths[0], str(pu.NOW_MS), *[str(x) for x in cfg], *paths[1:]], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok ") and "runtime error" not in r.stderr, (cfg, r.stdout[-2000:] + r.stderr[-4000:])
    return r.stdout


def run_prefixes(exe, stream, cfg, tmp):
    path = os.path.join(tmp, "chk_prefix_stream.bin")
    open(path, "wb").write(stream)
    r = subprocess.run([exe, "prefixes", path, str(pu.NOW_MS), *[str(x) for x in cfg]], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("ok prefixes") and "runtime error" not in r.stderr, (cfg, r.stdout[-2000:] + r.stderr[-4000:])
    return r.stdout


def main():
    assert pu.have_ref_full(), "needs oracle/_ref/full (run __graft_entry__.build() where the reference tree exists)"
    groups = pu.build_groups()
    out = {}
    res_of = {}
    past_of = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = pu.build_ref_harness(tmp)
        chk = build_check(tmp)
        for g, parts in groups.items():
            stream = pu.stream_of(parts)
            out[g + "_stream"] = np.frombuffer(stream, dtype=np.uint8)
            for cfg in pu.CONFIGS[g]:
                if g == "d2":
                    res = pu.run_ref_harness(exe, [pu.stream_of(groups["d"]), stream], cfg, tmp, ops=pu.ops_of(g))[1]
                else:
                    res = pu.run_ref_harness(exe, [stream], cfg, tmp, ops=pu.ops_of(g))[0]
                k = pu.key(g, cfg)
                res_of[k] = res
                if g != "d2":
                    line = run_check(chk, stream, cfg, pu.ops_of(g), res, tmp).strip()
                    past_of[k] = int(line.split()[8])
                    print(k, line, "bytes", len(stream))
                out[k + "_head"] = res["head"]
                out[k + "_class"] = res["cls"]
                out[k + "_off"] = np.diff(res["off"].astype(np.int64), prepend=0).astype(np.uint16)          # (stored as steps: cumsum gives them back)
                out[k + "_frame_of"] = np.diff(res["frame_of"].astype(np.int64), prepend=0).astype(np.uint16)
                out[k + "_signal"] = res["signal"]
                out[k + "_msgs"] = res["msgs"].view(np.uint8).reshape(-1, 64)
    # what the groups are for
    assert all((v != 0) == k.startswith("p_") for k, v in past_of.items()), past_of
    a0, a1 = res_of[pu.key("a", (1, 1, 0))], res_of[pu.key("a", (1, 1, 1))]
    assert set(a1["cls"].tolist()) >= {pu.MODEAC, pu.BAD, pu.ACCEPT, pu.UNKNOWN, pu.TYPE} and pu.MODEAC_OFF in a0["cls"] and pu.MODEAC not in a0["cls"]
    assert pu.MODEAC_OFF not in a1["cls"] and int(a0["head"][0]) < len(out["a_stream"])                # an incomplete frame at the end
    b = res_of[pu.key("b", (2, 1, 0))]
    assert int(b["head"][8]) > 0 and int(b["head"][9]) > 0 and int(b["head"][5]) > 0 and int(b["head"][6]) > 0
    d_parts, lstar, second, probes = pu.group_d_info()
    d = res_of[pu.key("d", (1, 1, 0))]
    for frame, addr, passes in probes:
        assert (d["cls"][frame] == pu.ACCEPT) == passes, (frame, hex(addr), passes)
    assert any(not p for f, a, p in probes if f > lstar and a in set(int(x) for x in pu.ru.D_INACTIVE))
    np.savez_compressed(pu.GOLDEN, **out)
    print("wrote", pu.GOLDEN, os.path.getsize(pu.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
