"""Writes tests/golden/beast_in_cases.npz: the streams of tests/beast_in_util.py's case groups and, per stream and configuration, what
the REFERENCE's readBeast + decodeBinMessage left for them (tests/host_stub/beast_in_ref_harness.c, which includes the reference's
net_io.c and runs its decodeModesMessage, CRC tables and ICAO filter): the counts and counters, a class and an offset per handler
call, the handler call, receiver id and mm->signalLevel of every message that was used, the messages' members as struct mgpu_msg.
Group d2 is run behind group d against the same filter.  The file holds inputs and the reference's recorded results only.  Needs the
reference's objects (`__graft_entry__.build()` where the reference tree exists).
Asserts, with tests/host_stub/beast_in_format_check.cpp, that the framer, the parser and the sequential walk reproduce every record; that
no stream has a stop on its chain (the reference would close the client or read a UUID); and that the groups hold what they are for.
    python tests/golden/make_beast_in_golden.py"""
import os
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import beast_in_util as bu  # noqa: E402
import helpers  # noqa: E402


def build_check(tmp, extra=("-O2",), name="beast_in_format_check"):
    exe = os.path.join(tmp, name)
    csrc = os.path.join(helpers.ROOT, "readsb_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-g", "-Wall", "-Werror", "-ffp-contract=off", *extra, "-I" + os.path.join(helpers.ROOT, "include"), "-I" + csrc,
                    os.path.join(helpers.ROOT, "tests", "host_stub", "beast_in_format_check.cpp"), os.path.join(csrc, "beast_in_host.cpp"), os.path.join(csrc, "raw_in_host.cpp"),
                    os.path.join(csrc, "tables.cpp"), "-o", exe, "-lm"], check=True)
    return exe


def run_check(exe, stream, cfg, ops, res, tmp, id_in=bu.ID_IN):
    """The sequential walk over a stream, compared by the program with the reference's results."""
    names = ("chk_stream.bin", "chk_filter.bin", "chk_head.bin", "chk_class.bin", "chk_off.bin", "chk_frame_of.bin", "chk_ids.bin", "chk_signal.bin", "chk_msgs.bin")
    paths = [os.path.join(tmp, n) for n in names]
    open(paths[0], "wb").write(stream)
    np.asarray(list(ops), dtype=np.int32).tofile(paths[1])
    np.asarray(res["head"], dtype=np.uint64).tofile(paths[2])
    np.asarray(res["cls"], dtype=np.uint8).tofile(paths[3])
    np.asarray(res["off"], dtype=np.uint64).tofile(paths[4])
    np.asarray(res["frame_of"], dtype=np.uint64).tofile(paths[5])
    np.asarray(res["ids"], dtype=np.uint64).tofile(paths[6])
    np.asarray(res["signal"], dtype=np.float64).tofile(paths[7])
    np.asarray(res["msgs"]).tofile(paths[8])
    r = subprocess.run([exe, paths[0], str(bu.NOW_MS), *[str(x) for x in cfg], str(id_in), *paths[1:]], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok ") and "runtime error" not in r.stderr, (cfg, r.stdout[-2000:] + r.stderr[-4000:])
    return r.stdout


def run_prefixes(exe, stream, cfg, tmp):
    path = os.path.join(tmp, "chk_prefix_stream.bin")
    open(path, "wb").write(stream)
    r = subprocess.run([exe, "prefixes", path, str(bu.NOW_MS), *[str(x) for x in cfg]], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("ok prefixes") and "runtime error" not in r.stderr, (cfg, r.stdout[-2000:] + r.stderr[-4000:])
    return r.stdout


def main():
    assert bu.have_ref_full(), "needs oracle/_ref/full (run __graft_entry__.build() where the reference tree exists)"
    from readsb_amd import binding
    lib = binding.load_library()
    groups = bu.build_groups()
    out = {}
    res_of = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = bu.build_ref_harness(tmp)
        chk = build_check(tmp)
        for g, parts in groups.items():
            stream = bu.stream_of(parts)
            out[g + "_stream"] = np.frombuffer(stream, dtype=np.uint8)
            for cfg in bu.CONFIGS[g]:
                assert bu.walk_host(lib, stream, cfg)["stop"] == bu.STOP_END, (g, cfg, "a stop on the chain")
                if g == "d2":
                    res = bu.run_ref_harness(exe, [bu.stream_of(groups["d"]), stream], cfg, tmp, ops=bu.ops_of(g))[1]
                elif g != "d2":
                    res = bu.run_ref_harness(exe, [stream], cfg, tmp, ops=bu.ops_of(g))[0]
                k = bu.key(g, cfg)
                res_of[k] = res
                if g != "d2":
                    print(k, run_check(chk, stream, cfg, bu.ops_of(g), res, tmp).strip(), "bytes", len(stream), "garbage", int(res["head"][10]))
                out[k + "_head"] = res["head"]
                out[k + "_class"] = res["cls"]
                out[k + "_off"] = np.diff(res["off"].astype(np.int64), prepend=0).astype(np.uint16)          # (stored as steps: cumsum gives them back)
                out[k + "_frame_of"] = np.diff(res["frame_of"].astype(np.int64), prepend=0).astype(np.uint16)
                out[k + "_ids"] = res["ids"]
                out[k + "_signal"] = res["signal"]
                out[k + "_msgs"] = res["msgs"].view(np.uint8).reshape(-1, 64)
    # what the groups are for
    a0, a1 = res_of[bu.key("a", (1, 1, 0, 0))], res_of[bu.key("a", (1, 1, 1, 0))]
    assert set(a1["cls"].tolist()) >= {bu.MODEAC, bu.BAD, bu.ACCEPT, bu.POSITION, bu.PONG} and bu.MODEAC_OFF in a0["cls"] and bu.MODEAC not in a0["cls"]
    assert int(a0["head"][10]) > 1000 and int(a0["head"][0]) < len(out["a_stream"])                  # garbage; an incomplete frame at the end
    assert len(set(a0["ids"].tolist())) > 20
    b = res_of[bu.key("b", (2, 1, 0, 0))]
    assert int(b["head"][8]) > 0 and int(b["head"][9]) > 0 and int(b["head"][5]) > 0 and int(b["head"][6]) > 0
    e0, e1 = res_of[bu.key("e", (1, 1, 1, 0))], res_of[bu.key("e", (1, 1, 1, 1))]
    assert len(set(e0["ids"].tolist())) > 20 and set(e1["ids"].tolist()) == {bu.ID_IN} and int(e1["head"][11]) == bu.ID_IN
    d_parts, lstar, second, probes = bu.group_d_info()
    d = res_of[bu.key("d", (1, 1, 0, 0))]
    for frame, addr, passes in probes:
        assert (d["cls"][frame] == bu.ACCEPT) == passes, (frame, hex(addr), passes)
    assert any(not p for f, a, p in probes if f > lstar and a in set(int(x) for x in bu.ru.D_INACTIVE))
    np.savez_compressed(bu.GOLDEN, **out)
    print("wrote", bu.GOLDEN, os.path.getsize(bu.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
