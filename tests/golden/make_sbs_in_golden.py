"""Writes tests/golden/sbs_in_cases.npz: the streams of tests/sbs_in_util.py's case groups and, per stream and source, what the
REFERENCE's readAscii + decodeSbsLine left for them (tests/host_stub/sbs_in_ref_harness.c, which includes the reference's net_io.c):
the five counts, the source line of every message, the messages' members as struct mgpu_sbs_rec.  The file holds inputs and the
reference's recorded results only.  Needs the reference's objects (`__graft_entry__.build()` where the reference tree exists).
Asserts, with tests/host_stub/sbs_in_format_check.cpp, that the parser reproduces every record, that nothing in groups (a) and (b)
is deferred and everything in group (c) is; and on the reference's records that every flag and every enumerated value appears.
    python tests/golden/make_sbs_in_golden.py"""
import os
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import sbs_in_util as su  # noqa: E402
import helpers  # noqa: E402


def build_check(tmp, extra=("-O2",), name="sbs_in_format_check"):
    exe = os.path.join(tmp, name)
    csrc = os.path.join(helpers.ROOT, "readsb_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-g", "-Wall", "-Werror", "-ffp-contract=off", *extra, "-I" + os.path.join(helpers.ROOT, "include"), "-I" + csrc,
                    os.path.join(helpers.ROOT, "tests", "host_stub", "sbs_in_format_check.cpp"), os.path.join(csrc, "sbs_in_host.cpp"), "-o", exe, "-lm"], check=True)
    return exe


def run_check(exe, stream, source, line_of, recs, tmp):
    """-> (lines, plain records, invalid lines, consumed, the deferred indices) by the parser, which the program has compared with the
    reference's records"""
    paths = [os.path.join(tmp, n) for n in ("chk_stream.bin", "chk_line_of.bin", "chk_recs.bin")]
    open(paths[0], "wb").write(stream)
    np.asarray(line_of, dtype=np.uint64).tofile(paths[1])
    np.asarray(recs).tofile(paths[2])
    r = subprocess.run([exe, paths[0], str(su.SOURCES[source]), str(su.NOW_MS), paths[1], paths[2]], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok ") and "runtime error" not in r.stderr, (source, r.stdout[-2000:] + r.stderr[-4000:])
    w = r.stdout.split()
    return int(w[2]), int(w[4]), int(w[6]), int(w[8]), [int(x) for x in w[10:]]


def main():
    assert su.have_ref_full(), "needs oracle/_ref/full (run __graft_entry__.build() where the reference tree exists)"
    groups = su.build_groups()
    out = {}
    seen = []
    with tempfile.TemporaryDirectory() as tmp:
        exe = su.build_ref_harness(tmp)
        chk = build_check(tmp)
        for g, lines in groups.items():
            stream = su.stream_of(lines)
            out[g + "_stream"] = np.frombuffer(stream, dtype=np.uint8)
            for s in su.GROUP_SOURCES[g]:
                head, line_of, recs = su.run_ref_harness(exe, stream, s, tmp)
                nlines = len(su.split_lines(stream))
                assert int(head[0]) == len(stream) and int(head[1]) == nlines and int(head[2]) == int(head[4]) == len(recs), (g, s, head)
                got_lines, nplain, ninvalid, consumed, deferred = run_check(chk, stream, s, line_of, recs, tmp)
                assert (got_lines, ninvalid, consumed) == (nlines, int(head[3]), len(stream)), (g, s, got_lines, ninvalid, head)
                if g == "c":
                    assert nplain == 0 and len(deferred) == len(recs) == len(lines), (g, s, nplain, len(deferred), len(recs))
                else:
                    assert deferred == [] and nplain == len(recs), (g, s, deferred)
                out[f"{g}_{s}_head"], out[f"{g}_{s}_line_of"], out[f"{g}_{s}_recs"] = head, line_of.astype(np.uint32), recs.view(np.uint8)
                seen.append(recs)
                print(g, s, nlines, "lines", len(recs), "records", int(head[3]), "invalid", len(deferred), "deferred")
    r = np.concatenate(seen)
    for bit in (0, 2, 3, 6, 8, 9, 14, 15, 16, 17):                                                # the MGPU_F_* bits the record uses, set and clear
        assert ((r["flags"] >> bit) & 1).sum() >= 5 and ((~r["flags"] >> bit) & 1).sum() >= 5, bit
    for bit in (0, 1, 2):
        assert ((r["sbs_flags"] >> bit) & 1).sum() >= 5, bit
    assert set(r["airground"]) == {0, 1, 2} and set(r["addrtype"]) == {4, 5, 6} and set(r["source"]) == {3, 4, 6, 11} and set(r["sbsMsgType"]) == set(range(10))
    assert (r["receiverCountMlat"] > 0).sum() >= 5 and (r["mlatEPU"] == 65535).sum() >= 1 and (r["reserved"] == 0).all() and (r["baro_alt_unit"] == 0).all()
    np.savez_compressed(su.GOLDEN, **out)
    size = os.path.getsize(su.GOLDEN)
    print(su.GOLDEN, size, "bytes")
    assert size < 400000


if __name__ == "__main__":
    main()
