"""Writes tests/golden/uat_cases.npz: the streams of tests/uat_util.py's case groups and, per stream, the bytes the REFERENCE's
uat2esnt printed for them (tests/host_stub/uat_ref_harness.c, linked against oracle/_ref/full's two uat2esnt objects) with the length
per line.  The file holds inputs and the reference's recorded bytes only.  Needs the reference's objects (`__graft_entry__.build()`
where the reference tree exists).  Asserts on the reference's output that every frame kind (type codes 0, 8, 18, 22, 19 with subtypes
1 and 2, 1-4, 28), every CF value and both IMF values appear in at least five cases; and, with tests/host_stub/uat_format_check.cpp,
that no case is short and that exactly the cases of group (f) are deferred.
    python tests/golden/make_uat_golden.py"""
import collections
import os
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import uat_util as uu  # noqa: E402
import helpers  # noqa: E402


def kinds(frames):
    """Per frame: its kind, its CF, its IMF (by the place the kind keeps it)."""
    out = []
    for f in frames:
        me = int.from_bytes(bytes(f[4:11]), "big")
        bit = lambda k: (me >> (56 - k)) & 1                                                      # noqa: E731
        tc, sub = me >> 51, (me >> 48) & 7
        kind = "tc19/%d" % sub if tc == 19 else "tc%d" % tc
        imf = bit(21) if tc == 8 else bit(9) if tc == 19 else bit(56) if tc == 28 else bit(8) if tc in (0, 18, 22) else 0
        out.append((kind, int(f[0]) & 7, imf))
    return out


def build_check(tmp):
    exe = os.path.join(tmp, "uat_format_check")
    csrc = os.path.join(helpers.ROOT, "readsb_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-I" + os.path.join(helpers.ROOT, "include"), "-I" + csrc,
                    os.path.join(helpers.ROOT, "tests", "host_stub", "uat_format_check.cpp"), os.path.join(csrc, "uat_host.cpp"), "-o", exe, "-lm"], check=True)
    return exe


def run_check(exe, stream, out, lens, tmp):
    """-> (lines, frames, short lines, the deferred indices) by the formatter, which the program has compared with the reference's bytes"""
    paths = [os.path.join(tmp, n) for n in ("chk_stream.bin", "chk_want.bin", "chk_lens.bin")]
    open(paths[0], "wb").write(stream)
    open(paths[1], "wb").write(out)
    np.asarray(lens, dtype=np.int32).tofile(paths[2])
    r = subprocess.run([exe, *paths], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok ") and "runtime error" not in r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    w = r.stdout.split()
    return int(w[1]), int(w[3]), int(w[5]), [int(x) for x in w[7:]]


def main():
    assert uu.have_ref_objs(), "needs oracle/_ref/full (run __graft_entry__.build() where the reference tree exists)"
    groups = uu.build_groups()
    out = {}
    count = collections.Counter()
    with tempfile.TemporaryDirectory() as tmp:
        exe = uu.build_ref_harness(tmp)
        chk = build_check(tmp)
        for g, lines in groups.items():
            stream = uu.stream_of(lines)
            assert stream.count(b"\n") == len(lines)
            ref, lens = uu.run_ref_harness(exe, stream, tmp)
            assert len(lens) == len(lines) and int(lens.sum()) == len(ref) and (lens % uu.FRAME_TEXT == 0).all() and lens.max() <= 4 * uu.FRAME_TEXT
            nlines, nframes, nshort, deferred = run_check(chk, stream, ref, lens, tmp)
            assert nshort == 0, (g, nshort)
            assert deferred == (list(range(len(lines))) if g == "f" else []), (g, deferred)
            _, frames = uu.frames_of(ref)
            at = 0
            for n in lens // uu.FRAME_TEXT:                                                       # per case: each kind, CF and IMF once
                ks = kinds(frames[at: at + n])
                at += n
                count.update({("kind", k) for k, _, _ in ks} | {("cf", c) for _, c, _ in ks} | {("imf", i) for _, _, i in ks})
            out[g + "_stream"], out[g + "_out"], out[g + "_lens"] = np.frombuffer(stream, dtype=np.uint8), np.frombuffer(ref, dtype=np.uint8), lens.astype(np.int16)
            print(g, len(lines), "cases", len(stream), "bytes in", len(ref), "bytes out")
    need = [("kind", k) for k in ("tc0", "tc8", "tc18", "tc22", "tc19/1", "tc19/2", "tc1", "tc2", "tc3", "tc4", "tc28")] + [("cf", c) for c in (1, 2, 6)] + [("imf", i) for i in (0, 1)]
    rare = [(k, count[k]) for k in need if count[k] < 5]
    assert not rare, rare
    print(sorted(count.items()))
    np.savez_compressed(uu.GOLDEN, **out)
    size = os.path.getsize(uu.GOLDEN)
    print(uu.GOLDEN, size, "bytes")
    assert size < 895000


if __name__ == "__main__":
    main()
