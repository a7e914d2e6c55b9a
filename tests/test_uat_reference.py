"""UAT input on the CPU: readsb_amd/csrc/uat_format.h — the formatter the kernels of kernels/uat.inc run — and uat_host.cpp's
mgpu_uat_format_host, compiled for the host and run, in their own process, against the bytes the reference's uat2esnt printed
(tests/golden/uat_cases.npz); the golden file against the live reference where its objects exist."""
import os
import subprocess

import numpy as np
import pytest

import helpers
import uat_util as uu

CSRC = os.path.join(helpers.ROOT, "readsb_amd", "csrc")
CHECK_SRCS = [os.path.join(helpers.ROOT, "tests", "host_stub", "uat_format_check.cpp"), os.path.join(CSRC, "uat_host.cpp")]
INCLUDES = ["-I" + os.path.join(helpers.ROOT, "include"), "-I" + CSRC]


@pytest.fixture(scope="module")
def golden():
    return uu.load_golden()


def _build_check(tmp_path, name, extra):
    exe = tmp_path / name
    subprocess.run(["g++", "-std=c++17", "-g", "-Wall", "-Werror", "-ffp-contract=off", *extra, *INCLUDES, *CHECK_SRCS, "-o", str(exe), "-lm"], check=True)
    return str(exe)


def _run_check(exe, tmp_path, golden):
    """Every group through the program -> {group: (lines, frames, short lines, deferred indices)}"""
    res = {}
    for g in uu.GROUPS:
        stream, out, lens = golden[g]
        paths = [str(tmp_path / name) for name in ("stream.bin", "want.bin", "lens.bin")]
        open(paths[0], "wb").write(stream)
        open(paths[1], "wb").write(out)
        lens.astype(np.int32).tofile(paths[2])
        r = subprocess.run([exe, *paths], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.startswith("ok ") and "runtime error" not in r.stderr, (g, r.stdout[-2000:] + r.stderr[-4000:])
        w = r.stdout.split()
        res[g] = (int(w[1]), int(w[3]), int(w[5]), [int(x) for x in w[7:]])
    return res


def _check(res, golden):
    """The program has compared the bytes; here: every line was seen, no golden case is short, exactly group (f) is deferred."""
    for g in uu.GROUPS:
        stream, out, lens = golden[g]
        nlines, nframes, nshort, deferred = res[g]
        assert nlines == len(lens) == stream.count(b"\n") and nshort == 0, g
        assert deferred == (list(range(nlines)) if g == "f" else []), (g, deferred)
        assert nframes == (0 if g == "f" else len(out) // uu.FRAME_TEXT), g


def test_formatter_equals_the_reference(tmp_path, golden):
    """The counting and the byte emitter agree, the bytes are the reference's for every non-deferred case, the deferred cases are
    exactly group (f) and mgpu_uat_format_host settles them to the reference's bytes; the signal table does not decrease."""
    _check(_run_check(_build_check(tmp_path, "uat_format_check", ["-O2"]), tmp_path, golden), golden)


def test_formatter_under_sanitizers(tmp_path, golden):
    """The same program built with ASan and UBSan, host only, run directly."""
    exe = _build_check(tmp_path, "uat_format_check_san", ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    _check(_run_check(exe, tmp_path, golden), golden)


def test_golden_is_what_the_generators_build(golden):
    """The golden's streams are the seeded generators' (so the groups are what tests/uat_util.py says they are), nothing in it but
    inputs and recorded bytes, every frame 45 bytes."""
    groups = uu.build_groups()
    for g in uu.GROUPS:
        stream, out, lens = golden[g]
        assert stream == uu.stream_of(groups[g]), g
        assert int(lens.sum()) == len(out) and (lens % uu.FRAME_TEXT == 0).all() and lens.max() <= 4 * uu.FRAME_TEXT, g
    assert os.path.getsize(uu.GOLDEN) < 895000


def test_short_lines_give_nothing(tmp_path):
    """The documented departure: a payload shorter than its type's decoders read is counted and gives no frame, at every type's
    boundary; one byte more and the line is taken."""
    exe = _build_check(tmp_path, "uat_format_check", ["-O2"])
    lines, want_short = [], 0
    for t in range(32):
        need = uu.NEEDED[t]
        for nbytes in (0, 1, 3, need - 1):
            lines.append(uu.line(uu.payload(t, 0, nbytes=nbytes)))
            want_short += 1
    stream = b"".join(lines)
    paths = [str(tmp_path / name) for name in ("stream.bin", "want.bin", "lens.bin")]
    open(paths[0], "wb").write(stream)
    open(paths[1], "wb").write(b"")
    np.zeros(len(lines), dtype=np.int32).tofile(paths[2])
    r = subprocess.run([exe, *paths], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    w = r.stdout.split()
    assert (int(w[1]), int(w[3]), int(w[5]), w[7:]) == (len(lines), 0, want_short, [])


@pytest.mark.skipif(not uu.have_ref_objs(), reason="needs the reference objects of oracle/_ref/full")
def test_live_reference_equals_the_golden(tmp_path, golden):
    """tests/host_stub/uat_ref_harness.c, linked against the reference's two objects, prints the golden's bytes; and with exactly
    `need` payload bytes of every type (the least that is not short) the formatter still equals it."""
    exe = uu.build_ref_harness(str(tmp_path))
    for g in uu.GROUPS:
        stream, out, lens = golden[g]
        ref, rlens = uu.run_ref_harness(exe, stream, str(tmp_path))
        assert ref == out and (rlens == lens).all(), g
    lines = [uu.line(uu.payload(t, aq, ag=ag, nbytes=uu.NEEDED[t])) for t in range(32) for aq in (0, 3) for ag in (0, 2)]
    stream = b"".join(lines)
    ref, rlens = uu.run_ref_harness(exe, stream, str(tmp_path))
    chk = _build_check(tmp_path, "uat_format_check", ["-O2"])
    paths = [str(tmp_path / name) for name in ("s.bin", "w.bin", "l.bin")]
    open(paths[0], "wb").write(stream)
    open(paths[1], "wb").write(ref)
    rlens.astype(np.int32).tofile(paths[2])
    r = subprocess.run([chk, *paths], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.split()[5] == "0", r.stdout + r.stderr[-2000:]
