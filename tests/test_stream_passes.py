"""The host forms' pass driver on the CPU: readsb_amd/csrc/stream_passes.h — the one loop that cuts a stream into passes for
mgpu_uat_encode, mgpu_sbs_decode, mgpu_raw_decode, mgpu_beast_decode, mgpu_asterix_decode and the beast input's sequential walk —
driven by tests/host_stub/stream_passes_check.cpp with a format made up there: texts without a newline, of newlines only, ending with
and without one, with one line longer than all the rest together, with 300 random line lengths 0..300, each at pass sizes 0, 1, 2, 3,
7, 255, 256, len - 1, len, len + 1.  The program asserts the totals and `consumed` of one call over the whole text, contiguous
committed stretches, exactly one undo before each repeat and none otherwise, at most floor(log2(len)) + 1 repeats, how each policy
ends (the line formats' pass over the tail alone; the stream's end; a stop in the middle, with nothing run behind it).  Built with
-Wall -Werror, plain and under ASan + UBSan, and run in its own process."""
import os
import subprocess

import pytest

import helpers

CSRC = os.path.join(helpers.ROOT, "readsb_amd", "csrc")
CHECK = os.path.join(helpers.ROOT, "tests", "host_stub", "stream_passes_check.cpp")


@pytest.mark.parametrize("name,extra", [("plain", ("-O2",)), ("san", ("-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"))])
def test_the_pass_driver_over_a_made_up_format(tmp_path, name, extra):
    exe = str(tmp_path / f"stream_passes_check_{name}")
    subprocess.run(["g++", "-std=c++17", "-g", "-Wall", "-Werror", *extra, "-I" + CSRC, CHECK, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok ") and "runtime error" not in r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    assert int(r.stdout.split()[1]) >= 150                      # texts x pass sizes x policies: none was skipped
