"""CPU: the snip tests' checker (tests/snip_util.py) pinned to the reference program, the per-word mask function the kernels use
(readsb_amd/csrc/snip_mask.h) against the reference's sequential loop under sanitizers, and the entries' place in the C ABI."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import helpers
import snip_util as su


def test_model_is_the_sequential_loop():
    """The closed form against the loop of readsb.c:1196-1205 restated, carries included (no reference binary needed)."""
    for level in su.LEVELS:
        iq = su.crafted(level, 6001)
        for c_in in (0, 1, 31, 32, 33, 34, 1 << 40):
            assert su.model(iq, level, c_in) == su.sequential(iq, level, c_in), (level, c_in)
    iq = su.random_stream(5000, 1 / 33, seed=1)
    assert su.model(iq, 4) == su.sequential(iq, 4)
    assert su.model(b"", 4, 7) == (b"", 7)
    # what the builders promise: both kinds of sample at the levels that have both, the 32/33 boundary on both sides
    q = su.quiet_flags(su.crafted(2), 2)
    assert 0.5 < q.mean() < 0.9 and not q[0]
    assert su.quiet_flags(su.crafted(0), 0).sum() == 0 and su.quiet_flags(su.crafted(129), 129).all()
    assert su.quiet_flags(b"\x00\x7f\xff\x7f\x7f\x7f", 128).tolist() == [True, False, True]         # asymmetric: 0 -> 127, 255 -> 128


@pytest.mark.skipif(not su.have_reference(), reason="needs `make -C oracle full` (the reference program, built where its sources are)")
@pytest.mark.parametrize("level", su.LEVELS)
def test_model_is_the_reference_program(level):
    iq = su.crafted(level)
    want = su.reference_snip(iq, level)
    assert su.model(iq, level)[0] == want
    if level == 2:
        assert su.reference_snip(iq + b"\x7f", level) == want                                      # a trailing odd byte is dropped
        r = su.random_stream(1 << 16, 1 / 33, seed=2)
        assert su.model(r, 4)[0] == su.reference_snip(r, 4)


def test_mask_function_under_sanitizers(tmp_path):
    """tests/host_stub/snip_mask_check.cpp, its own process: snip_keep_word / snip_carry_word / snip_quiet against the sequential loop."""
    exe = tmp_path / "snip_mask_check"
    src = os.path.join(helpers.ROOT, "tests", "host_stub", "snip_mask_check.cpp")
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", src, "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and "runtime error" not in r.stderr, r.stdout[-2000:] + r.stderr[-2000:]


def test_c_abi_without_a_device(tmp_path):
    from readsb_amd import binding
    lib = binding.load_library()
    header = open(os.path.join(helpers.ROOT, "include", "modes_gpu.h")).read()
    for name in ("mgpu_snip", "mgpu_snip_device"):
        assert re.search(r"\bint %s\(mgpu_ctx \*ctx, const struct mgpu_snip_args \*args\);" % name, header), name
        assert hasattr(lib, name), name
    for name in ("snip", "snip_device"):
        assert callable(getattr(binding.Demodulator, name))
    assert "readsb.c:1187-1206" in header
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "modes_gpu.h"\nint main(void){printf("%zu %zu %zu\\n",sizeof(struct mgpu_snip_args),'
                   'offsetof(struct mgpu_snip_args, quiet_run),offsetof(struct mgpu_snip_args, pass_samples));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(helpers.ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(binding.SnipArgs), binding.SnipArgs.quiet_run.offset, binding.SnipArgs.pass_samples.offset]
    assert int(re.search(r"#define MGPU_ABI_VERSION (\d+)", header).group(1)) == 6 == binding.ABI_VERSION      # no struct that existed changed
    nout = C.c_uint64(0)
    iq, out = np.zeros(16, dtype=np.uint8), np.zeros(16, dtype=np.uint8)
    good = binding.SnipArgs(C.sizeof(binding.SnipArgs), 4, iq.ctypes.data, 8, out.ctypes.data, 8, C.pointer(nout), None, 0)
    short = binding.SnipArgs(C.sizeof(binding.SnipArgs) - 8, 4, iq.ctypes.data, 8, out.ctypes.data, 8, C.pointer(nout), None, 0)
    no_nout = binding.SnipArgs(C.sizeof(binding.SnipArgs), 4, iq.ctypes.data, 8, out.ctypes.data, 8, None, None, 0)
    not_a_ctx = C.create_string_buffer(64)                  # the argument checks come before anything looks at the context
    for f in (lib.mgpu_snip, lib.mgpu_snip_device):
        f.restype = C.c_int
        assert f(None, C.byref(good)) == su.MGPU_E_INVAL
        assert f(not_a_ctx, None) == su.MGPU_E_INVAL
        assert f(not_a_ctx, C.byref(short)) == su.MGPU_E_INVAL
        assert f(not_a_ctx, C.byref(no_nout)) == su.MGPU_E_INVAL
    assert not out.any() and nout.value == 0


def test_command_line_on_the_standin_has_no_snip(tmp_path):
    """readsb_gpu_ifile built against the stand-in library (no mgpu_snip, so without snip_gpu.c) still links, and says what it lacks."""
    host = os.path.join(helpers.ROOT, "readsb_amd", "host")
    exe = str(tmp_path / "readsb_gpu_ifile_standin")
    subprocess.run(["gcc", "-std=gnu11", "-O1", "-Wall", "-ffp-contract=off", "-o", exe, os.path.join(host, "readsb_gpu_ifile.c"),
                    os.path.join(host, "demod_gpu.c"), os.path.join(helpers.ROOT, "tests", "host_stub", "modes_gpu_standin.c"),
                    os.path.join(helpers.ORACLE_DIR, "modes_oracle.c"), os.path.join(helpers.ORACLE_DIR, "modes_oracle_fields.c"),
                    "-lpthread", "-lm"], check=True)
    r = subprocess.run([exe, "--snip", "4"], input=b"\x7f\x7f", capture_output=True, timeout=60)
    assert r.returncode == 2 and b"--snip: this build has no GPU chain" in r.stderr and r.stdout == b""
