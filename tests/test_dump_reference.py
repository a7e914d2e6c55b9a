"""The message dump on the CPU: readsb_amd/csrc/dump_format.h — the formatter the kernels of kernels/dump.inc run — compiled for the
host and run, in its own process, against the bytes the reference's displayModesMessage printed (tests/golden/dump_cases.npz); the
golden file against the live reference where its tree and the full build exist; the rules about who gets a dump."""
import os
import subprocess

import numpy as np
import pytest

import dump_util as du
import helpers

CHECK_SRC = os.path.join(helpers.ROOT, "tests", "host_stub", "dump_format_check.cpp")
INCLUDES = ["-I" + os.path.join(helpers.ROOT, "include"), "-I" + os.path.join(helpers.ROOT, "readsb_amd", "csrc")]


@pytest.fixture(scope="module")
def golden():
    return du.load_golden()


def _build_check(tmp_path, name, extra):
    exe = tmp_path / name
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *extra, *INCLUDES, CHECK_SRC, "-o", str(exe), "-lm"], check=True)
    return str(exe)


def _run_check(exe, tmp_path, golden, show=None):
    """Every group in every mode through the program -> {(group, mode): the indices it says the device defers}"""
    sets, ref, _ = golden
    deferred = {}
    for g in du.GROUPS:
        for mode, flags in du.MODES.items():
            stream, lens = ref[(g, mode)]
            paths = [str(tmp_path / name) for name in ("cases.bin", "want.bin", "lens.bin")]
            du.case_records(sets[g], flags).tofile(paths[0])
            open(paths[1], "wb").write(stream)
            lens.astype(np.int32).tofile(paths[2])
            r = subprocess.run([exe, *paths, str(flags), "0"], capture_output=True, text=True, timeout=120)
            assert r.returncode == 0 and r.stdout.startswith("ok ") and "runtime error" not in r.stderr, (g, mode, r.stdout[-2000:] + r.stderr[-4000:])
            words = r.stdout.split()
            assert int(words[1]) == int((lens != 0).sum())
            deferred[(g, mode)] = [int(w) for w in words[3:]]
    return deferred


def _check_deferred(deferred, near):
    """Exactly the near cases of group (e), in the full modes only: elsewhere the reference alone stays within "0 deferred"."""
    for (g, mode), idx in deferred.items():
        assert idx == (near.tolist() if g == "e" and mode in ("full", "mlat") else []), (g, mode, idx)


def test_model_equals_the_reference(golden):
    """The plain-Python model (dump_util.model_dump) prints the golden's reference bytes, case by case, in every mode: this runs
    everywhere and pins the model the GPU tests use where no golden exists."""
    sets, ref, _ = golden
    for g in du.GROUPS:
        for mode, flags in du.MODES.items():
            want = du.chunks(*ref[(g, mode)])
            for i, (a, b) in enumerate(zip(du.model_chunks(sets[g], flags), want)):
                assert a == b, (g, mode, i, a, b)


def test_formatter_equals_the_reference(tmp_path, golden):
    """The counting sink and the byte sink agree, and the bytes are the reference's, for every golden case in every mode."""
    _check_deferred(_run_check(_build_check(tmp_path, "dump_format_check", ["-O2"]), tmp_path, golden), golden[2])


def test_formatter_under_sanitizers(tmp_path, golden):
    """The same program built with ASan and UBSan, host only, run directly."""
    exe = _build_check(tmp_path, "dump_format_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    _check_deferred(_run_check(exe, tmp_path, golden), golden[2])


def test_classes_and_golden_agree(golden):
    """The restated rules (dump_util.classes) give a dump exactly where the golden has one; the longest stays within the bound; a
    quiet run keeps the matching addresses only and counts nothing."""
    sets, ref, near = golden
    for g in du.GROUPS:
        for mode, flags in du.MODES.items():
            stream, lens = ref[(g, mode)]
            cls = du.classes(sets[g], flags)
            assert ((cls != du.SKIP) == (lens != 0)).all() and lens.sum() == len(stream) and lens.max() <= du.DUMP_MAX, (g, mode)
            assert np.nonzero(cls == du.DEFER)[0].tolist() == (near.tolist() if g == "e" and mode in ("full", "mlat") else [])
    c = sets["a"]
    addr = int(c["fields"]["addr"][3])
    cls = du.classes(c, du.QUIET, addr)
    assert (cls[c["fields"]["addr"] != addr] == du.NONE).all() and cls[3] != du.NONE
    stream, lens = ref[("a", "full")]
    got, _, skipped, _ = du.expected(c, du.QUIET, du.chunks(stream, lens), addr)
    assert skipped == 0 and got == b"".join(t for t, a in zip(du.chunks(stream, lens), c["fields"]["addr"].tolist()) if a == addr)


@pytest.mark.skipif(not du.have_ref_full(), reason="needs the reference tree and oracle/_ref/full")
def test_live_reference_equals_the_golden(tmp_path, golden):
    """tests/host_stub/dump_ref_harness.c, linked against the reference's objects, prints the golden's bytes; the generators are
    the golden's."""
    sets, ref, near = golden
    groups, near_now = du.build_groups()
    assert near_now.tolist() == near.tolist()
    exe = du.build_ref_harness(str(tmp_path))
    for g in du.GROUPS:
        for k, v in groups[g].items():
            assert v.tobytes() == sets[g][k].tobytes(), (g, k)
        for mode, flags in du.MODES.items():
            stream, lens = du.run_ref_harness(exe, sets[g], flags, str(tmp_path))
            assert stream == ref[(g, mode)][0] and (lens == ref[(g, mode)][1]).all(), (g, mode)


def test_command_line_on_the_standin_has_no_dump(tmp_path):
    """readsb_gpu_ifile built against the stand-in library (no device, so without dump_gpu.c) still links, and says what it lacks."""
    host = os.path.join(helpers.ROOT, "readsb_amd", "host")
    exe = str(tmp_path / "readsb_gpu_ifile_standin")
    subprocess.run(["gcc", "-std=gnu11", "-O1", "-Wall", "-ffp-contract=off", "-o", exe, os.path.join(host, "readsb_gpu_ifile.c"),
                    os.path.join(host, "demod_gpu.c"), os.path.join(helpers.ROOT, "tests", "host_stub", "modes_gpu_standin.c"),
                    os.path.join(helpers.ORACLE_DIR, "modes_oracle.c"), os.path.join(helpers.ORACLE_DIR, "modes_oracle_fields.c"),
                    "-lpthread", "-lm"], check=True)
    r = subprocess.run([exe, "--ifile", "-", "--dump-out", str(tmp_path / "out.txt")], input=b"", capture_output=True, timeout=60)
    assert r.returncode == 2 and b"--dump-out: this build has no GPU chain" in r.stderr and r.stdout == b""


def test_bound_is_stated_once():
    """MGPU_DUMP_MAX of include/modes_gpu.h is the binding's and the checker's DUMP_MAX."""
    import re
    from readsb_amd import binding
    text = open(os.path.join(helpers.ROOT, "include", "modes_gpu.h")).read()
    value = int(re.search(r"^#define MGPU_DUMP_MAX (\d+)", text, flags=re.M).group(1))
    assert value == binding.DUMP_MAX == du.DUMP_MAX
