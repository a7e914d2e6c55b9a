"""CPU: the text outputs' checker (tests/sbs_util.py) pinned to the reference's own writers, and the four entries' place in the C ABI.

tests/golden/text_cases.npz holds what modesSendSBSOutput / modesSendRawOutput printed for the case records (tests/golden/
make_text_golden.py, through tests/host_stub/text_ref_harness.c).  sbs_reference / raw_reference must print the same bytes; where the
full reference build is present the harness is run again and must still print them.  tests/test_gpu_text.py then compares the kernels
with the checker."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import helpers
import sbs_util as su


@pytest.fixture(scope="module")
def golden():
    return su.load_golden()


def _plain(c, **kw):
    """The checker as the reference's writer sees a record: no verdicts."""
    return su.sbs_reference(c["msgs"], c["fields"], su.NOW_MS, positions=c["positions"], geom_delta=c["geom_delta"], **kw)


def test_checker_prints_the_reference_bytes(golden):
    sets, (raw_msgs, _), streams, _ = golden
    for g in su.GROUPS:
        sub = su.in_domain(sets[g])
        assert len(sub["msgs"]) > 0.9 * len(sets[g]["msgs"])
        for gnss in (0, 1):
            assert _plain(sub, use_gnss=bool(gnss))[0] == streams[f"ref_sbs_{g}_g{gnss}"], (g, gnss)
    assert streams["ref_sbs_a_g0"] != streams["ref_sbs_a_g1"] and streams["ref_sbs_b_g0"] != streams["ref_sbs_b_g1"]
    sub = su.in_domain(su.override_cases(sets["b"]))
    for o in su.OVERRIDES:
        assert _plain(sub, override_squawk=o)[0] == streams[f"ref_sbs_b_o{o}"], o
        assert (",%04d," % o).encode() in streams[f"ref_sbs_b_o{o}"]
    carried = raw_msgs[np.isin(raw_msgs["msgbits"], (16, 56, 112))]
    for mlat in (0, 1):
        for verbatim in (0, 1):
            assert su.raw_reference(carried, mlat=bool(mlat), verbatim=bool(verbatim))[0] == streams[f"ref_raw_m{mlat}v{verbatim}"]


def test_known_lines(golden):
    """A DF17 airborne position and a fourteen-digit timestamp, as the reference printed them."""
    c = su._base(1)
    f = c["fields"]
    f["flags"] = su.F_BARO_ALT | su.F_SQUAWK | su.F_GS | su.F_HEADING | su.F_ALERT_VALID | su.F_ALERT
    f["baro_alt"], f["squawkDec"], f["airground"], f["gs_selected"], f["heading"], f["heading_type"] = 38000, 77, 2, 0.5, 359.5, 1
    c["positions"]["method"], c["positions"]["lat"], c["positions"]["lon"] = 1, 52.2572021484375, -3.91937255859375
    assert su.sbs_of(c)[0] == b"MSG,3,1,1,4840D6,1,2023/11/14,22:13:20.999,2023/11/14,22:13:20.123,,38000,0,360,52.257202,-3.919373,,0077,-1,0,,0\r\n"
    m = np.zeros(1, dtype=su.MSG)
    m["timestamp"], m["msgbits"], m["msg"] = 0x1234567890AB5D, 56, 0x5D
    assert su.raw_reference(m, mlat=True)[0] == b"@1234567890AB5D5D5D5D5D5D5D;\n"
    assert su.raw_reference(m)[0] == b"*5D5D5D5D5D5D5D;\n"


def test_line_rules_on_the_reference_lines(golden):
    """With verdicts and the skip rule: a stream is the reference's lines of exactly the records of class LINE, the deferred list names
    the records of class DEFER at the offsets their lines would start at, the skipped count is the class SKIP."""
    sets, _, streams, classes = golden
    for g in su.GROUPS:
        c = sets[g]
        cls, _ = su.sbs_classes(c["fields"], c["msgs"]["sysTimestamp"], c["positions"], c["verdict"])
        assert (cls == classes[g]).all(), g
        plain_cls = su.sbs_classes(c["fields"], c["msgs"]["sysTimestamp"], c["positions"], None)[0]
        keep = plain_cls != su.SKIP
        sub = {k: v[keep] for k, v in c.items()}
        for gnss in (0, 1):
            ref = streams[f"ref_sbs_{g}_g{gnss}"]
            lens = _plain(sub, use_gnss=bool(gnss))[1]
            assert lens.sum() == len(ref)
            ends = np.cumsum(lens)
            due = cls[keep] == su.LINE
            want = b"".join(ref[int(e - l):int(e)] for e, l in zip(ends[due], lens[due]))
            stream, length, deferred, nskipped = su.sbs_of(c, use_gnss=bool(gnss))
            assert stream == want, (g, gnss)
            assert nskipped == int((cls == su.SKIP).sum())
            assert (deferred["index"] == np.nonzero(cls == su.DEFER)[0]).all()
            assert (deferred["offset"] == (np.cumsum(length) - length)[cls == su.DEFER]).all()
    for g, least in (("a", 0.05), ("b", 0.02)):
        for k in (su.NONE, su.LINE, su.DEFER):
            assert (classes[g] == k).mean() >= least, (g, k)
    # edge_cases: 5 stamps outside the range, 6 of its 7 floats on the speed and 6 on the heading, 9 of its 11 positions (method 1)
    assert (classes["b"] == su.SKIP).sum() == 5 + 6 + 6 + 9
    _, (raw_msgs, raw_verdict), streams, _ = golden
    for name, want in su.raw_expectations(raw_msgs, raw_verdict).items():
        assert streams["want_" + name] == want, name


def test_cut_lists(golden):
    """A list cut at 1, 255, 256 and 1000 and concatenated is the one call's stream."""
    sets, (raw_msgs, raw_verdict), _, _ = golden
    c = su.concat_cases([sets["a"], sets["b"]])
    n = len(c["msgs"])
    whole, length, deferred, nskipped = su.sbs_of(c, use_gnss=True)
    for cut in (1, 255, 256, 1000):
        lo = n // 3 if cut == 1 else 0                  # (single records: a stretch of the list)
        hi = lo + 300 if cut == 1 else n
        parts = [su.sbs_of(su.slice_cases(c, k, min(k + cut, hi)), use_gnss=True) for k in range(lo, hi, cut)]
        start = int(length[:lo].sum())
        assert b"".join(p[0] for p in parts) == whole[start:start + int(length[lo:hi].sum())]
        assert sum(len(p[2]) for p in parts) == int(((deferred["index"] >= lo) & (deferred["index"] < hi)).sum())
    for cut in (1, 255, 256, 1000):
        parts = [su.raw_reference(raw_msgs[k:k + cut], True, raw_verdict[k:k + cut], True)[0] for k in range(0, len(raw_msgs), cut)]
        assert b"".join(parts) == su.raw_reference(raw_msgs, True, raw_verdict, True)[0]


@pytest.mark.skipif(not su.have_ref_full(), reason="needs the reference tree and oracle/_ref/full (make -C oracle full)")
def test_fresh_harness_run_prints_the_golden_bytes(golden, tmp_path):
    sets, (raw_msgs, _), streams, _ = golden
    exe = su.build_ref_harness(str(tmp_path))
    for g in su.GROUPS:
        sub = su.in_domain(sets[g])
        for gnss in (0, 1):
            got, lens = su.run_ref_harness(exe, "sbs", sub, use_gnss=gnss, workdir=str(tmp_path))
            assert got == streams[f"ref_sbs_{g}_g{gnss}"], (g, gnss)
            assert (lens == _plain(sub, use_gnss=bool(gnss))[1]).all()
    sub = su.in_domain(su.override_cases(sets["b"]))
    for o in su.OVERRIDES:
        assert su.run_ref_harness(exe, "sbs", sub, override_squawk=o, workdir=str(tmp_path))[0] == streams[f"ref_sbs_b_o{o}"]
    carried = raw_msgs[np.isin(raw_msgs["msgbits"], (16, 56, 112))]
    for mlat in (0, 1):
        for verbatim in (0, 1):
            assert su.run_ref_harness(exe, "raw", carried, mlat=mlat, verbatim=verbatim, workdir=str(tmp_path))[0] == streams[f"ref_raw_m{mlat}v{verbatim}"]


ENTRIES = ("mgpu_sbs_encode_ex", "mgpu_sbs_encode_ex_device", "mgpu_raw_encode_ex", "mgpu_raw_encode_ex_device")


def test_entries_in_header_library_and_binding(built, tmp_path):
    """The header declares the four entries, the library exports them, the binding mirrors both argument blocks at the size a C
    caller sees — and the entries refuse a NULL context before anything else (a block shorter than the library's: tests/test_gpu_text.py)."""
    import readsb_amd
    from readsb_amd import binding
    header = open(os.path.join(helpers.ROOT, "include", "modes_gpu.h")).read()
    lib = C.CDLL(readsb_amd.lib_path())
    for name in ENTRIES:
        assert re.search(r"\bint %s\(mgpu_ctx \*" % name, header), name
        assert hasattr(lib, name), name
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "modes_gpu.h"\nint main(void){printf("%zu %zu %u %u %u %u\\n",sizeof(struct mgpu_sbs_args),'
                   'sizeof(struct mgpu_raw_args),MGPU_SBS_USE_GNSS,MGPU_RAW_NET_RULE,MGPU_RAW_VERBATIM,MGPU_RAW_MLAT);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(helpers.ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(binding.SbsArgs), C.sizeof(binding.RawArgs), binding.SBS_USE_GNSS, binding.RAW_NET_RULE, binding.RAW_VERBATIM, binding.RAW_MLAT]
    assert int(re.search(r"#define MGPU_ABI_VERSION (\d+)", header).group(1)) == 6        # no struct that existed changed
    for name in ("sbs_encode", "sbs_encode_device", "raw_encode", "raw_encode_device"):
        assert callable(getattr(binding.Demodulator, name))
    nb = C.c_uint64(0)
    a = binding.SbsArgs(C.sizeof(binding.SbsArgs), 0, None, None, None, None, None, 0, su.NOW_MS, -1, None, 0, C.pointer(nb), None, 0, None, None)
    for f in (lib.mgpu_sbs_encode_ex, lib.mgpu_sbs_encode_ex_device):
        f.argtypes, f.restype = [C.c_void_p, C.POINTER(binding.SbsArgs)], C.c_int
        assert f(None, C.byref(a)) == su.MGPU_E_INVAL
    r = binding.RawArgs(C.sizeof(binding.RawArgs), 0, None, None, 0, None, 0, C.pointer(nb), None, 0, None)
    for f in (lib.mgpu_raw_encode_ex, lib.mgpu_raw_encode_ex_device):
        f.argtypes, f.restype = [C.c_void_p, C.POINTER(binding.RawArgs)], C.c_int
        assert f(None, C.byref(r)) == su.MGPU_E_INVAL
