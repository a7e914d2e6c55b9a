"""CPU: the ASTERIX CAT021 output's checker (tests/asterix_util.py) pinned to the reference's own writer, and the two entries' place in
the C ABI.

tests/golden/asterix_cases.npz holds what modesSendAsterixOutput wrote for the case records (tests/golden/make_asterix_golden.py,
through tests/host_stub/asterix_ref_harness.c).  asterix_reference must write the same bytes; where the full reference build is present
the harness is run again and must still write them.  tests/test_gpu_asterix.py then compares the kernels with the checker."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import asterix_util as au
import helpers


@pytest.fixture(scope="module")
def golden():
    return au.load_golden()


def _plain(c, **kw):
    """The checker as the reference's writer sees a record: no verdicts."""
    return au.asterix_of(c, gated=False, **kw)


def test_checker_writes_the_reference_bytes(golden):
    sets, streams, _ = golden
    for g in ("a", "b", "c"):
        sub = au.in_domain(sets[g])
        assert len(sub["msgs"]) == len(sets[g]["msgs"]), "groups a to c lie in the domain"
        for now_ms, remote in au.RUNS:
            assert _plain(sub, now_ms=now_ms, remote=bool(remote))[0] == streams[f"ref_{g}_r{remote}"], (g, remote)
    assert streams["ref_a_r0"] != streams["ref_a_r1"] and streams["ref_b_r0"] != streams["ref_b_r1"]
    clock = au.clock_cases()
    for now_ms in au.CLOCKS:
        assert _plain(clock, now_ms=now_ms)[0] == streams[f"ref_clock_{now_ms}"], now_ms
    # 7 ms after midnight are still 0 units of 1/128 s, 8 ms are 1: the same records, and others
    mid = au.CLOCKS[0]
    assert streams[f"ref_clock_{mid}"] == streams[f"ref_clock_{mid + 7}"] != streams[f"ref_clock_{mid + 8}"]
    assert len({streams[f"ref_clock_{t}"] for t in au.CLOCKS}) == len(au.CLOCKS) - 1


def test_reference_records_parse(golden):
    """Every record of the reference's streams: category 21, its own length, an FSPEC of 4 to 6 bytes with I021/010, /040, /080, /090 and
    /077 set; group b reaches every FSPEC length and the 74 bytes of the bound, nothing is longer."""
    _, streams, _ = golden
    flens, longest = set(), 0
    for name, s in streams.items():
        for r in au.split_records(s):
            k = 3
            while r[k] & 1:
                k += 1
            flens.add(k - 2)
            assert 4 <= k - 2 <= 6 and r[3] & 0xC0 == 0xC0 and r[4] & 0x10 and r[5] & 0x20 and r[6] & 0x02, name
            longest = max(longest, len(r))
    assert flens == {4, 5, 6} and longest == au.RECORD_MAX


def test_known_records():
    """Two records decoded by hand.  2023/11/14 22:13:20.123 is 80000.123 s after midnight: 80000123 * 0.128 = 10240015 = 0x9C400F."""
    c = au._base(1)
    c["ac_category"][:] = 0xA1
    # FSPEC C1 11 21 02: I021/010, /040 | /080 | /090 | /077; SAC/SIC 00 01, descriptor 00, address, quality 00, time of transmission
    assert au.asterix_of(c)[0] == bytes.fromhex("150011" "c1112102" "0001" "00" "4840d6" "00" "9c400f")
    c = au._base(1)
    f = c["fields"]
    f["flags"] |= au.F_BARO_ALT | au.F_SQUAWK | au.F_CALLSIGN
    f["baro_alt"], f["squawkHex"], f["callsign"] = 38000, 0x7421, b"KLM 1023"
    c["positions"]["method"], c["positions"]["lat"], c["positions"]["lon"] = 1, 52.25, -4.75
    c["ids"][:] = 0x1FF
    # 52.25 / (180 / 2^23) = 2435026.49 -> 0x2527D2; -4.75 -> -221366 + 2^24 = 0xFC9F4A; the message 876 ms earlier: 0x9C3F9F; squawk 7421 ->
    # 0F 11; 38000 / 25 = 1520 = 0x05F0; "KLM 1023" in six bits each; the aircraft's category is 0: a 0 byte; receiver id 0x1FF -> FF
    assert au.asterix_of(c)[0] == bytes.fromhex("150028" "c5192b03c104" "0001" "00" "2527d2fc9f4a" "4840d6" "9c3f9f" "00" "0f11" "05f0" "9c400f"
                                                "2cc360c70cb3" "00" "ff")
    # an empty first extension of I021/090: the second's bits stand in its place
    c = au._base(1)
    c["ac_category"][:] = 1
    c["fields"]["acc_flags"], c["fields"]["sda"], c["fields"]["nac_v"] = au.ACC_SDA_VALID | au.ACC_NAC_V_VALID, 2, 3
    assert au.asterix_of(c)[0] == bytes.fromhex("150012" "c1112102" "0001" "00" "4840d6" "6110" "9c400f")
    # a category without a case: the FSPEC bit and no byte
    c = au._base(1)
    c["fields"]["flags"] |= au.F_CATEGORY
    c["fields"]["category"] = 0xC2
    assert au.asterix_of(c)[0] == bytes.fromhex("150012" "c111210340" "0001" "00" "4840d6" "00" "9c400f")


def test_record_rules_on_the_reference_records(golden):
    """With verdicts and the skip rule: a stream is the reference's records of exactly the messages of class LINE, the deferred list names
    those of class DEFER at the offsets their records would start at, the skipped count is the class SKIP."""
    sets, streams, classes = golden
    for g in au.GROUPS:
        c = sets[g]
        cls = au.asterix_classes(c["fields"], c["positions"], c["verdict"], c["ac_baro_alt"])
        assert (cls == classes[g]).all(), g
        stream, length, deferred, nskipped = au.asterix_of(c)
        assert nskipped == int((cls == au.SKIP).sum())
        assert (deferred["index"] == np.nonzero(cls == au.DEFER)[0]).all()
        assert (deferred["offset"] == (np.cumsum(length) - length)[cls == au.DEFER]).all()
        assert ((length > 0) == (cls == au.LINE)).all()
        if g == "d":
            continue
        ref = au.split_records(streams[f"ref_{g}_r0"])
        assert len(ref) == len(cls)
        assert stream == b"".join(r for r, k in zip(ref, cls.tolist()) if k == au.LINE), g
    v = sets["a"]["verdict"] & 3
    assert ((classes["a"] == au.LINE) == (v == au.GATE_FORWARD)).all() and ((classes["a"] == au.DEFER) == (v == au.GATE_DEFER)).all()
    for k in (au.NONE, au.LINE, au.DEFER):
        assert (classes["a"] == k).mean() >= 0.02, k
    # outside the domain: a skip only where the record has the item, whatever the verdict but a drop
    d = sets["d"]
    plain = au.asterix_classes(d["fields"], d["positions"], None, d["ac_baro_alt"])
    assert (plain == au.SKIP).sum() >= 60 and (plain == au.LINE).sum() >= 40
    assert ((classes["d"] == au.SKIP) == ((plain == au.SKIP) & np.isin(d["verdict"] & 3, (au.GATE_FORWARD, au.GATE_DEFER)))).all()


def test_cut_lists(golden):
    """A list cut at 1, 255, 256 and 1000 and concatenated is the one call's stream."""
    sets, _, _ = golden
    c = au.concat_cases([sets["a"], au.slice_cases(sets["b"], 0, 3000), sets["d"]])
    n = len(c["msgs"])
    whole, length, deferred, nskipped = au.asterix_of(c, remote=True)
    for cut in (1, 255, 256, 1000):
        lo = n // 3 if cut == 1 else 0                  # (single records: a stretch of the list)
        hi = lo + 300 if cut == 1 else n
        parts = [au.asterix_of(au.slice_cases(c, k, min(k + cut, hi)), remote=True) for k in range(lo, hi, cut)]
        start = int(length[:lo].sum())
        assert b"".join(p[0] for p in parts) == whole[start:start + int(length[lo:hi].sum())]
        assert sum(len(p[2]) for p in parts) == int(((deferred["index"] >= lo) & (deferred["index"] < hi)).sum())
        if cut != 1:
            assert sum(p[3] for p in parts) == nskipped


@pytest.mark.skipif(not au.have_ref_full(), reason="needs the reference tree and oracle/_ref/full (make -C oracle full)")
def test_fresh_harness_run_writes_the_golden_bytes(golden, tmp_path):
    sets, streams, _ = golden
    exe = au.build_ref_harness(str(tmp_path))
    for g in ("a", "b", "c"):
        for now_ms, remote in au.RUNS:
            got, lens = au.run_ref_harness(exe, sets[g], now_ms=now_ms, remote=remote, workdir=str(tmp_path))
            assert got == streams[f"ref_{g}_r{remote}"], (g, remote)
            assert (lens == _plain(sets[g], now_ms=now_ms, remote=bool(remote))[1]).all()
    clock = au.clock_cases()
    for now_ms in au.CLOCKS:
        assert au.run_ref_harness(exe, clock, now_ms=now_ms, workdir=str(tmp_path))[0] == streams[f"ref_clock_{now_ms}"], now_ms


ENTRIES = ("mgpu_asterix_encode_ex", "mgpu_asterix_encode_ex_device")


def test_entries_in_header_library_and_binding(built, tmp_path):
    """The header declares the two entries, the library exports them, the binding mirrors the argument block at the size a C caller
    sees — and the entries refuse a NULL context before anything else."""
    import readsb_amd
    from readsb_amd import binding
    header = open(os.path.join(helpers.ROOT, "include", "modes_gpu.h")).read()
    lib = C.CDLL(readsb_amd.lib_path())
    for name in ENTRIES:
        assert re.search(r"\bint %s\(mgpu_ctx \*" % name, header), name
        assert hasattr(lib, name), name
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "modes_gpu.h"\nint main(void){printf("%zu %zu %zu %zu %u\\n",sizeof(struct mgpu_asterix_args),'
                   'offsetof(struct mgpu_asterix_args, ids),offsetof(struct mgpu_asterix_args, now_ms),offsetof(struct mgpu_asterix_args, nskipped),'
                   'MGPU_ASTERIX_REMOTE);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(helpers.ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    A = binding.AsterixArgs
    assert got == [C.sizeof(A), A.ids.offset, A.now_ms.offset, A.nskipped.offset, binding.ASTERIX_REMOTE]
    assert binding.ASTERIX_RECORD_MAX == au.RECORD_MAX
    kernel = open(os.path.join(helpers.ROOT, "readsb_amd", "csrc", "kernels", "asterix.inc")).read()
    assert int(re.search(r"constexpr int kAsterixRecordMax = (\d+);", kernel).group(1)) == au.RECORD_MAX
    for name in ("asterix_encode", "asterix_encode_device"):
        assert callable(getattr(binding.Demodulator, name))
    nb = C.c_uint64(0)
    a = A(C.sizeof(A), 0, None, None, None, None, None, None, None, 0, au.NOW_MS, None, 0, C.pointer(nb), None, 0, None, None)
    for f in (lib.mgpu_asterix_encode_ex, lib.mgpu_asterix_encode_ex_device):
        f.argtypes, f.restype = [C.c_void_p, C.POINTER(A)], C.c_int
        assert f(None, C.byref(a)) == au.su.MGPU_E_INVAL
