"""Raw input on the CPU: readsb_amd/csrc/raw_in_format.h — the parser the kernels of kernels/raw_in.inc run — and raw_in_host.cpp's
sequential resolver, compiled for the host and run, in their own process, against the messages the reference's readAscii +
processHexMessage left (tests/golden/raw_in_cases.npz); the parallel rule of the kernels, restated in plain C++, against the
sequential walk on drawn streams; the golden file against the live reference where its objects exist."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import helpers
import raw_in_util as ru

sys.path.insert(0, os.path.join(helpers.ROOT, "tests", "golden"))
import make_raw_in_golden as maker  # noqa: E402

SAN = ("-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")


@pytest.fixture(scope="module")
def golden():
    return ru.load_golden()


def _check_all(exe, tmp_path, golden):
    """Every group and configuration through the program, which compares counts, counters, the class of every line and, with == on
    bytes, every record, source line and signal double."""
    for g in ru.GROUPS:
        for cfg in ru.CONFIGS[g]:
            e = golden[ru.key(g, cfg)]
            out = maker.run_check(exe, e["stream"], cfg, ru.ops_of(g), e, str(tmp_path))
            assert out.split()[:5] == ["ok", "lines", str(int(e["head"][1])), "msgs", str(len(e["msgs"]))], (g, cfg, out)


def test_parser_and_resolver_equal_the_reference(tmp_path, golden):
    """mgpu_raw_parse_line_host plus the sequential resolver give the reference's record for every golden message, and its class
    for every line; the Aerobits signal byte equals the reference's beast byte for every value from -1100 to 1100 mV."""
    exe = maker.build_check(str(tmp_path))
    _check_all(exe, tmp_path, golden)
    r = subprocess.run([exe, "mv"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout == "ok mv\n", r.stdout + r.stderr


def test_parser_under_sanitizers(tmp_path, golden):
    """The same program built with ASan and UBSan, host only, run directly; every line also parsed in a heap copy of exactly its
    bytes."""
    exe = maker.build_check(str(tmp_path), extra=SAN, name="raw_in_format_check_san")
    _check_all(exe, tmp_path, golden)
    r = subprocess.run([exe, "mv"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout == "ok mv\n" and "runtime error" not in r.stderr, r.stdout + r.stderr


@pytest.mark.parametrize("extra, name", [(("-O2",), "raw_in_resolve_check"), (SAN, "raw_in_resolve_check_san")])
def test_parallel_rule_equals_the_sequential_walk(tmp_path, extra, name):
    """tests/host_stub/raw_in_resolve_check.cpp: first adders, new adds, k*, L* and the three-way test against the sequential walk over
    the filter's model on 10 000 drawn streams of 50 to 600 lines — every line's verdict and the final filter equal; plain and under
    ASan and UBSan."""
    exe = maker.build_check(str(tmp_path), extra=extra, name=name, src="raw_in_resolve_check.cpp")
    r = subprocess.run([exe, "10000", "7"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok streams 10000 ") and "runtime error" not in r.stderr, r.stdout[-2000:] + r.stderr[-2000:]
    w = r.stdout.split()
    assert int(w[6]) > 1000 and int(w[8]) > 10000, r.stdout            # streams that crossed a growth; lines the growth made unknown


def test_golden_is_what_the_generators_build(golden):
    """The golden's streams are the seeded generators' (so the groups are what tests/raw_in_util.py says they are), 5 to 7 tiles each;
    the reference consumed every stream whole, its counters add up, every record carries the stamp."""
    groups = ru.build_groups()
    for g, cfgs in ru.CONFIGS.items():
        for cfg in cfgs:
            e = golden[ru.key(g, cfg)]
            assert e["stream"] == ru.stream_of(groups[g]), g
            head = [int(x) for x in e["head"]]
            assert head[0] == len(e["stream"]) and head[1] == len(ru.split_lines(e["stream"])) == len(e["cls"]) and head[2] == len(e["msgs"]) == len(e["line_of"]) == len(e["signal"])
            assert head[3] == head[5] + head[6] + sum(head[7:10]) and head[2] == head[4] + sum(head[7:10]), (g, cfg, head)
            assert (e["msgs"]["sysTimestamp"] == ru.NOW_MS).all() and (e["msgs"]["score"] == 0).all() and (e["msgs"]["phase"] == 0).all() and (e["msgs"]["sig_len"] == 1).all()
            assert (np.diff(e["line_of"].astype(np.int64)) > 0).all(), (g, cfg)
            accepted = np.isin(e["cls"], (ru.ACCEPT, ru.MODEAC))
            assert (np.nonzero(accepted)[0] == e["line_of"]).all(), (g, cfg)
            if g != "d2":
                assert 5 * ru.TILE - 1000 <= len(e["stream"]) <= 7.5 * ru.TILE, (g, len(e["stream"]))
    assert os.path.getsize(ru.GOLDEN) < 700000


def test_abi_version_and_struct_sizes():
    """MGPU_ABI_VERSION is still 6; the binding's mirrors have the header's sizes."""
    import readsb_amd.binding as rb
    text = open(os.path.join(helpers.ROOT, "include", "modes_gpu.h")).read()
    assert re.search(r"^#define MGPU_ABI_VERSION 6$", text, flags=re.M) and rb.ABI_VERSION == 6
    assert C.sizeof(rb.RawInArgs) == 120 and C.sizeof(rb.RawInCounters) == 56 and C.sizeof(rb.RawInConfig) == 16 and C.sizeof(rb.RawInLine) == 88 and C.sizeof(rb.RawInFilter) == 40
    assert rb.MSG_DTYPE.itemsize == 64 == ru.MSG.itemsize and rb.MSG_DTYPE.names == ru.MSG.names
    assert (rb.RAW_NONE, rb.RAW_MODEAC, rb.RAW_BAD, rb.RAW_ACCEPT, rb.RAW_COND, rb.RAW_UNKNOWN) == (ru.NONE, ru.MODEAC, ru.BAD, ru.ACCEPT, ru.COND, ru.UNKNOWN)
    for name, value in (("NONE", 0), ("MODEAC", 1), ("BAD", 2), ("ACCEPT", 3), ("COND", 4), ("UNKNOWN", 5)):
        assert re.search(r"^#define MGPU_RAW_%s +%du" % (name, value), text, flags=re.M), name


def test_host_entries_through_the_library(golden):
    """mgpu_raw_parse_line_host and mgpu_raw_decode_host of the built library (no GPU needed): a line's class, address and adder flag;
    group (c) and group (d) from its prepared filter; the departures; bad arguments; a capacity one short leaves the filter alone."""
    import readsb_amd.binding as rb
    lib = rb.load_library()
    cfg = rb.RawInConfig(C.sizeof(rb.RawInConfig), 1, 1, 0)
    out = rb.RawInLine()

    def parse(line, c=cfg):
        buf = np.frombuffer(line, dtype=np.uint8)
        return int(lib.mgpu_raw_parse_line_host(buf.ctypes.data if len(line) else None, len(line), ru.NOW_MS, C.byref(c), C.byref(out)))
    assert parse(ru.avr(ru.es(0x4840D6, 1), end=b"\r")) == 1 and (out.cls, out.addr, out.adder) == (ru.ACCEPT, 0x4840D6, 1)
    assert parse(ru.avr(ru.es(0x4840D6, 1, True), end=b"")) == 1 and (out.cls, out.addr, out.adder) == (ru.ACCEPT, 0x4840D6, 0)
    assert parse(ru.avr(ru.df11(0x4840D6, 3), end=b"")) == 1 and (out.cls, out.addr, out.adder) == (ru.ACCEPT, 0x4840D6, 0)
    assert parse(ru.avr(ru.flipped(ru.es(0x4840D6, 1), 1), end=b"")) == 1 and (out.cls, out.adder) == (ru.ACCEPT, 0)      # fixDF17msgtype: accepted, never adds
    assert parse(ru.avr(ru.ap(20, 0x123456, 1), end=b"")) == 1 and (out.cls, out.addr, out.adder) == (ru.COND, 0x123456, 0)
    assert parse(ru.avr(ru.flipped(ru.es(0x4840D6, 1), 50, 51, 52), end=b"")) == 1 and out.cls == ru.BAD and not bytes(out.msg).strip(b"\0")
    assert parse(b"*7700;") == 0 and out.cls == ru.NONE
    assert parse(b"*7700;", rb.RawInConfig(C.sizeof(rb.RawInConfig), 1, 1, 1)) == 1 and out.cls == ru.MODEAC and out.addr == 0x7700
    assert parse(b"") == 0 and parse(b"\r") == 0 and parse(ru.LONG_LINES[0][:-1]) == 0                                   # the departures
    assert lib.mgpu_raw_parse_line_host(None, 5, 0, C.byref(cfg), C.byref(out)) == ru.MGPU_E_INVAL
    assert parse(b"*7700;", rb.RawInConfig(8, 1, 1, 0)) == ru.MGPU_E_INVAL and parse(b"*7700;", rb.RawInConfig(C.sizeof(rb.RawInConfig), 3, 1, 0)) == ru.MGPU_E_INVAL
    for g in ("c", "d"):
        e = golden[ru.key(g, (1, 1, 0))]
        f = ru.FilterModel()
        for op in ru.ops_of(g):
            f.expire() if op < 0 else f.add(op)
        res = ru.host_decode(lib, e["stream"], (1, 1, 0), f)
        assert res["rc"] == ru.MGPU_OK and [res["consumed"], res["nlines"], res["nmsgs"], *res["counters"]] == [int(x) for x in e["head"]]
        assert res["msgs"].tobytes() == e["msgs"].tobytes() and res["cls"].tobytes() == e["cls"].tobytes() and res["signal"].tobytes() == e["signal"].tobytes()
        if g == "d":                                                       # two growths: 256 -> 1024 buckets, the inactive generation gone
            assert (f.bits, f.occupied, len(f.inactive)) == (10, len(f.active), 0) and len(f.active) == 40 + 150 + 2
    # a capacity one short: MGPU_E_OVERFLOW with what is needed, the filter as it was
    e = golden[ru.key("c", (1, 1, 0))]
    f = ru.FilterModel()
    buf = np.frombuffer(e["stream"], dtype=np.uint8)
    n = len(e["msgs"])
    msgs = np.zeros(n, dtype=ru.MSG)
    c = [C.c_uint64(0) for _ in range(3)]
    cn = rb.RawInCounters()
    a = rb.RawInArgs(C.sizeof(rb.RawInArgs), 0, buf.ctypes.data, buf.size, ru.NOW_MS, msgs.ctypes.data, None, None, n - 1, None, 0, *[C.pointer(x) for x in c], C.pointer(cn), 0)
    ga, gi = np.zeros(buf.size, dtype=np.uint32), np.zeros(1, dtype=np.uint32)
    flt = rb.RawInFilter(ga.ctypes.data, gi.ctypes.data, 0, 0, 0, 8)
    assert lib.mgpu_raw_decode_host(C.byref(a), C.byref(cfg), C.byref(flt)) == ru.MGPU_E_OVERFLOW
    assert int(c[2].value) == n and (flt.n_active, flt.occupied, flt.table_bits) == (0, 0, 8) and msgs[: n - 1].tobytes() == e["msgs"][: n - 1].tobytes() and not msgs[n - 1:].tobytes().strip(b"\0")
    a.msgs_cap = n
    assert lib.mgpu_raw_decode_host(C.byref(a), C.byref(cfg), C.byref(flt)) == ru.MGPU_OK and flt.n_active > 30 and msgs.tobytes() == e["msgs"].tobytes()


@pytest.mark.skipif(not ru.have_ref_full(), reason="needs the reference tree and the objects of oracle/_ref/full")
def test_live_reference_equals_the_golden(tmp_path, golden):
    """tests/host_stub/raw_in_ref_harness.c, which includes the reference's net_io.c, leaves the golden's results; and on a stream cut
    in the middle of a line it consumes up to the last terminator only."""
    exe = ru.build_ref_harness(str(tmp_path))
    for g in ru.GROUPS:
        for cfg in ru.CONFIGS[g]:
            streams = [golden[ru.key(g, cfg)]["stream"]] + ([golden[ru.key("d2", cfg)]["stream"]] if g == "d" else [])
            for name, res in zip((g, "d2"), ru.run_ref_harness(exe, streams, cfg, str(tmp_path), ops=ru.ops_of(g))):
                e = golden[ru.key(name, cfg)]
                assert (res["head"] == e["head"]).all() and (res["cls"] == e["cls"]).all() and (res["line_of"] == e["line_of"]).all(), (name, cfg)
                assert res["signal"].tobytes() == e["signal"].tobytes() and res["msgs"].tobytes() == e["msgs"].tobytes(), (name, cfg)
    e = golden[ru.key("c", (1, 1, 0))]
    cut = e["stream"][: len(e["stream"]) // 2 + 7]
    res = ru.run_ref_harness(exe, [cut], (1, 1, 0), str(tmp_path))[0]
    assert int(res["head"][0]) == max(cut.rfind(b"\n"), cut.rfind(b"\0")) + 1 and int(res["head"][1]) == len(ru.split_lines(cut))
    assert res["msgs"].tobytes() == e["msgs"][: len(res["msgs"])].tobytes()
