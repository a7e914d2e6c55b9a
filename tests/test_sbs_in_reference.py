"""SBS input on the CPU: readsb_amd/csrc/sbs_in_format.h — the parser the kernels of kernels/sbs_in.inc run — and sbs_in_host.cpp's
mgpu_sbs_parse_host, compiled for the host and run, in their own process, against the records the reference's readAscii +
decodeSbsLine left (tests/golden/sbs_in_cases.npz); the golden file against the live reference where its objects exist."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import helpers
import sbs_in_util as su

sys.path.insert(0, os.path.join(helpers.ROOT, "tests", "golden"))
import make_sbs_in_golden as maker  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return su.load_golden()


def _check_all(exe, tmp_path, golden):
    """Every group and source through the program, which compares record by record; here: the counts and who is deferred."""
    for g in su.GROUPS:
        stream, by_source = golden[g]
        nlines = len(su.split_lines(stream))
        for s, (head, line_of, recs) in by_source.items():
            got_lines, nplain, ninvalid, consumed, deferred = maker.run_check(exe, stream, s, line_of, recs, str(tmp_path))
            assert (got_lines, ninvalid, consumed) == (nlines, int(head[3]), int(head[0])), (g, s)
            if g == "c":                                      # every hostile number is deferred, and the host settles it to the reference's record
                assert nplain == 0 and deferred == list(range(nlines)) and len(recs) == nlines, (g, s)
            else:                                             # a condition of the groups: nothing ordinary is deferred
                assert deferred == [] and nplain == len(recs), (g, s, deferred)


def test_parser_equals_the_reference(tmp_path, golden):
    """The plain parse gives the reference's record for every line of groups (a) and (b) and defers none; every line of group (c) is
    deferred and mgpu_sbs_parse_host gives the reference's record; invalid lines and heartbeats give none and are counted as the
    reference counts them."""
    _check_all(maker.build_check(str(tmp_path)), tmp_path, golden)


def test_parser_under_sanitizers(tmp_path, golden):
    """The same program built with ASan and UBSan, host only, run directly; every line parsed in a heap copy of exactly its bytes."""
    exe = maker.build_check(str(tmp_path), extra=("-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"), name="sbs_in_format_check_san")
    _check_all(exe, tmp_path, golden)


def test_golden_is_what_the_generators_build(golden):
    """The golden's streams are the seeded generators' (so the groups are what tests/sbs_in_util.py says they are); the reference
    consumed every stream whole, its two counters add up, every record carries the stamp and its source, padding is zero."""
    groups = su.build_groups()
    for g in su.GROUPS:
        stream, by_source = golden[g]
        assert stream == su.stream_of(groups[g]), g
        for s, (head, line_of, recs) in by_source.items():
            assert int(head[0]) == len(stream) and int(head[1]) == len(su.split_lines(stream)) and int(head[2]) == int(head[4]) == len(recs) == len(line_of), (g, s)
            assert (recs["sysTimestamp"] == su.NOW_MS).all() and (recs["source"] == su.SOURCES[s]).all() and (recs["reserved"] == 0).all(), (g, s)
            assert (np.diff(line_of.astype(np.int64)) > 0).all(), (g, s)
    assert os.path.getsize(su.GOLDEN) < 400000


def test_abi_version_and_record_layout():
    """MGPU_ABI_VERSION is still 6; the binding's mirrors have the header's sizes (the header asserts 96 for the record)."""
    import readsb_amd.binding as rb
    text = open(os.path.join(helpers.ROOT, "include", "modes_gpu.h")).read()
    assert re.search(r"^#define MGPU_ABI_VERSION 6$", text, flags=re.M) and rb.ABI_VERSION == 6
    assert "_Static_assert(sizeof(struct mgpu_sbs_rec) == 96" in text
    assert rb.SBS_REC_DTYPE.itemsize == 96 == su.REC.itemsize and rb.SBS_REC_DTYPE == su.REC
    assert C.sizeof(rb.SbsInArgs) == 120
    assert rb.SBS_SOURCES == su.SOURCES


def test_parse_host_through_the_library(golden):
    """mgpu_sbs_parse_host / _line_host of the built library (no GPU needed): group (c)'s records; bad arguments."""
    import readsb_amd.binding as rb
    lib = rb.load_library()
    stream, by_source = golden["c"]
    buf = np.frombuffer(stream, dtype=np.uint8)
    one = np.zeros(1, dtype=su.REC)
    for s, (head, line_of, recs) in by_source.items():
        a = rb.SbsInArgs(size=C.sizeof(rb.SbsInArgs), source=su.SOURCES[s], text=buf.ctypes.data, nbytes=buf.size, now_ms=su.NOW_MS)
        for k in (0, 1, len(recs) // 2, len(recs) - 1):
            assert lib.mgpu_sbs_parse_host(C.byref(a), int(line_of[k]), one.ctypes.data) == 1
            assert one.tobytes() == recs[k: k + 1].tobytes(), (s, k)
        assert lib.mgpu_sbs_parse_host(C.byref(a), int(head[1]), one.ctypes.data) == su.MGPU_E_INVAL
        a.source = 5
        assert lib.mgpu_sbs_parse_host(C.byref(a), 0, one.ctypes.data) == su.MGPU_E_INVAL
        a.source, a.size = su.SOURCES[s], C.sizeof(rb.SbsInArgs) - 8
        assert lib.mgpu_sbs_parse_host(C.byref(a), 0, one.ctypes.data) == su.MGPU_E_INVAL
    line = su.sbs(alt="35000H", end=b"\r")
    lb = np.frombuffer(line, dtype=np.uint8)
    assert lib.mgpu_sbs_parse_line_host(lb.ctypes.data, lb.size, 3, 7, one.ctypes.data) == 1 and int(one["baro_alt"][0]) == 35000 and int(one["sysTimestamp"][0]) == 7
    assert lib.mgpu_sbs_parse_line_host(lb.ctypes.data, lb.size, 3, 7, None) == su.MGPU_E_INVAL
    assert lib.mgpu_sbs_parse_line_host(lb.ctypes.data, 5, 3, 7, one.ctypes.data) == 0 and not one.tobytes().strip(b"\0")


@pytest.mark.skipif(not su.have_ref_full(), reason="needs the reference tree and the objects of oracle/_ref/full")
def test_live_reference_equals_the_golden(tmp_path, golden):
    """tests/host_stub/sbs_in_ref_harness.c, which includes the reference's net_io.c, leaves the golden's records; and on a stream cut
    in the middle of a line it consumes up to the last terminator only."""
    exe = su.build_ref_harness(str(tmp_path))
    for g in su.GROUPS:
        stream, by_source = golden[g]
        for s, (head, line_of, recs) in by_source.items():
            rhead, rline_of, rrecs = su.run_ref_harness(exe, stream, s, str(tmp_path))
            assert (rhead == head).all() and (rline_of == line_of).all() and rrecs.tobytes() == recs.tobytes(), (g, s)
    stream, by_source = golden["a"]
    cut = stream[: len(stream) // 2 + 7]
    head, line_of, recs = su.run_ref_harness(exe, cut, "sbs", str(tmp_path))
    assert int(head[0]) == max(cut.rfind(b"\n"), cut.rfind(b"\0")) + 1 and int(head[1]) == len(su.split_lines(cut))
    assert recs.tobytes() == by_source["sbs"][2][: len(recs)].tobytes()
