"""ASTERIX input on the CPU: readsb_amd/csrc/asterix_in_format.h — the framing rule and the parser the kernels of
kernels/asterix_in.inc run — and asterix_in_host.cpp's mgpu_asterix_parse_host, compiled for the host and run, in their own process,
against the records the reference's readAsterix + decodeAsterixMessage left (tests/golden/asterix_in_cases.npz); the golden file and
freshly drawn streams against the live reference where its objects exist."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import helpers
import asterix_in_util as au

sys.path.insert(0, os.path.join(helpers.ROOT, "tests", "golden"))
import make_asterix_in_golden as maker  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return au.load_golden()


def _check_all(exe, tmp_path, golden):
    """The rules without a reference, then every group at both clocks through the program, which compares record by record; here: the
    counts."""
    maker.run_rules(exe)
    for g in au.GROUPS:
        stream, by_now = golden[g]
        for now_ms, (head, frame_of, recs) in by_now.items():
            frames, nrecs, nother, nundef, consumed, stop = maker.run_check(exe, stream, now_ms, frame_of, recs, str(tmp_path))
            assert (consumed, frames, nrecs, nother, stop) == tuple(int(x) for x in head) and nundef == 0, (g, now_ms)


def test_parser_equals_the_reference(tmp_path, golden):
    """The parser gives the reference's record for every frame of every group, frames and stops as the reference's; the time function
    equals (int)(raw / .128) for all 2^24 raw values; the high-precision arithmetic, a length of 0, an incomplete record and chains of
    190 to 193 extension bytes in all four places behave as include/modes_gpu.h says."""
    _check_all(maker.build_check(str(tmp_path)), tmp_path, golden)


def test_parser_under_sanitizers(tmp_path, golden):
    """The same program built with ASan and UBSan, host only, run directly; the stream parsed in a heap copy of exactly its bytes."""
    exe = maker.build_check(str(tmp_path), extra=("-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"), name="asterix_in_format_check_san")
    _check_all(exe, tmp_path, golden)


def test_golden_is_what_the_generators_build(golden):
    """The golden's streams are the seeded generators'; the counts are the framing rule's; the stops are where the groups put them;
    padding is zero; the high-precision arithmetic's wrapped values are there."""
    groups = au.build_groups()
    for g in au.GROUPS:
        stream, by_now = golden[g]
        assert stream == au.stream_of(groups[g]), g
        starts, end, stop = au.frames_of(stream)
        assert stop == au.STOP_END
        for now_ms, (head, frame_of, recs) in by_now.items():
            assert int(head[2]) == len(recs) == len(frame_of) and (recs["reserved"] == 0).all() and (recs["source"] == au.SOURCE).all(), (g, now_ms)
            assert (np.diff(frame_of.astype(np.int64)) > 0).all(), (g, now_ms)
            if g == "c1":
                assert int(head[4]) == au.STOP_CLOSED and int(head[1]) == 21 and len(recs) == 20 and int(head[0]) == starts[21]
            else:
                assert int(head[4]) == au.STOP_END and int(head[0]) == end and int(head[1]) == len(starts), (g, now_ms)
        assert (by_now[au.NOWS[0]][2]["sysTimestamp"] < 0).sum() >= 5 or g.startswith("c")
    assert golden["c2"][1][au.NOWS[0]][0][0] < len(golden["c2"][0])                                 # the truncated tail is not consumed
    assert os.path.getsize(au.GOLDEN) < 400000


def test_abi_version_and_record_layout():
    """MGPU_ABI_VERSION is still 6; the binding's mirrors have the header's sizes (the header asserts 128 for the record)."""
    import readsb_amd.binding as rb
    text = open(os.path.join(helpers.ROOT, "include", "modes_gpu.h")).read()
    assert re.search(r"^#define MGPU_ABI_VERSION 6$", text, flags=re.M) and rb.ABI_VERSION == 6
    assert "_Static_assert(sizeof(struct mgpu_asterix_rec) == 128" in text
    assert rb.ASTERIX_REC_DTYPE.itemsize == 128 and rb.ASTERIX_REC_DTYPE == au.REC
    assert C.sizeof(rb.AsterixInArgs) == 112
    assert (rb.AST_STOP_END, rb.AST_STOP_ZERO_LEN, rb.AST_STOP_CLOSED) == (au.STOP_END, au.STOP_ZERO_LEN, au.STOP_CLOSED)


def test_parse_host_through_the_library(golden):
    """mgpu_asterix_parse_host / _parse_record_host of the built library (no GPU needed): the golden's records bytewise through
    tests/asterix_in_util.py's expect(), which the GPU tests use; bad arguments."""
    import readsb_amd.binding as rb
    lib = rb.load_library()
    for g in au.GROUPS:
        stream, by_now = golden[g]
        for now_ms, (head, frame_of, recs) in by_now.items():
            want = au.expect(lib, stream, now_ms=now_ms)
            assert want["recs"].tobytes() == recs.tobytes() and (want["frame_of"] == frame_of).all(), (g, now_ms)
            assert (want["consumed"], want["nframes"], want["nother"], want["stop"], want["nundefined"]) == (int(head[0]), int(head[1]), int(head[3]), int(head[4]), 0)
    stream, by_now = golden["b"]
    head, frame_of, recs = by_now[au.NOWS[1]]
    buf = np.frombuffer(stream, dtype=np.uint8)
    one = np.zeros(1, dtype=au.REC)
    a = rb.AsterixInArgs(size=C.sizeof(rb.AsterixInArgs), source=au.SOURCE, data=buf.ctypes.data, nbytes=buf.size, now_ms=au.NOWS[1])
    for k in (0, 1, len(recs) // 2, len(recs) - 1):
        assert lib.mgpu_asterix_parse_host(C.byref(a), int(frame_of[k]), one.ctypes.data) == 1
        assert one.tobytes() == recs[k: k + 1].tobytes(), k
    assert lib.mgpu_asterix_parse_host(C.byref(a), int(head[1]), one.ctypes.data) == au.MGPU_E_INVAL
    a.source = 12
    assert lib.mgpu_asterix_parse_host(C.byref(a), 0, one.ctypes.data) == au.MGPU_E_INVAL
    a.source, a.size = au.SOURCE, C.sizeof(rb.AsterixInArgs) - 8
    assert lib.mgpu_asterix_parse_host(C.byref(a), 0, one.ctypes.data) == au.MGPU_E_INVAL
    assert lib.mgpu_asterix_parse_record_host(buf.ctypes.data, buf.size, buf.size, au.SOURCE, 0, one.ctypes.data) == au.MGPU_E_INVAL
    assert lib.mgpu_asterix_parse_record_host(buf.ctypes.data, buf.size, 0, au.SOURCE, -1, one.ctypes.data) == au.MGPU_E_INVAL
    assert lib.mgpu_asterix_parse_record_host(buf.ctypes.data, buf.size, 0, au.SOURCE, 0, None) == au.MGPU_E_INVAL
    zero = np.frombuffer(b"\x15\x00\x00\x01\x10", dtype=np.uint8)                                   # the rules the reference cannot be given
    want = au.expect(lib, zero.tobytes())
    assert (want["stop"], want["consumed"], want["nframes"]) == (au.STOP_ZERO_LEN, 0, 0)
    long_chain = bytes([21]) + au.len_bytes(300) + b"\xff" * 297
    want = au.expect(lib, long_chain + au.frame({"080": b"\x01\x02\x03"}))
    assert (want["stop"], want["nframes"], want["nundefined"], len(want["recs"])) == (au.STOP_END, 2, 1, 1)


@pytest.mark.skipif(not au.have_ref_full(), reason="needs the reference tree and the objects of oracle/_ref/full")
def test_live_reference_equals_the_golden(tmp_path, golden):
    """tests/host_stub/asterix_in_ref_harness.c, which includes the reference's net_io.c, leaves the golden's records."""
    exe = au.build_ref_harness(str(tmp_path))
    for g in au.GROUPS:
        stream, by_now = golden[g]
        for now_ms, (head, frame_of, recs) in by_now.items():
            rhead, rframe_of, rrecs = au.run_ref_harness(exe, stream, str(tmp_path), now_ms=now_ms)
            assert (rhead == head).all() and (rframe_of == frame_of).all() and rrecs.tobytes() == recs.tobytes(), (g, now_ms)


@pytest.mark.skipif(not au.have_ref_full(), reason="needs the reference tree and the objects of oracle/_ref/full")
def test_live_reference_equals_the_host_parser_on_fresh_streams(tmp_path):
    """Freshly drawn streams of every group's kind — well-formed records, drawn item bytes behind consistent headers with other
    categories between them, a record without an address in the middle, a truncated tail — at a drawn clock and source: the host
    parser's records, frames, counts and stop are the live reference's."""
    import readsb_amd.binding as rb
    lib = rb.load_library()
    exe = au.build_ref_harness(str(tmp_path))
    seed = int.from_bytes(os.urandom(4), "little")
    rng = np.random.default_rng(seed)
    now_ms = int(rng.integers(1600000000000, 1900000000000))
    source = int(rng.integers(0, 12))
    fresh = au.feed(300, seed=seed, now_ms=now_ms)
    hostile = []
    for k in range(200):
        it = au.every_item(rng)
        hostile.append(au.frame({name: v for name, v in it.items() if name == "080" or rng.integers(0, 2)}, cat=21 if k % 7 else int(rng.integers(0, 256))))
    closed = au.frame({"145": au.be(5, 2)})
    for name, stream in (("a", b"".join(fresh)), ("b", b"".join(hostile)), ("c1", b"".join(fresh[:50]) + closed + b"".join(fresh[50:])), ("c2", b"".join(fresh)[:-3])):
        head, frame_of, recs = au.run_ref_harness(exe, stream, str(tmp_path), source=source, now_ms=now_ms)
        want = au.expect(lib, stream, source=source, now_ms=now_ms)
        assert (want["consumed"], want["nframes"], len(want["recs"]), want["nother"], want["stop"]) == tuple(int(x) for x in head), (name, seed)
        assert want["recs"].tobytes() == recs.tobytes() and (want["frame_of"] == frame_of).all() and want["nundefined"] == 0, (name, seed)
