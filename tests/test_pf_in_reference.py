"""Planefinder input on the CPU: readsb_amd/csrc/pf_in_format.h — the framer and parser the kernels of kernels/pf_in.inc run — and
pf_in_host.cpp's sequential walk, compiled for the host and run, in their own process, against what the reference's readPlanefinder +
decodePfMessage left (tests/golden/pf_in_cases.npz); every prefix of hostile streams under ASan and UBSan; the host entries of the built
library, the passes of the host form among them; the golden file and a few thousand drawn streams against the live reference where its
objects exist."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import beast_in_util as bu
import helpers
import pf_in_util as pu
import raw_in_util as ru

sys.path.insert(0, os.path.join(helpers.ROOT, "tests", "golden"))
import make_pf_in_golden as maker  # noqa: E402

SAN = ("-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")
D, E = b"\x10", b"\x03"


@pytest.fixture(scope="module")
def golden():
    return pu.load_golden()


@pytest.fixture(scope="module")
def lib():
    import readsb_amd.binding as rb
    return rb.load_library()


def hostile_streams():
    """Short streams whose every prefix is walked."""
    long_, short, ac = ru.es(pu.A, 3)[:14].tobytes(), ru.df11(pu.A)[:7].tobytes(), b"\x77\x00"
    good = pu.frame(long_)
    rng = np.random.default_rng(5)
    bare = b""
    for at in range(11 + 7):                                                                 # a bare DLE in every field position, and the same stuffed
        body = bytearray(b"\x00\x01\x80" + bytes.fromhex("0123456700 89abcd".replace(" ", "")) + short)
        body[at] = 0x10
        bare += D + b"\xc1" + bytes(body) + D + E + D + b"\xc1" + pu.stuffed(body) + D + E
    types = b"".join(pu.frame(short if t & 1 else long_, type_=t) for t in list(range(16)) + [hi << 4 | t for t, hi in zip(range(16), (15, 1, 2, 4, 8, 3, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15))])
    return [pu.frame(long_[:6] + D + E + long_[8:]) + good + pu.TINY + good + good[:25],      # DLE DLE ETX in a body; the 4-byte frame; no end
            pu.TINY + pu.TINY + pu.frame(ac) + pu.TINY + pu.frame(short) + pu.TINY,           # ... running through its end into the frames behind, and behind the buffer
            bare,
            b"".join(D * n + good for n in range(1, 8)) + D + E + good + D + E + D + E + D,   # runs of DLE; DLE ETX while searching; a DLE as last byte
            pu.frame(long_, pid=0x41) + good + pu.frame(long_, pid=0x10) + good + D + b"\x41" + good + good,
            types + pu.frame(long_, secs=0xFFFFFFFF, nanos=0xFFFFFFFF, sig=0xFF) + pu.frame(ac, secs=0xFFFFFFFF, nanos=0xFFFFFFFF),
            pu.draw_stream(rng, 12, hostile=1.0), pu.draw_stream(rng, 12, hostile=2.0), pu.draw_automaton_stream(rng, 400)]


def _check_all(exe, tmp_path, golden):
    for g in pu.GROUPS:
        for cfg in pu.CONFIGS[g]:
            e = golden[pu.key(g, cfg)]
            out = maker.run_check(exe, e["stream"], cfg, pu.ops_of(g), e, str(tmp_path)).split()
            assert out[:5] == ["ok", "frames", str(int(e["head"][1])), "msgs", str(len(e["msgs"]))], (g, cfg, out)
            assert (int(out[8]) != 0) == (g == "p"), (g, out)                                # past_end: in exactly the group built for it


def test_framer_parser_and_walk_equal_the_reference(tmp_path, golden):
    """The sequential walk gives the reference's counts, counters, class and offset per handler call and, with == on bytes, every
    record, handler-call index and signal double of every golden stream; and agrees with a walk over mgpu_pf_parse_host alone, and with
    itself in passes of 1, 7 and 33 bytes, on every prefix of the hostile streams."""
    exe = maker.build_check(str(tmp_path))
    _check_all(exe, tmp_path, golden)
    for s in hostile_streams():
        for cfg in ((1, 1, 1), (1, 1, 0)):
            assert maker.run_prefixes(exe, s, cfg, str(tmp_path)).split()[2] == str(len(s) + 1)


def test_framer_and_parser_under_sanitizers(tmp_path, golden):
    """The same stand-alone program built with ASan and UBSan, host only, run directly: the golden streams and every prefix of the
    hostile ones, each in a heap copy of exactly its bytes."""
    exe = maker.build_check(str(tmp_path), extra=SAN, name="pf_in_format_check_san")
    _check_all(exe, tmp_path, golden)
    for s in hostile_streams():
        assert maker.run_prefixes(exe, s, (1, 1, 1), str(tmp_path)).split()[2] == str(len(s) + 1)


def test_golden_is_what_the_generators_build(golden):
    """The golden's streams are the seeded generators', three to five tiles each (the second call of group d aside); every class is
    there where its configuration allows it; the reference's counters add up, every record carries the stamp, the accepted handler calls
    are the messages' sources; the file is no larger than the beast input's."""
    groups = pu.build_groups()
    seen = {0: set(), 1: set()}
    for g, cfgs in pu.CONFIGS.items():
        for cfg in cfgs:
            e = golden[pu.key(g, cfg)]
            assert e["stream"] == pu.stream_of(groups[g]), g
            head = [int(x) for x in e["head"]]
            assert head[0] <= len(e["stream"]) and head[1] == len(e["cls"]) == len(e["off"]) and head[2] == len(e["msgs"]) == len(e["frame_of"]) == len(e["signal"])
            assert head[1] <= len(e["stream"]) // 4 and head[2] <= head[1]
            assert head[3] == head[5] + head[6] + sum(head[7:10]), (g, cfg, head)
            assert head[4] == int((e["cls"] == pu.MODEAC).sum()) and head[2] == head[4] + sum(head[7:10])
            assert (e["msgs"]["sysTimestamp"] == pu.NOW_MS).all() and (e["msgs"]["score"] == 0).all() and (e["msgs"]["sig_len"] == 1).all()
            assert (np.nonzero(np.isin(e["cls"], (pu.ACCEPT, pu.MODEAC)))[0] == e["frame_of"]).all(), (g, cfg)
            stream = np.frombuffer(e["stream"], dtype=np.uint8)
            off = e["off"].astype(np.int64)
            assert (np.diff(off) >= 4).all() and (stream[off] == pu.DLE).all() and (stream[off + 1] == pu.PID).all()
            if g != "d2":
                assert 3 * pu.TILE <= len(e["stream"]) <= 5 * pu.TILE, (g, len(e["stream"]))
            seen[cfg[2]] |= set(e["cls"].tolist())
    assert seen[0] == {pu.BAD, pu.ACCEPT, pu.UNKNOWN, pu.MODEAC_OFF, pu.TYPE} and seen[1] == {pu.MODEAC, pu.BAD, pu.ACCEPT, pu.UNKNOWN, pu.TYPE}
    assert os.path.getsize(pu.GOLDEN) <= os.path.getsize(bu.GOLDEN)


def test_abi_version_and_struct_sizes():
    """MGPU_ABI_VERSION is still 6; the binding's mirrors have the header's sizes; the classes the filter passes share are MGPU_RAW_*'s."""
    import readsb_amd.binding as rb
    text = open(os.path.join(helpers.ROOT, "include", "modes_gpu.h")).read()
    assert re.search(r"^#define MGPU_ABI_VERSION 6$", text, flags=re.M) and rb.ABI_VERSION == 6
    assert C.sizeof(rb.PfInArgs) == 128 and C.sizeof(rb.PfInCounters) == 72 and C.sizeof(rb.PfInFrame) == 112
    for name, value in (("MODEAC", 1), ("BAD", 2), ("ACCEPT", 3), ("COND", 4), ("UNKNOWN", 5), ("MODEAC_OFF", 6), ("TYPE", 7)):
        assert re.search(r"^#define MGPU_PF_IN_%s +%du" % (name, value), text, flags=re.M), name
    for name in ("MODEAC", "BAD", "ACCEPT", "COND", "UNKNOWN"):
        assert getattr(pu, name) == getattr(ru, name)
    for name, value in (("END", 0), ("SKIP", 1), ("OTHER", 2), ("FRAME", 3), ("INCOMPLETE", 4)):
        assert re.search(r"^#define MGPU_PF_STEP_%s +%du" % (name, value), text, flags=re.M), name


def test_parse_host_step_by_step(lib):
    """mgpu_pf_parse_host: the som a step leaves, the kind and what a handler call carries, for each kind of step."""
    cfg, ac = (1, 1, 0), (1, 1, 1)
    long_ = ru.es(0x4840D6, 1)[:14].tobytes()
    good = pu.frame(long_, secs=0x10203040, nanos=0x05060710, sig=0x10)
    rc, f = pu.parse_host(lib, good, 0, cfg)
    assert rc == 1 and (f.step, f.next, f.frame_off, f.cls, f.addr, f.adder, f.past_end) == (pu.STEP_FRAME, len(good), 0, pu.ACCEPT, 0x4840D6, 1, 0)
    m = np.frombuffer(bytes(f.msg), dtype=pu.MSG)[0]
    assert int(m["timestamp"]) == 0x10203040 * 1000000000 + 0x05060710 and bytes(m["raw"]) == long_ and int(m["sig_sumsq"]) == (257 * 0x10) ** 2
    assert f.signal_level == (0x10 / 255.0) * (0x10 / 255.0) and int(m["sysTimestamp"]) == pu.NOW_MS and int(m["sig_len"]) == 1
    rc, f = pu.parse_host(lib, b"xyz" + good, 0, cfg)                                         # memchr skips to the DLE
    assert rc == 1 and (f.step, f.next, f.frame_off) == (pu.STEP_FRAME, 3 + len(good), 3)
    rc, f = pu.parse_host(lib, pu.frame(long_, secs=0xFFFFFFFF, nanos=0xFFFFFFFF), 0, cfg)
    assert rc == 1 and int(np.frombuffer(bytes(f.msg), dtype=pu.MSG)[0]["timestamp"]) == 0xFFFFFFFF * 1000000000 + 0xFFFFFFFF
    for s, step, nxt, off in ((b"xyz", pu.STEP_END, 0, 0), (D, pu.STEP_SKIP, 1, 0), (D + D + b"\xc1", pu.STEP_SKIP, 1, 0), (D + E + good, pu.STEP_SKIP, 1, 0),
                              (b"ab" + D + E, pu.STEP_SKIP, 3, 0), (good[:-1], pu.STEP_INCOMPLETE, 0, 0), (b"q" + good[:-2], pu.STEP_INCOMPLETE, 0, 1),
                              (pu.frame(long_, pid=0x41) + good, pu.STEP_OTHER, len(pu.frame(long_, pid=0x41)), 0), (D + b"\x41" + D + D + E + good, pu.STEP_OTHER, 5, 0),
                              (D + b"\xc1" + D + E[:0], pu.STEP_INCOMPLETE, 0, 0)):
        rc, f = pu.parse_host(lib, s, 0, cfg)
        assert rc == 0 and (f.step, f.next, f.frame_off, f.cls) == (step, nxt, off, 0), s
    # the 4-byte frame: the decode runs through its own end; at the end of the buffer it reads zeros, past it
    rc, f = pu.parse_host(lib, pu.TINY + good, 0, ac)
    assert rc == 1 and (f.step, f.next, f.past_end) == (pu.STEP_FRAME, 4, 0) and f.cls in (pu.BAD, pu.MODEAC, pu.ACCEPT, pu.COND, pu.TYPE)
    rc, f = pu.parse_host(lib, pu.TINY, 0, ac)
    assert rc == 1 and (f.cls, f.addr, f.past_end, f.signal_level) == (pu.MODEAC, 0, 1, 0.0)
    rc, f = pu.parse_host(lib, pu.TINY, 0, cfg)
    assert rc == 1 and (f.cls, f.past_end) == (pu.MODEAC_OFF, 0) and not bytes(f.msg).strip(b"\0")
    rc, f = pu.parse_host(lib, pu.frame(b"\x77\x00"), 0, ac)
    assert rc == 1 and (f.cls, f.addr) == (pu.MODEAC, 0x7700)
    for t in range(3, 16):
        assert pu.parse_host(lib, pu.frame(long_, type_=t | 0x50), 0, ac)[1].cls == pu.TYPE
    rc, f = pu.parse_host(lib, pu.frame_of_df(ru.ap(20, 0x123456, 1), type_=0xF2), 0, cfg)
    assert rc == 1 and (f.cls, f.addr, f.adder) == (pu.COND, 0x123456, 0)
    assert pu.parse_host(lib, good, len(good), cfg)[0] == pu.MGPU_E_INVAL and pu.parse_host(lib, good, 0, (3, 1, 0))[0] == pu.MGPU_E_INVAL


def test_host_walk_through_the_library(lib, golden):
    """mgpu_pf_decode_host of the built library (no GPU needed) on the golden streams, groups (d) and (d2) from the prepared filter one
    behind the other; consumed around DLE ETX, a last DLE and a frame without end; a capacity one short leaves the filter alone."""
    import readsb_amd.binding as rb
    for g in pu.GROUPS:
        for cfg in pu.CONFIGS[g]:
            f = ru.FilterModel()
            for op in pu.ops_of(g):
                f.expire() if op < 0 else f.add(op)
            res = pu.host_decode(lib, golden[pu.key(g, cfg)]["stream"], cfg, f)
            pu.compare(res, golden[pu.key(g, cfg)], (g, cfg))
            assert (res["counters"]["past_end"] != 0) == (g == "p")
            if g == "d":
                assert (f.bits, f.occupied, len(f.inactive)) == (10, len(f.active), 0) and len(f.active) == 40 + 150 + 2
                pu.compare(pu.host_decode(lib, golden[pu.key("d2", cfg)]["stream"], cfg, f), golden[pu.key("d2", cfg)], "d2")
    cfg = (1, 1, 1)
    good = pu.frame(ru.es(pu.A, 3)[:14].tobytes())
    n = len(good)
    for s, consumed, nframes, skipped in ((b"", 0, 0, 0), (D, 1, 0, 0), (b"x", 0, 0, 0), (D + E, 1, 0, 0), (b"xy" + D + E + b"z", 3, 0, 0), (D + D + D + D, 4, 0, 0),
                                          (D + E + D + E, 3, 0, 0), (good + D, n + 1, 1, 0), (good + b"zzz", n, 1, 0), (good + good[:-1], n, 1, 0),
                                          (good + D + D + good[:-2], n + 2, 1, 0), (good + pu.frame(b"\x01" * 7, pid=0x41), n + len(pu.frame(b"\x01" * 7)), 1, 1),
                                          (D + b"\x41" + good + good, 2 * n + 2, 1, 1), (D + b"\xc1" + D, 0, 0, 0), (D + b"\xc1" + D + b"\x00", 0, 0, 0)):
        r = pu.host_decode(lib, s, cfg)
        assert (r["rc"], r["consumed"], r["nframes"], r["counters"]["nskipped"]) == (pu.MGPU_OK, consumed, nframes, skipped), (s, r["consumed"], r["nframes"])
    # mode_ac off: no record, nothing counted
    s = pu.frame(b"\x77\x00") + good + pu.frame(b"\x12\x34", sig=0x10)
    r = pu.host_decode(lib, s, (1, 1, 0))
    assert r["cls"].tolist() == [pu.MODEAC_OFF, pu.ACCEPT, pu.MODEAC_OFF] and r["nmsgs"] == 1 and r["counters"]["remote_received_modeac"] == 0
    r = pu.host_decode(lib, s, cfg)
    assert r["cls"].tolist() == [pu.MODEAC, pu.ACCEPT, pu.MODEAC] and r["nmsgs"] == 3 and r["counters"]["remote_received_modeac"] == 2
    # the 4-byte frame before the end of the stream: the decode reads behind the buffer, zeros
    r = pu.host_decode(lib, good + pu.TINY, cfg)
    assert r["cls"].tolist() == [pu.ACCEPT, pu.MODEAC] and r["counters"]["past_end"] == 1 and r["consumed"] == n + 4 and int(r["msgs"][1]["timestamp"]) == 0
    # a capacity one short: MGPU_E_OVERFLOW with what is needed, nothing stored beyond it, the filter as it was
    e = golden[pu.key("c", (1, 1, 0))]
    buf = np.frombuffer(e["stream"], dtype=np.uint8)
    n, nf = len(e["msgs"]), len(e["cls"])
    for mcap, fcap in ((n - 1, nf), (n, nf - 1)):
        arrays = pu.new_arrays(len(e["stream"]))
        outs, cn = pu.new_outs(), rb.PfInCounters()
        a = pu.pf_args(rb, buf.ctypes.data, buf.size, arrays, outs, cn, msgs_cap=mcap, frames_cap=fcap)
        ga, gi = np.zeros(buf.size, dtype=np.uint32), np.zeros(1, dtype=np.uint32)
        flt = rb.RawInFilter(ga.ctypes.data, gi.ctypes.data, 0, 0, 0, 8)
        kcfg = rb.RawInConfig(C.sizeof(rb.RawInConfig), 1, 1, 0)
        assert lib.mgpu_pf_decode_host(C.byref(a), C.byref(kcfg), C.byref(flt)) == pu.MGPU_E_OVERFLOW
        assert (int(outs[2].value), int(outs[1].value)) == (n, nf) and (flt.n_active, flt.occupied, flt.table_bits) == (0, 0, 8)
        assert arrays["msgs"][:mcap].tobytes() == e["msgs"][:mcap].tobytes() and not arrays["msgs"][mcap:].tobytes().strip(b"\0") and not arrays["cls"][fcap:].any()
        a.msgs_cap, a.frames_cap = n, nf
        assert lib.mgpu_pf_decode_host(C.byref(a), C.byref(kcfg), C.byref(flt)) == pu.MGPU_OK and flt.n_active > 30


def test_passes_give_the_whole_call(lib, golden):
    """The passes of the host form (stream_passes, here over the sequential walk) with pass_bytes small enough to cut inside frames,
    between a DLE and the byte that decides it, and inside the 53 bytes a handler call reads: exactly the result of one call over the
    whole stream, past_end included."""
    rng = np.random.default_rng(8)
    good = pu.frame(ru.es(pu.A, 3)[:14].tobytes())
    streams = [(golden[pu.key("a", (1, 1, 1))]["stream"][:9000], (1, 1, 1)), (golden[pu.key("p", (1, 1, 1))]["stream"][-3000:], (1, 1, 1)),
               (good + D + b"\x41" + bytes(700) + D + E + pu.TINY * 5 + good + D, (1, 1, 1)), (pu.draw_stream(rng, 300, 0.5), (2, 1, 0)),
               (pu.draw_automaton_stream(rng, 3000), (1, 1, 1)), (good * 3 + pu.TINY, (1, 1, 1))]
    for stream, cfg in streams:
        whole = pu.host_decode(lib, stream, cfg)
        assert whole["rc"] == pu.MGPU_OK
        for pass_bytes in (1, 7, 33, 64, 100, 1000):
            pu.same(pu.host_decode(lib, stream, cfg, pass_bytes=pass_bytes), whole, (pass_bytes, len(stream)))


@pytest.mark.skipif(not pu.have_ref_full(), reason="needs the reference tree and the objects of oracle/_ref/full")
def test_live_reference_equals_the_golden_and_the_host_walk(tmp_path, golden, lib):
    """tests/host_stub/pf_in_ref_harness.c, which includes the reference's net_io.c, leaves the golden's results; and the library's
    sequential walk equals it on 3600 drawn streams (damaged traffic, and streams over the framer's five bytes), 300 per configuration
    of nfix_crc, fixDF and mode_ac, each configuration's streams one behind the other against one filter."""
    exe = pu.build_ref_harness(str(tmp_path))
    for g in pu.GROUPS:
        for cfg in pu.CONFIGS[g]:
            streams = [golden[pu.key(g, cfg)]["stream"]] + ([golden[pu.key("d2", cfg)]["stream"]] if g == "d" else [])
            for name, res in zip((g, "d2"), pu.run_ref_harness(exe, streams, cfg, str(tmp_path), ops=pu.ops_of(g))):
                e = golden[pu.key(name, cfg)]
                for k in ("head", "cls", "off", "frame_of", "signal", "msgs"):
                    assert res[k].tobytes() == np.asarray(e[k]).astype(res[k].dtype).tobytes(), (name, cfg, k)
    rng = np.random.default_rng(99)
    for cfg in pu.ALL_CONFIGS:
        streams = [pu.draw_stream(rng, int(rng.integers(3, 40)), hostile=float(rng.uniform(0, 0.8))) for _ in range(200)]
        streams += [pu.draw_automaton_stream(rng, int(rng.integers(1, 300))) for _ in range(100)]
        f = ru.FilterModel()
        for k, res in enumerate(pu.run_ref_harness(exe, streams, cfg, str(tmp_path))):
            pu.compare(pu.host_decode(lib, streams[k], cfg, f), res, (cfg, k))
