"""Beast input on the CPU: readsb_amd/csrc/beast_in_format.h — the framer and parser the kernels of kernels/beast_in.inc run — and
beast_in_host.cpp's sequential walk, compiled for the host and run, in their own process, against what the reference's readBeast +
decodeBinMessage left (tests/golden/beast_in_cases.npz); every prefix of hostile streams under ASan and UBSan; the host entries of the
built library, the passes of the host form among them; the golden file and a few thousand drawn streams against the live reference
where its objects exist."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import beast_in_util as bu
import helpers
import raw_in_util as ru

sys.path.insert(0, os.path.join(helpers.ROOT, "tests", "golden"))
import make_beast_in_golden as maker  # noqa: E402

SAN = ("-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")


@pytest.fixture(scope="module")
def golden():
    return bu.load_golden()


@pytest.fixture(scope="module")
def lib():
    import readsb_amd.binding as rb
    return rb.load_library()


def hostile_streams():
    """Short streams whose every prefix is walked: the maximal frame, abandoned prefixes and bodies, stops, runs of 0x1a, the tail rule."""
    good = bu.frame(ru.es(bu.A, 3)[:14].tobytes())
    rng = np.random.default_rng(5)
    return [bu.MAXIMAL + bu.MAXIMAL[:30] + bu.MAXIMAL,
            b"\x1a\xe3" + b"\x1a" * 9 + good + b"\x1a\xe3\x00\x1a\x31" + good + bu.prefix(5) + b"\x1a\xe4" + good,
            good[:9] + good + b"\x1a" * 7 + good + b"\x1aW" + b"\x1a\xe8" + bytes(8) + good,
            b"\x1a\xe8" + bytes(3) + b"\x1a\x1a\x1a5" + bytes(300) + good + bytes(257),
            bu.draw_stream(rng, 12, hostile=1.0), bu.draw_stream(rng, 12, hostile=2.0)]


def _check_all(exe, tmp_path, golden):
    for g in bu.GROUPS:
        for cfg in bu.CONFIGS[g]:
            e = golden[bu.key(g, cfg)]
            out = maker.run_check(exe, e["stream"], cfg, bu.ops_of(g), e, str(tmp_path))
            assert out.split()[:5] == ["ok", "frames", str(int(e["head"][1])), "msgs", str(len(e["msgs"]))], (g, cfg, out)


def test_framer_parser_and_walk_equal_the_reference(tmp_path, golden):
    """The sequential walk gives the reference's counts, counters, class and offset per handler call and, with == on bytes, every
    record, receiver id, handler-call index and signal double of every golden stream; and agrees with a walk over
    mgpu_beast_parse_host alone on every prefix of the hostile streams."""
    exe = maker.build_check(str(tmp_path))
    _check_all(exe, tmp_path, golden)
    for s in hostile_streams():
        for cfg in ((1, 1, 1, 0), (1, 1, 0, 1)):
            assert maker.run_prefixes(exe, s, cfg, str(tmp_path)).split()[2] == str(len(s) + 1)


def test_framer_and_parser_under_sanitizers(tmp_path, golden):
    """The same stand-alone program built with ASan and UBSan, host only, run directly: the golden streams and every prefix of the
    hostile ones, each in a heap copy of exactly its bytes."""
    exe = maker.build_check(str(tmp_path), extra=SAN, name="beast_in_format_check_san")
    _check_all(exe, tmp_path, golden)
    for s in hostile_streams():
        assert maker.run_prefixes(exe, s, (1, 1, 1, 0), str(tmp_path)).split()[2] == str(len(s) + 1)


def test_golden_is_what_the_generators_build(golden):
    """The golden's streams are the seeded generators', a few tiles each; the reference's counters add up, every record carries the
    stamp, the accepted handler calls are the messages' sources; the file is no larger than the raw input's."""
    groups = bu.build_groups()
    for g, cfgs in bu.CONFIGS.items():
        for cfg in cfgs:
            e = golden[bu.key(g, cfg)]
            assert e["stream"] == bu.stream_of(groups[g]), g
            head = [int(x) for x in e["head"]]
            assert head[0] <= len(e["stream"]) and head[1] == len(e["cls"]) == len(e["off"]) and head[2] == len(e["msgs"]) == len(e["frame_of"]) == len(e["ids"]) == len(e["signal"])
            assert head[3] == head[5] + head[6] + sum(head[7:10]), (g, cfg, head)
            assert head[4] == int(np.isin(e["cls"], (bu.MODEAC, bu.MODEAC_OFF)).sum()) and head[2] == int((e["cls"] == bu.MODEAC).sum()) + sum(head[7:10])
            assert (e["msgs"]["sysTimestamp"] == bu.NOW_MS).all() and (e["msgs"]["score"] == 0).all() and (e["msgs"]["sig_len"] == 1).all()
            assert (np.nonzero(np.isin(e["cls"], (bu.ACCEPT, bu.MODEAC)))[0] == e["frame_of"]).all(), (g, cfg)
            assert (np.diff(e["off"].astype(np.int64)) >= 5).all() and (np.frombuffer(e["stream"], dtype=np.uint8)[e["off"].astype(np.int64)] == 0x1A).all()
            if g != "d2":
                assert 3 * bu.TILE <= len(e["stream"]) <= 5.5 * bu.TILE, (g, len(e["stream"]))
    assert os.path.getsize(bu.GOLDEN) <= os.path.getsize(ru.GOLDEN)


def test_abi_version_and_struct_sizes():
    """MGPU_ABI_VERSION is still 6; the binding's mirrors have the header's sizes; the classes the filter passes share are MGPU_RAW_*'s."""
    import readsb_amd.binding as rb
    text = open(os.path.join(helpers.ROOT, "include", "modes_gpu.h")).read()
    assert re.search(r"^#define MGPU_ABI_VERSION 6$", text, flags=re.M) and rb.ABI_VERSION == 6
    assert C.sizeof(rb.BeastInArgs) == 176 and C.sizeof(rb.BeastInCounters) == 80 and C.sizeof(rb.BeastInConfig) == 24 and C.sizeof(rb.BeastInFrame) == 128
    for name, value in (("MODEAC", 1), ("BAD", 2), ("ACCEPT", 3), ("COND", 4), ("UNKNOWN", 5), ("MODEAC_OFF", 6), ("POSITION", 7), ("PONG", 8)):
        assert re.search(r"^#define MGPU_BEAST_IN_%s +%du" % (name, value), text, flags=re.M), name
    for name in ("MODEAC", "BAD", "ACCEPT", "COND", "UNKNOWN"):
        assert getattr(bu, name) == getattr(ru, name)
    for name, value in (("END", 0), ("SYNTH", 1), ("UUID", 2)):
        assert re.search(r"^#define MGPU_BEAST_STOP_%s +%du" % (name, value), text, flags=re.M), name


def test_parse_host_step_by_step(lib):
    """mgpu_beast_parse_host: the successor, the kind and what a step carries, for each kind of step."""
    cfg, ac = (1, 1, 0, 0), (1, 1, 1, 0)
    long_ = ru.es(0x4840D6, 1)[:14].tobytes()
    good = bu.frame(long_, ts=0x1A2B3C4D5E6F, sig=0x1A)
    rc, f = bu.parse_host(lib, good, 0, cfg)
    assert rc == 1 and (f.step, f.next, f.frame_off, f.cls, f.addr, f.adder, f.garbage, f.id_set) == (bu.STEP_FRAME, len(good), 0, bu.ACCEPT, 0x4840D6, 1, 0, 0)
    m = np.frombuffer(bytes(f.msg), dtype=bu.MSG)[0]
    assert int(m["timestamp"]) == 0x1A2B3C4D5E6F and bytes(m["raw"]) == long_ and int(m["sig_sumsq"]) == (257 * 0x1A) ** 2 and f.signal_level == (0x1A / 255.0) * (0x1A / 255.0)
    rc, f = bu.parse_host(lib, bu.prefix(0x1A00000000001A00) + good, 0, cfg)
    assert rc == 1 and (f.step, f.next, f.frame_off, f.id_set, f.receiver_id) == (bu.STEP_FRAME, 12 + len(good), 12, 1, 0x1A00000000001A00)
    rc, f = bu.parse_host(lib, bu.prefix(7) + good, 0, (1, 1, 0, 1))                           # net_ingest: framed, the id not taken
    assert rc == 1 and (f.id_set, f.frame_off) == (0, 10)
    rc, f = bu.parse_host(lib, bu.prefix(7) + b"xy" + good, 0, cfg)                            # a prefix without a frame behind it
    assert rc == 0 and (f.step, f.next, f.id_set, f.receiver_id, f.garbage) == (bu.STEP_SKIP, 10, 1, 7, 0)
    rc, f = bu.parse_host(lib, b"\x1a\xe3\x01\x1a\x31" + bytes(20), 0, cfg)                    # an id byte 0x1a and another byte: som BEHIND the 0x1a
    assert rc == 0 and (f.step, f.next, f.garbage, f.id_set) == (bu.STEP_SKIP, 4, 4, 0)
    rc, f = bu.parse_host(lib, b"\x1a\x33\x01\x02\x1a\x33" + bytes(30), 0, cfg)                # a body's 0x1a and another byte: som ON the 0x1a
    assert rc == 0 and (f.step, f.next, f.garbage) == (bu.STEP_SKIP, 4, 4)
    for s, step, nxt, garbage, cmd in ((b"\x1aWO...", bu.STEP_SKIP, 2, 0, 1), (b"\x1a4....", bu.STEP_SKIP, 2, 2, 0), (b"\x1a\x1a33", bu.STEP_SKIP, 2, 2, 0),
                                       (b"x\x1a33", bu.STEP_GARBAGE, 1, 1, 0), (b"\x1a", bu.STEP_INCOMPLETE, 0, 0, 0), (good[:-1], bu.STEP_INCOMPLETE, 0, 0, 0),
                                       (b"\x1a\xe4" + bytes(40), bu.STEP_UUID, 0, 0, 0), (b"\x1a\xe8" + bytes(8), bu.STEP_SYNTH, 0, 0, 0),
                                       (b"\x1a\xe8" + bytes(7), bu.STEP_INCOMPLETE, 0, 0, 0), (bu.prefix(9)[:-1] + b"\x00", bu.STEP_INCOMPLETE, 0, 0, 0)):
        rc, f = bu.parse_host(lib, s, 0, cfg)
        assert rc == 0 and (f.step, f.next, f.garbage, f.command) == (step, nxt, garbage, cmd), s
    rc, f = bu.parse_host(lib, bu.prefix(9) + b"\x1a\xe4" + bytes(40), 0, cfg)                 # behind a taken prefix: the stop is the inner 0x1a
    assert rc == 0 and (f.step, f.next, f.id_set, f.receiver_id) == (bu.STEP_UUID, 10, 1, 9)
    rc, f = bu.parse_host(lib, bu.prefix(9) + b"\x1a\xe8" + bytes(40), 0, cfg)                 # ... where 0xe8 is an unknown type
    assert rc == 0 and (f.step, f.next, f.garbage) == (bu.STEP_SKIP, 12, 2)
    rc, f = bu.parse_host(lib, bu.prefix(9) + good[:5], 0, cfg)                                # incomplete behind a taken prefix: the inner 0x1a, the id stays
    assert rc == 0 and (f.step, f.next, f.id_set) == (bu.STEP_INCOMPLETE, 10, 1)
    rc, f = bu.parse_host(lib, bu.frame(b"\x77\x00"), 0, cfg)
    assert rc == 1 and f.cls == bu.MODEAC_OFF and not bytes(f.msg).strip(b"\0")
    rc, f = bu.parse_host(lib, bu.frame(b"\x77\x00"), 0, ac)
    assert rc == 1 and (f.cls, f.addr) == (bu.MODEAC, 0x7700)
    assert bu.parse_host(lib, bu.position(), 0, cfg)[1].cls == bu.POSITION and bu.parse_host(lib, bu.pong(), 0, cfg)[1].cls == bu.PONG
    rc, f = bu.parse_host(lib, bu.frame_of_df(ru.ap(20, 0x123456, 1)), 0, cfg)
    assert rc == 1 and (f.cls, f.addr, f.adder) == (bu.COND, 0x123456, 0)
    assert bu.parse_host(lib, good, len(good), cfg)[0] == bu.MGPU_E_INVAL and bu.parse_host(lib, good, 0, (3, 1, 0, 0))[0] == bu.MGPU_E_INVAL


def test_host_walk_through_the_library(lib, golden):
    """mgpu_beast_decode_host of the built library (no GPU needed) on the golden streams, groups (d) and (d2) from the prepared filter
    one behind the other; stops; tails; a capacity one short leaves the filter alone."""
    import readsb_amd.binding as rb
    for g in bu.GROUPS:
        for cfg in bu.CONFIGS[g]:
            f = ru.FilterModel()
            for op in bu.ops_of(g):
                f.expire() if op < 0 else f.add(op)
            bu.compare(bu.host_decode(lib, golden[bu.key(g, cfg)]["stream"], cfg, f), golden[bu.key(g, cfg)], (g, cfg))
            if g == "d":
                assert (f.bits, f.occupied, len(f.inactive)) == (10, len(f.active), 0) and len(f.active) == 40 + 150 + 2
                bu.compare(bu.host_decode(lib, golden[bu.key("d2", cfg)]["stream"], cfg, f), golden[bu.key("d2", cfg)], "d2")
    cfg = (1, 1, 1, 0)
    good = bu.frame(ru.es(bu.A, 3)[:14].tobytes())
    # stops: the first on the chain wins; the same bytes in a payload or in garbage stop nothing
    inert = bu.frame(b"\x1a\xe4" + bytes(12)) + b"xx\xe4\x1a\x1a\xe8" + bu.frame(b"\x1a\xe8", sig=0xE4) + good
    for stopper, kind in ((b"\x1a\xe4", bu.STOP_UUID), (b"\x1a\xe8" + bytes(8), bu.STOP_SYNTH)):
        s = inert + stopper + good + b"\x1a\xe8" + bytes(8) + b"\x1a\xe4"
        r = bu.host_decode(lib, s, cfg)
        assert (r["rc"], r["stop"], r["stop_off"], r["consumed"]) == (bu.MGPU_OK, kind, len(inert), len(inert)) and r["nframes"] == 3, r
    r = bu.host_decode(lib, inert, cfg)
    assert (r["stop"], r["consumed"], r["nframes"]) == (bu.STOP_END, len(inert), 3)
    # tails: a trailing run without 0x1a of 256 bytes stays, of 257 is garbage and consumed; 0, 1 and 2 bytes
    for n, consumed, garbage in ((256, len(good), 0), (257, len(good) + 257, 257)):
        r = bu.host_decode(lib, good + bytes(n), cfg)
        assert (r["consumed"], r["counters"]["remote_malformed_beast"], r["nmsgs"]) == (consumed, garbage, 1)
    for s, consumed in ((b"", 0), (b"\x1a", 0), (b"x", 0), (b"\x1a3", 0), (b"x\x1a", 1), (b"xy", 0), (b"\x1aW", 2)):
        r = bu.host_decode(lib, s, cfg)
        assert (r["rc"], r["consumed"], r["nframes"], r["id_out"]) == (bu.MGPU_OK, consumed, 0, bu.ID_IN), s
    for cut in range(1, bu.MAX_FRAME):                                                       # the maximal frame cut at each of its lengths
        r = bu.host_decode(lib, good + bu.MAXIMAL[:cut], cfg)
        assert (r["consumed"], r["nframes"]) == (len(good) + (18 if cut >= 20 else 0), 1), cut
        assert r["id_out"] == (0x1A1A1A1A1A1A1A1A if cut >= 20 else bu.ID_IN)
    # a capacity one short: MGPU_E_OVERFLOW with what is needed, nothing stored beyond it, the filter as it was
    e = golden[bu.key("c", (1, 1, 0, 0))]
    buf = np.frombuffer(e["stream"], dtype=np.uint8)
    n, nf = len(e["msgs"]), len(e["cls"])
    for mcap, fcap in ((n - 1, nf), (n, nf - 1)):
        arrays = bu.new_arrays(len(e["stream"]))
        outs, cn = bu.new_outs(), rb.BeastInCounters()
        a = bu.beast_args(rb, buf.ctypes.data, buf.size, arrays, outs, cn, msgs_cap=mcap, frames_cap=fcap)
        ga, gi = np.zeros(buf.size, dtype=np.uint32), np.zeros(1, dtype=np.uint32)
        flt = rb.RawInFilter(ga.ctypes.data, gi.ctypes.data, 0, 0, 0, 8)
        kcfg = rb.RawInConfig(C.sizeof(rb.RawInConfig), 1, 1, 0)
        assert lib.mgpu_beast_decode_host(C.byref(a), C.byref(kcfg), C.byref(flt)) == bu.MGPU_E_OVERFLOW
        assert (int(outs[2].value), int(outs[1].value)) == (n, nf) and (flt.n_active, flt.occupied, flt.table_bits) == (0, 0, 8)
        assert arrays["msgs"][:mcap].tobytes() == e["msgs"][:mcap].tobytes() and not arrays["msgs"][mcap:].tobytes().strip(b"\0") and not arrays["cls"][fcap:].any()
        a.msgs_cap, a.frames_cap = n, nf
        assert lib.mgpu_beast_decode_host(C.byref(a), C.byref(kcfg), C.byref(flt)) == bu.MGPU_OK and flt.n_active > 30


def test_passes_give_the_whole_call(lib, golden):
    """The passes of the host form (stream_passes, here over the sequential walk) with pass_bytes small enough to cut inside frames,
    inside prefixes and inside runs of garbage: exactly the result of one call over the whole stream."""
    import readsb_amd.binding as rb
    rng = np.random.default_rng(8)
    streams = [(golden[bu.key("a", (1, 1, 1, 0))]["stream"], (1, 1, 1, 0)), (golden[bu.key("e", (1, 1, 1, 0))]["stream"][:9000], (1, 1, 1, 0)),
               (bu.frame(b"\x12\x34") + bytes(700) + bu.MAXIMAL + bytes(257), (1, 1, 1, 0)), (bu.draw_stream(rng, 300, 0.5), (2, 1, 0, 0)),
               (bu.frame(b"\x12\x34") + bytes(300) + b"\x1a\xe4" + bytes(50), (1, 1, 1, 0))]
    for stream, cfg in streams:
        whole = bu.host_decode(lib, stream, cfg)
        for pass_bytes in (1, 7, 33, 64, 100, 1000):
            buf = np.frombuffer(bytes(stream), dtype=np.uint8)
            arrays, outs, cn = bu.new_arrays(len(stream)), bu.new_outs(), rb.BeastInCounters()
            a = bu.beast_args(rb, buf.ctypes.data, buf.size, arrays, outs, cn, net_ingest=cfg[3], pass_bytes=pass_bytes)
            ga, gi = np.zeros(buf.size, dtype=np.uint32), np.zeros(1, dtype=np.uint32)
            flt = rb.RawInFilter(ga.ctypes.data, gi.ctypes.data, 0, 0, 0, 8)
            kcfg = rb.RawInConfig(C.sizeof(rb.RawInConfig), *cfg[:3])
            assert lib.mgpu_beast_decode_host(C.byref(a), C.byref(kcfg), C.byref(flt)) == bu.MGPU_OK
            r = bu.result_of(rb, 0, arrays, outs, cn)
            for k in ("consumed", "nframes", "nmsgs", "stop", "stop_off", "id_out", "counters"):
                assert r[k] == whole[k], (pass_bytes, k, r[k], whole[k])
            for k in ("msgs", "ids", "signal", "frame_of", "cls", "off"):
                assert r[k].tobytes() == whole[k].tobytes(), (pass_bytes, k)


@pytest.mark.skipif(not bu.have_ref_full(), reason="needs the reference tree and the objects of oracle/_ref/full")
def test_live_reference_equals_the_golden_and_the_host_walk(tmp_path, golden, lib):
    """tests/host_stub/beast_in_ref_harness.c, which includes the reference's net_io.c, leaves the golden's results; and the library's
    sequential walk equals it on the golden streams and 2400 drawn ones (damaged traffic, cut in front of a stop), 100 per configuration
    of nfix_crc, fixDF, mode_ac and net_ingest, each configuration's streams one behind the other against one filter."""
    exe = bu.build_ref_harness(str(tmp_path))
    for g in bu.GROUPS:
        for cfg in bu.CONFIGS[g]:
            streams = [golden[bu.key(g, cfg)]["stream"]] + ([golden[bu.key("d2", cfg)]["stream"]] if g == "d" else [])
            for name, res in zip((g, "d2"), bu.run_ref_harness(exe, streams, cfg, str(tmp_path), ops=bu.ops_of(g))):
                e = golden[bu.key(name, cfg)]
                for k in ("head", "cls", "off", "frame_of", "ids", "signal", "msgs"):
                    assert res[k].tobytes() == np.asarray(e[k]).astype(res[k].dtype).tobytes(), (name, cfg, k)
    rng = np.random.default_rng(99)
    base = [golden[bu.key(g, bu.CONFIGS[g][0])]["stream"] for g in ("a", "b", "e")]
    for cfg in bu.ALL_CONFIGS:
        streams = [bu.cut_at_stop(lib, bu.draw_stream(rng, int(rng.integers(5, 90)), hostile=float(rng.uniform(0, 0.6))), cfg) for _ in range(100)]
        streams += [bu.cut_at_stop(lib, s, cfg) for s in base]
        f = ru.FilterModel()
        for k, res in enumerate(bu.run_ref_harness(exe, streams, cfg, str(tmp_path))):
            bu.compare(bu.host_decode(lib, streams[k], cfg, f), res, (cfg, k))
