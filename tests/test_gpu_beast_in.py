"""-m gpu: beast input on the device (kernels/beast_in.inc, mgpu_beast_decode / mgpu_beast_decode_device): the accepted messages, their
receiver ids, handler calls and signal doubles' bit patterns, the class and offset of every handler call, the counts, the stop and the
counters compared with == on bytes against what the reference's readBeast + decodeBinMessage left (tests/golden/beast_in_cases.npz)
and, for built streams, against the library's sequential walk (tests/test_beast_in_reference.py holds both to the live reference on
the CPU).  Every output array sits between canaries and both forms are run.

Shapes: a tile is 8192 bytes, a lane takes the steps that start in 32 of them, a step reaches at most 62 bytes so a tile has 64 entry
offsets (its halo), a load is 16 bytes, 64 tiles' exit maps are composed into one group; the filter passes over the candidates run in
workgroups of 256.  The golden groups are 3 to 5 tiles; the tile-edge streams are three tiles at every misalignment of the data."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import beast_in_util as bu
import beast_util as hu
import helpers
import raw_in_util as ru

pytestmark = pytest.mark.gpu

GUARD = 4                                        # entries in front of and behind every array
CANARY = 0xA5A5A5A5A5A5A5A5
EXTERNAL = 2                                     # MGPU_FILTER_CLOCK_EXTERNAL: the filter starts empty, as the harness's does
CLI = os.path.join(helpers.ROOT, "readsb_amd", "host", "readsb_gpu_beast_in")
BEHIND = b"\x1a3" + bytes(21) + b"\x1a\xe4"       # bytes behind the stream: nothing of them may count
LONG = ru.es(bu.A, 3)[:14].tobytes()
GOOD = bu.frame(LONG)


@pytest.fixture(scope="module")
def ctxs(built):
    import readsb_amd
    hip = hu.Hip()
    made = {}

    def get(cfg):
        k = tuple(cfg[:3])
        if k not in made:
            made[k] = readsb_amd.Demodulator(nfix_crc=k[0], fix_df=k[1], mode_ac=k[2], startup_time_ms=helpers.STARTUP_MS, max_samples=131072, filter_clock=EXTERNAL)
        made[k].reset()
        return made[k]
    try:
        yield get, hip
    finally:
        hip.free_all()
        for d in made.values():
            d.close()


@pytest.fixture(scope="module")
def golden():
    return bu.load_golden()


def prepare(d, ops):
    for op in ops:
        d.filter_expire() if op < 0 else d.filter_add(op)


def run(d, hip, form, data, cfg, msgs_cap=None, frames_cap=None, data_off=0, pass_bytes=0, id_in=bu.ID_IN, optional=True):
    """One call with every array between canaries -> bu.result_of's dict with `intact`.  cfg[3] is net_ingest."""
    from readsb_amd import binding
    data = bytes(data)
    msgs_cap = len(data) // 11 + 1 if msgs_cap is None else msgs_cap
    frames_cap = len(data) // 5 + 1 if frames_cap is None else frames_cap
    sizes = dict(msgs=(msgs_cap, 64), ids=(msgs_cap, 8), signal=(msgs_cap, 8), frame_of=(msgs_cap, 8), cls=(frames_cap, 1), off=(frames_cap, 8))
    dtypes = dict(msgs=bu.MSG, ids=np.uint64, signal=np.float64, frame_of=np.uint64, cls=np.uint8, off=np.uint64)
    src = np.frombuffer(b"\x1a" * data_off + data + BEHIND, dtype=np.uint8)
    outs, cn = bu.new_outs(), binding.BeastInCounters()
    host, ptr = {}, {}
    for k, (n, size) in sizes.items():
        nb = (n + 2 * GUARD) * size
        if form == "host":
            host[k] = np.full(nb, 0xA5, dtype=np.uint8)
            ptr[k] = host[k].ctypes.data + GUARD * size
        else:
            host[k] = hip.malloc(nb)
            hip.fill(host[k], 0xA5, nb)
            ptr[k] = host[k] + GUARD * size
    if not optional:
        ptr.update(signal=None, frame_of=None, cls=None, off=None)
    d_data = None
    if form == "host":
        dp = src.ctypes.data + data_off if data else None
    else:
        d_data = hip.upload(src)
        dp = d_data + data_off
    a = bu.beast_args(binding, dp, len(data), None, outs, cn, id_in=id_in, net_ingest=cfg[3], msgs_cap=msgs_cap, frames_cap=frames_cap if optional else 0, pass_bytes=pass_bytes,
                      pointers=ptr)
    f = d.lib.mgpu_beast_decode if form == "host" else d.lib.mgpu_beast_decode_device
    rc = int(f(d.ctx, C.byref(a)))
    raw = {}
    for k, (n, size) in sizes.items():
        nb = (n + 2 * GUARD) * size
        raw[k] = host[k] if form == "host" else hip.download(host[k], nb)
        if form != "host":
            hip.free(host[k])
    if d_data is not None:
        hip.free(d_data)
    nm = min(int(outs[2].value), msgs_cap) if rc != bu.MGPU_E_INVAL else 0
    nf = min(int(outs[1].value), frames_cap) if rc != bu.MGPU_E_INVAL else 0
    arrays, intact = {}, True
    for k, (n, size) in sizes.items():
        used = (nm if k in ("msgs", "ids", "signal", "frame_of") else nf) if (optional or k in ("msgs", "ids")) else 0
        lo, hi = GUARD * size, (GUARD + used) * size
        intact = intact and bool((raw[k][:lo] == 0xA5).all() and (raw[k][hi:] == 0xA5).all())
        arrays[k] = raw[k][lo:hi].copy().view(dtypes[k])
    res = bu.result_of(binding, rc, arrays, outs, cn)
    res["intact"] = intact
    return res


def same(res, want, what=None):
    """want: a golden entry or a result of bu.host_decode"""
    assert res["rc"] == bu.MGPU_OK and res["intact"], (what, res["rc"], res["intact"])
    if "head" in want:
        bu.compare(res, want, what)
        assert res["stop"] == bu.STOP_END and res["stop_off"] == res["consumed"]
        return
    for k in ("consumed", "nframes", "nmsgs", "stop", "stop_off", "id_out", "counters"):
        assert res[k] == want[k], (what, k, res[k], want[k])
    for k in ("msgs", "ids", "signal", "frame_of", "cls", "off"):
        assert res[k].tobytes() == want[k].tobytes(), (what, k)


def both(ctxs, data, cfg, what=None, ops=(), **kw):
    """The stream through both forms against the sequential walk -> the walk's result."""
    get, hip = ctxs
    f = ru.FilterModel()
    for op in ops:
        f.expire() if op < 0 else f.add(op)
    want = bu.host_decode(get(cfg).lib, data, cfg, f, id_in=kw.get("id_in", bu.ID_IN))
    assert want["rc"] == bu.MGPU_OK
    for form in ("device", "host"):
        d = get(cfg)
        prepare(d, ops)
        same(run(d, hip, form, data, cfg, **kw), want, (what, form))
    return want


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("group", bu.GROUPS)
def test_golden_groups(ctxs, golden, group, form):
    """Every golden group under every configuration through the C entry of either form.  After group (d) a second call with one
    Address/Parity frame per prepared address: the context's filter stands where the reference's does."""
    get, hip = ctxs
    for k, cfg in enumerate(bu.CONFIGS[group]):
        d = get(cfg)
        prepare(d, bu.ops_of(group))
        same(run(d, hip, form, golden[bu.key(group, cfg)]["stream"], cfg, data_off=5 * k), golden[bu.key(group, cfg)], (group, cfg))
        if group == "d":
            same(run(d, hip, form, golden[bu.key("d2", cfg)]["stream"], cfg), golden[bu.key("d2", cfg)], ("d2", cfg))


def edge_stream(first, traffic):
    """Three tiles of traffic (a list of frames, more than three tiles of them) with the maximal frame (62 bytes, every escapable byte
    0x1a) starting at stream position `first`."""
    head, at, k = [], 0, 0
    while at + len(traffic[k]) <= first:
        head.append(traffic[k])
        at += len(traffic[k])
        k += 1
    head.append(b"\x55" * (first - at))                                                      # garbage up to the place
    s = b"".join(head) + bu.MAXIMAL
    while len(s) < 3 * bu.TILE + 100:
        s += traffic[k]
        k += 1
    return s


def test_tile_edges(ctxs):
    """The maximal frame placed so that each of its 62 bytes in turn is the first byte of the second tile, in both forms (in the
    device form the misalignment of the data going round 0..15 with it); and one stream, the frame across the
    end of the second tile, at every misalignment 0..15."""
    get, hip = ctxs
    cfg = (1, 1, 1, 0)
    traffic = bu.pad_to([], 3 * bu.TILE + 400, np.random.default_rng(31))
    for k in range(bu.MAX_FRAME):
        s = edge_stream(bu.TILE - k, traffic)
        assert s[bu.TILE - k: bu.TILE - k + bu.MAX_FRAME] == bu.MAXIMAL and 3 * bu.TILE < len(s)
        want = bu.host_decode(get(cfg).lib, s, cfg)
        assert bu.TILE - k + 18 in want["off"].tolist() and 0x1A1A1A1A1A1A1A1A in want["ids"].tolist()
        same(run(get(cfg), hip, "device", s, cfg, data_off=k % 16), want, ("edge", k))
        same(run(get(cfg), hip, "host", s, cfg), want, ("edge host", k))
    s = edge_stream(2 * bu.TILE - 1, traffic)
    want = bu.host_decode(get(cfg).lib, s, cfg)
    for off in range(16):
        same(run(get(cfg), hip, "device", s, cfg, data_off=off), want, ("misalignment", off))


def test_escapes_and_resynchronisation(ctxs):
    """0x1a in every field position of every type, escaped and bare (a body broken by 0x1a and a type byte that starts a valid frame);
    runs of one to seven 0x1a in front of a valid frame; 0x1a and every one of the 256 second bytes (0xe4 and 0xe8, which stop, each in
    a stream of its own)."""
    parts = []
    for msg, t in ((b"\x77\x00", b"1"), (ru.df11(bu.A)[:7].tobytes(), b"2"), (LONG, b"3"), (bytes(range(0x40, 0x40 + 14)), b"3")):
        for at in range(7 + len(msg)):
            body = bytearray(int(0x0123456789AB).to_bytes(6, "big") + b"\x80" + msg)
            body[at] = 0x1A
            parts += [b"\x1a" + t + bu.esc(body), b"\x1a" + t + bytes(body[: at + 1]) + GOOD[1:], b"\x1a" + t + bytes(body), GOOD]
    for at in range(21):
        p = bytearray(range(0x40, 0x40 + 21))
        p[at] = 0x1A
        parts += [bu.position(bytes(p)), b"\x1a5" + bytes(p), GOOD]
    for at in range(3):
        p = bytearray(b"\x01\x02\x03")
        p[at] = 0x1A
        parts += [bu.pong(bytes(p)), b"\x1aP" + bytes(p), GOOD]
    for at in range(8):
        rid = bytearray(int(0x1122334455667788).to_bytes(8, "big"))
        rid[at] = 0x1A
        parts += [b"\x1a\xe3" + bu.esc(rid) + GOOD, b"\x1a\xe3" + bytes(rid) + GOOD, GOOD]
    for n in range(1, 8):
        parts += [b"\x1a" * n + GOOD, b"xyz"]
    for b in range(256):
        if b not in (0xE4, 0xE8):
            parts += [bytes([0x1A, b]), GOOD]
    s = bu.stream_of(parts)
    want = both(ctxs, s, (1, 1, 1, 0), "escapes")
    assert want["stop"] == bu.STOP_END and want["consumed"] == len(s) and want["nmsgs"] > 300 and want["counters"]["remote_malformed_beast"] > 500
    for b, kind in ((0xE4, bu.STOP_UUID), (0xE8, bu.STOP_SYNTH)):
        s = GOOD * 3 + bytes([0x1A, b]) + bytes(8) + GOOD
        want = both(ctxs, s, (1, 1, 1, 0), "second byte %02x" % b)
        assert (want["stop"], want["stop_off"], want["nmsgs"]) == (kind, 3 * len(GOOD), 3)


def test_chain_dependence_across_groups(ctxs):
    """Streams longer than one composition group of tiles, both forms.
    (1) A stream whose framing from offset 0 and from offset 1 never meet.  (A frame start — 0x1a and a type byte — resynchronises
    every chain that reaches it: inside another chain's body it abandons that frame.  Two chains stay apart only over steps that pass
    it by: a run of 0x1a, which each chain takes two bytes at a time.)  The run is followed by '3' and a frame's body: which chain is
    the one from offset 0 — the run's parity — decides whether that is a frame or garbage, and the parity has to be carried through
    every tile's and group's exit map.
    (2) Ordinary traffic with prefixes, escapes and garbage over GROUP + 2 tiles, in a unit whose length is no divisor of the tile:
    the chain enters every tile at another of its 64 entry offsets, and frames, messages and receiver ids are indexed across groups."""
    get, hip = ctxs
    cfg = (1, 1, 1, 0)
    n = (bu.GROUP + 2) * bu.TILE + 1000
    for run_len in (n, n + 1):
        s = GOOD + b"\x1a" * run_len + GOOD[1:] + GOOD
        want = both(ctxs, s, cfg, ("run", run_len))
        assert want["nmsgs"] == (3 if run_len % 2 else 2) and want["counters"]["remote_malformed_beast"] == run_len - (run_len % 2) + (0 if run_len % 2 else len(GOOD) - 1)
    unit = bu.stream_of(bu.pad_to([], bu.TILE + 900, np.random.default_rng(37), period=150))
    s = unit * ((bu.GROUP + 2) * bu.TILE // len(unit) + 1)
    assert len(s) > (bu.GROUP + 2) * bu.TILE and len(unit) % bu.TILE
    want = both(ctxs, s, cfg, "traffic over a group")
    entries = set()                                                                          # where the chain enters the tiles: the first step at or behind each tile's start
    off = want["off"].astype(np.int64)
    for t in range(1, bu.GROUP + 2):
        entries.add(int(off[np.searchsorted(off, t * bu.TILE)]) - t * bu.TILE)
    assert len(entries) > 20 and want["consumed"] > (bu.GROUP + 2) * bu.TILE and len(set(want["ids"].tolist())) > 5


def test_receiver_ids(ctxs, golden):
    """One 0xe3 at offset 0 in front of three tiles of frames; an 0xe3 in the last bytes of each tile; 0xe3 not followed by 0x1a;
    0xe3 cut at every point of the tail; the same under net_ingest."""
    rng = np.random.default_rng(41)
    plain = bu.stream_of(bu.pad_to([], 3 * bu.TILE + 50, rng, ids=False))
    for ingest in (0, 1):
        cfg = (1, 1, 1, ingest)
        want = both(ctxs, bu.prefix(0x1A2B3C4D5E6F7081) + plain, cfg, "one id")
        assert set(want["ids"].tolist()) == {bu.ID_IN if ingest else 0x1A2B3C4D5E6F7081} and want["nmsgs"] > 800
        for backs in ((1, 10, 19), (2, 9, 11)):                                              # a prefix that starts `back` bytes in front of each tile's end
            parts = []
            for tile, back in zip((1, 2, 3), backs):
                have = sum(len(x) for x in parts)
                parts.append(bu.stream_of(bu.pad_to([], tile * bu.TILE - back - have - 40, rng, ids=False)))
                have += len(parts[-1])
                parts.append(b"\x55" * (tile * bu.TILE - back - have))
                parts.append(bu.prefix(0x1A00000000000000 + 256 * tile + back) + bu.frame(LONG, sig=back))
                assert sum(len(x) for x in parts[:-1]) == tile * bu.TILE - back
            s = bu.stream_of(parts) + plain[:500] + bu.prefix(77) + b"zz" + GOOD + bu.prefix(78) + bu.prefix(79) + GOOD
            want = both(ctxs, s, cfg, ("ids at tile ends", backs))
            assert ingest or len(set(want["ids"].tolist())) >= 5
        for cut in range(1, 20):                                                             # 0xe3 cut at every point of the tail
            s = GOOD * 13 + bu.prefix(0x1A1A1A1A1A1A1A1A)[:cut]
            want = both(ctxs, s, cfg, ("cut", cut))
            assert want["consumed"] == 13 * len(GOOD) and want["id_out"] == bu.ID_IN


def test_tails_and_stops(ctxs):
    """A maximal frame cut at each of its lengths (consumed stops at its 0x1a); a trailing run without 0x1a of 256 and of 257 bytes;
    streams of 0, 1 and 2 bytes; 0xe4 and 0xe8 on the chain, the first one winning, in the first tile and in the third; the same bytes
    in payload and in garbage: no stop."""
    get, hip = ctxs
    cfg = (1, 1, 1, 0)
    rng = np.random.default_rng(43)
    for cut in range(1, bu.MAX_FRAME):
        want = both(ctxs, GOOD * 2 + bu.MAXIMAL[:cut], cfg, ("cut", cut))
        assert want["consumed"] == 2 * len(GOOD) + (18 if cut >= 20 else 0)
    for n, eaten in ((256, 0), (257, 257)):
        want = both(ctxs, GOOD + bytes(n), cfg, ("tail", n))
        assert want["consumed"] == len(GOOD) + eaten and want["counters"]["remote_malformed_beast"] == eaten
    for s in (b"", b"\x1a", b"x", b"\x1a3", b"x\x1a", b"xy", b"\x1aW"):
        both(ctxs, s, cfg, s)
    plain = bu.stream_of(bu.pad_to([], 2 * bu.TILE + 300, rng))
    inert = bu.frame(b"\x1a\xe4" + bytes(12)) + b"xx\xe4\x1a\x1a\xe8" + bu.frame(b"\x1a\xe8", sig=0xE4)
    for head in (GOOD, plain):
        for first, second, kind in ((b"\x1a\xe4", b"\x1a\xe8" + bytes(8), bu.STOP_UUID), (b"\x1a\xe8" + bytes(8), b"\x1a\xe4", bu.STOP_SYNTH)):
            s = head + inert + first + GOOD + second + GOOD
            want = both(ctxs, s, cfg, ("stop", kind, len(head)))
            assert (want["stop"], want["stop_off"]) == (kind, len(head) + len(inert))
        want = both(ctxs, head + inert + GOOD, cfg, "inert")
        assert want["stop"] == bu.STOP_END and want["consumed"] == len(head) + len(inert) + len(GOOD)
    want = both(ctxs, plain + bu.prefix(0x4242) + b"\x1a\xe4" + GOOD, cfg, "a stop behind a taken prefix")
    assert (want["stop"], want["stop_off"], want["id_out"]) == (bu.STOP_UUID, len(plain) + 10, 0x4242)


def filter_state(d, hip, addrs):
    """Which of the addresses the context's filter holds, asked with Address/Parity frames (which add nothing)."""
    stream = b"".join(bu.frame_of_df(ru.ap(4, int(a), k)) for k, a in enumerate(addrs))
    return run(d, hip, "device", stream, (1, 1, 0, 0))["cls"].tolist()


@pytest.mark.parametrize("form", ["host", "device"])
def test_filter_order_growth_and_state(ctxs, golden, form):
    """The raw input's order cases carried over as beast frames (group c: a conditional frame in front of and behind its adder, in the
    same lane's bytes and in the next tile); a foreign add (mgpu_filter_add between two calls); the growth of the table (group d: the
    reference's classes around L*); afterwards the context's filter agrees with the reference's, asked address by address."""
    get, hip = ctxs
    cfg = (1, 1, 0, 0)
    d = get(cfg)
    same(run(d, hip, form, golden[bu.key("c", cfg)]["stream"], cfg), golden[bu.key("c", cfg)], "c")
    d = get(cfg)
    foreign = 0x7B1234
    probe = bu.frame_of_df(ru.ap(4, foreign, 1)) + bu.frame_of_df(ru.ap(20, foreign, 2))
    assert run(d, hip, form, probe, cfg)["cls"].tolist() == [bu.UNKNOWN, bu.UNKNOWN]
    d.filter_add(foreign)
    assert run(d, hip, form, probe, cfg)["cls"].tolist() == [bu.ACCEPT, bu.ACCEPT]
    d = get(cfg)
    prepare(d, bu.ops_of("d"))
    g = golden[bu.key("d", cfg)]
    parts, lstar, lstar2, probes = bu.group_d_info()
    inactive = set(int(x) for x in ru.D_INACTIVE)
    assert sum(1 for ln, a, ok in probes if a in inactive and ln < lstar and ok) >= 20 and sum(1 for ln, a, ok in probes if a in inactive and ln > lstar and not ok) >= 20
    res = run(d, hip, form, g["stream"], cfg)
    same(res, g, "d")
    assert all(res["cls"][ln] == (bu.ACCEPT if ok else bu.UNKNOWN) for ln, a, ok in probes)
    asked = np.concatenate([ru.D_INACTIVE[:12], ru.D_ACTIVE[:4], ru.D_NEW[:12]])
    assert filter_state(d, hip, asked) == [bu.UNKNOWN] * 7 + [bu.ACCEPT] + [bu.UNKNOWN] * 3 + [bu.ACCEPT] + [bu.ACCEPT] * 16


def test_the_demodulator_sees_beast_learnt_addresses(ctxs):
    """The pre-screen, as tests/test_gpu_raw_in.py checks it: one capture with DF4 / DF5 frames of an address learnt only from the
    beast feed (a clean DF17 behind a receiver id, in either form), demodulated after the call, is accepted by mgpu_feed_iq; the same
    capture on a fresh context is not, nor after a call that overflowed (the filter and the pre-screen stay where they stood)."""
    import filter_util
    import frames_util as fr
    import readsb_amd
    get, hip = ctxs
    addr = 0x4CA2D6
    frames = fr.ap_frames(np.array([4, 4, 5]), addr, payload_seed=5)
    iq = filter_util.modulate_buffers([(frames, np.full(3, 56))])
    stream = bu.prefix(0x77) + bu.frame_of_df(ru.es(addr, 1)) + GOOD
    got = {}
    for how in ("fresh", "overflow", "host", "device"):
        d = readsb_amd.Demodulator(startup_time_ms=helpers.STARTUP_MS, max_samples=8 * helpers.BUF_SAMPLES, filter_clock=EXTERNAL)
        try:
            if how == "overflow":
                res = run(d, hip, "device", stream, (1, 1, 0, 0), msgs_cap=1)
                assert res["rc"] == bu.MGPU_E_OVERFLOW and res["nmsgs"] == 2 and res["intact"]
            elif how != "fresh":
                res = run(d, hip, how, stream, (1, 1, 0, 0))
                assert res["rc"] == bu.MGPU_OK and res["cls"].tolist() == [bu.ACCEPT, bu.ACCEPT] and res["ids"].tolist() == [0x77, 0x77]
            got[how] = d.demodulate_capture(iq)[0]
        finally:
            d.close()
    assert len(got["fresh"]) == 0 and len(got["overflow"]) == 0
    for how in ("host", "device"):
        assert len(got[how]) == 3 and (got[how]["addr"] == addr).all() and got[how]["msg"].tobytes() == frames[:, :14].tobytes(), how


def test_modeac_off_is_counted_and_leaves_no_record(ctxs):
    s = bu.frame(b"\x77\x00") + GOOD + bu.frame(b"\x12\x34", sig=0x1A) + bu.prefix(5) + bu.frame(b"\x00\x00")
    want = both(ctxs, s, (1, 1, 0, 0), "mode_ac off")
    assert want["cls"].tolist() == [bu.MODEAC_OFF, bu.ACCEPT, bu.MODEAC_OFF, bu.MODEAC_OFF] and want["nmsgs"] == 1 and want["counters"]["remote_received_modeac"] == 3
    want = both(ctxs, s, (1, 1, 1, 0), "mode_ac on")
    assert want["cls"].tolist() == [bu.MODEAC, bu.ACCEPT, bu.MODEAC, bu.MODEAC] and want["nmsgs"] == 4 and want["counters"]["remote_received_modeac"] == 3


@pytest.mark.parametrize("form", ["host", "device"])
def test_capacities_one_short(ctxs, golden, form):
    """msgs_cap and the frame capacity exact, then each one short: MGPU_E_OVERFLOW with the needed counts, the canaries intact, nothing
    stored at or beyond a capacity, the filter untouched; then the same call with room gives the golden.  The optional arrays left out."""
    get, hip = ctxs
    cfg = (1, 1, 0, 0)
    g = golden[bu.key("d", cfg)]
    need, nframes = len(g["msgs"]), len(g["cls"])
    asked = np.concatenate([ru.D_INACTIVE[:12], ru.D_ACTIVE[:4], ru.D_NEW[:12]])
    d = get(cfg)
    prepare(d, bu.ops_of("d"))
    state0 = filter_state(d, hip, asked)
    assert state0 == [bu.ACCEPT] * 16 + [bu.UNKNOWN] * 12
    for kw in (dict(msgs_cap=need - 1), dict(frames_cap=nframes - 1), dict(msgs_cap=7, frames_cap=3), dict(msgs_cap=need // 2, pass_bytes=9000)):
        if "pass_bytes" in kw and form == "device":
            continue
        res = run(d, hip, form, g["stream"], cfg, **{**dict(msgs_cap=need, frames_cap=nframes), **kw})
        assert res["rc"] == bu.MGPU_E_OVERFLOW and res["intact"], kw
        assert (res["nmsgs"], res["nframes"], res["consumed"]) == (need, nframes, int(g["head"][0])), kw
        assert res["msgs"].tobytes() == g["msgs"][: len(res["msgs"])].tobytes() and res["ids"].tobytes() == g["ids"][: len(res["ids"])].tobytes(), kw
        assert res["cls"].tobytes() == g["cls"][: len(res["cls"])].tobytes() and res["off"].tobytes() == g["off"][: len(res["off"])].tobytes(), kw
        assert filter_state(d, hip, asked) == state0, kw                                     # the filter is where it stood
    res = run(d, hip, form, g["stream"], cfg, msgs_cap=need, frames_cap=nframes, optional=False)
    assert res["rc"] == bu.MGPU_OK and res["intact"] and res["msgs"].tobytes() == g["msgs"].tobytes() and res["ids"].tobytes() == g["ids"].tobytes()
    d = get(cfg)
    prepare(d, bu.ops_of("d"))
    same(run(d, hip, form, g["stream"], cfg, msgs_cap=need, frames_cap=nframes), g, "exact")


def test_host_passes_and_bad_arguments(ctxs, golden):
    """The host form with pass_bytes that cut inside frames (down to 1: every pass grows until it reaches a som) gives the bytes of
    one call; the binding's beast_decode gives the golden; MGPU_E_INVAL as documented."""
    from readsb_amd import binding
    get, hip = ctxs
    cfg = (1, 1, 1, 0)
    g = golden[bu.key("a", cfg)]
    for pass_bytes in (len(g["stream"]) // 3 + 1, bu.TILE, 1000):
        same(run(get(cfg), hip, "host", g["stream"], cfg, pass_bytes=pass_bytes), g, pass_bytes)
    part = g["stream"][:2500]
    same(run(get(cfg), hip, "host", part, cfg, pass_bytes=1), bu.host_decode(get(cfg).lib, part, cfg), 1)
    d = get(cfg)
    res = d.beast_decode(g["stream"], now_ms=bu.NOW_MS, receiver_id=bu.ID_IN)
    assert res["msgs"].tobytes() == g["msgs"].tobytes() and res["receiver_id"].tobytes() == g["ids"].tobytes() and res["frame_class"].tobytes() == g["cls"].tobytes()
    assert res["signal_level"].tobytes() == g["signal"].tobytes() and res["consumed"] == int(g["head"][0]) and res["counters"]["remote_malformed_beast"] == int(g["head"][10])
    buf = np.frombuffer(GOOD * 3, dtype=np.uint8)
    for form in ("host", "device"):
        f = d.lib.mgpu_beast_decode if form == "host" else d.lib.mgpu_beast_decode_device
        arrays, outs, cn = bu.new_arrays(buf.size), bu.new_outs(), binding.BeastInCounters()
        dp = buf.ctypes.data if form == "host" else hip.upload(buf)
        dev = {k: hip.malloc(v.nbytes) for k, v in arrays.items()} if form == "device" else None

        def args(**kw):
            a = bu.beast_args(binding, dp, buf.size, arrays, outs, cn, pointers=dev)
            for k, v in kw.items():
                setattr(a, k, v)
            return C.byref(a)
        assert f(d.ctx, args()) == bu.MGPU_OK and int(outs[2].value) == 3
        assert f(None, None) == bu.MGPU_E_INVAL and f(d.ctx, None) == bu.MGPU_E_INVAL
        for kw in (dict(size=C.sizeof(binding.BeastInArgs) - 8), dict(size=0), dict(data=None), dict(msgs=None), dict(receiver_id=None), dict(counters=None), dict(stop=None),
                   dict(receiver_id_out=None), dict(frame_class=None, frame_off=None), dict(now_ms=-1), dict(now_ms=253402300800000), dict(nbytes=1 << 32)):
            assert f(d.ctx, args(**kw)) == bu.MGPU_E_INVAL, (form, kw)
        if form == "device":
            assert f(d.ctx, args(msgs=dev["msgs"] + 4)) == bu.MGPU_E_INVAL                      # records off their alignment
            hip.free(dp)
            for p in dev.values():
                hip.free(p)
        assert f(d.ctx, args(nbytes=0, data=None)) == bu.MGPU_OK and [int(x.value) for x in outs] == [0, 0, 0, 0, 0, bu.ID_IN]


def test_round_trip_through_the_encoder(ctxs, golden):
    """mgpu_beast_encode_ex with ids and --verbatim over a record list, then mgpu_beast_decode with a filter that knows every address:
    the records' raw, timestamps, signal bytes and ids come back unchanged."""
    get, hip = ctxs
    cfg = (1, 1, 1, 0)
    e = golden[bu.key("e", cfg)]
    msgs, ids = e["msgs"], e["ids"]
    d = get(cfg)
    stream = bytes(d.beast_encode_ex(msgs, verbatim=True, ids=ids)[0])
    d = get(cfg)
    for a in set(int(x) for x in msgs["addr"][msgs["msgtype"] != 77]):
        d.filter_add(a)
    for form in ("device", "host"):
        res = run(d, hip, form, stream, cfg, id_in=0)
        assert res["rc"] == bu.MGPU_OK and res["intact"] and res["nmsgs"] == len(msgs) and res["consumed"] == len(stream) and res["counters"]["remote_malformed_beast"] == 0
        assert res["msgs"]["raw"].tobytes() == msgs["raw"].tobytes() and (res["msgs"]["timestamp"] == msgs["timestamp"]).all() and (res["msgs"]["sig_sumsq"] == msgs["sig_sumsq"]).all()
        assert res["ids"].tobytes() == ids.tobytes()


def test_command_line_against_the_library(ctxs, golden):
    """readsb_gpu_beast_in as a child process on a golden stream: its output equals the encoder's over the expected records with their
    ids, with a block smaller than the stream so that frames, the id and the filter are carried between calls; the counters on stderr.
    A UUID frame is reported, skipped on the host, and the stream goes on."""
    get, hip = ctxs
    for g, cfg, flags, block in (("a", (1, 1, 1, 0), ["--fix", "--mode-ac"], 3000), ("e", (1, 1, 1, 1), ["--mode-ac", "--net-ingest", "--verbatim"], 1 << 20)):
        e = golden[bu.key(g, cfg)]
        stream = e["stream"]
        want = bu.host_decode(get(cfg).lib, stream, cfg, id_in=0)
        enc = bytes(get(cfg).beast_encode_ex(want["msgs"], verbatim="--verbatim" in flags, ids=want["ids"])[0])
        r = subprocess.run([CLI, *flags, "--now", str(bu.NOW_MS), "--block", str(block)], input=stream, capture_output=True, timeout=120)
        assert r.returncode == 0, r.stderr[-500:]
        assert r.stdout == enc, (g, cfg, len(r.stdout), len(enc))
        words = r.stderr.decode().split()
        assert words[:4] == ["frames", str(want["nframes"]), "messages", str(want["nmsgs"])] and words[words.index("remote_malformed_beast") + 1] == str(want["counters"]["remote_malformed_beast"])
    cfg = (1, 1, 1, 0)
    # stops are reported and stepped over as the reference steps over them: a UUID's 32 digits with their dashes, a synthetic time's
    # eight bytes as they stand (here they spell the start of a frame); a UUID cut short by a 0x1a loses that 0x1a, as in read_uuid
    uuid = b"01234567-89ab-cdef-0123-456789ABCDEF"
    stream = GOOD * 2 + b"\x1a\xe4" + uuid + GOOD + b"\x1a\xe8" + GOOD[:8] + GOOD + b"\x1a\xe4" + b"0123" + GOOD + GOOD
    r = subprocess.run([CLI, "--mode-ac", "--now", str(bu.NOW_MS), "--block", "64"], input=stream, capture_output=True, timeout=120)
    want = bu.host_decode(get(cfg).lib, GOOD * 5, cfg, id_in=0)
    err = r.stderr.decode()
    assert r.returncode == 0 and r.stdout == bytes(get(cfg).beast_encode_ex(want["msgs"], ids=want["ids"])[0]), err
    assert "UUID (0xe4) frame at byte %d: skipped 38 bytes" % (2 * len(GOOD)) in err and "synthetic timestamp (0xe8) frame at byte %d: skipped 10 bytes" % (3 * len(GOOD) + 38) in err
    assert "UUID (0xe4) frame at byte %d: skipped 7 bytes" % (4 * len(GOOD) + 48) in err
    words = err.splitlines()[-1].split()                                                      # the counters' line
    assert words[words.index("stops") + 1] == "3" and words[words.index("skipped") + 1] == "55" and words[words.index("remote_malformed_beast") + 1] == str(len(GOOD) - 1)
