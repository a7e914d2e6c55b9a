"""-m gpu: Planefinder input on the device (kernels/pf_in.inc, mgpu_pf_decode / mgpu_pf_decode_device): the accepted messages, their
handler calls and signal doubles' bit patterns, the class and offset of every handler call, the counts and the counters compared with
== on bytes against what the reference's readPlanefinder + decodePfMessage left (tests/golden/pf_in_cases.npz) and, for built streams,
against the library's sequential walk (tests/test_pf_in_reference.py holds both to the live reference on the CPU).  Every output array
sits between canaries and both forms are run.

Shapes: a tile is 8192 bytes, a lane takes the 32 of them whose DLEs it judges with one byte of lookahead, a load is 16 bytes, a
handler call reads at most 53 bytes from its start; the framer's state crosses lanes by a ballot, waves through LDS and tiles through
one scan by 256 threads; the filter passes over the candidates run in workgroups of 256.  The golden groups are 3 to 5 tiles; the
tile-edge streams are three tiles at every misalignment of the data; the far-carried states span 2 and 66 tiles, and 300 tiles so
that a thread of the scan takes more than one."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import beast_util as hu
import helpers
import pf_in_util as pu
import raw_in_util as ru

pytestmark = pytest.mark.gpu

GUARD = 4                                        # entries in front of and behind every array
EXTERNAL = 2                                     # MGPU_FILTER_CLOCK_EXTERNAL: the filter starts empty, as the harness's does
CLI = os.path.join(helpers.ROOT, "readsb_amd", "host", "readsb_gpu_pf_in")
D, E = b"\x10", b"\x03"
BEHIND = E + D + b"\xc1" + bytes(30) + D + E     # bytes behind the stream: nothing of them may count
LONG = ru.es(pu.A, 3)[:14].tobytes()
GOOD = pu.frame(LONG)
# every unstuffed byte behind a DLE: the handler reads as far as it can (the id cannot be stuffed: 52 of the 53 bytes)
MAXIMAL = D + b"\xc1" + D + D + D + b"\x12" + D + D * 1 + (D + D) * 8 + (D + D) * 14 + D + E
assert len(MAXIMAL) == pu.REACH + 1


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
    return pu.load_golden()


def prepare(d, ops):
    for op in ops:
        d.filter_expire() if op < 0 else d.filter_add(op)


def run(d, hip, form, data, cfg, msgs_cap=None, frames_cap=None, data_off=0, pass_bytes=0, optional=True):
    """One call with every array between canaries -> pu.result_of's dict with `intact`."""
    from readsb_amd import binding
    data = bytes(data)
    msgs_cap = len(data) // 4 + 1 if msgs_cap is None else msgs_cap
    frames_cap = len(data) // 4 + 1 if frames_cap is None else frames_cap
    sizes = dict(msgs=(msgs_cap, 64), signal=(msgs_cap, 8), frame_of=(msgs_cap, 8), cls=(frames_cap, 1), off=(frames_cap, 8))
    dtypes = dict(msgs=pu.MSG, signal=np.float64, frame_of=np.uint64, cls=np.uint8, off=np.uint64)
    src = np.frombuffer(D * data_off + data + BEHIND, dtype=np.uint8)
    outs, cn = pu.new_outs(), binding.PfInCounters()
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
    a = pu.pf_args(binding, dp, len(data), None, outs, cn, msgs_cap=msgs_cap, frames_cap=frames_cap if optional else 0, pass_bytes=pass_bytes, pointers=ptr)
    f = d.lib.mgpu_pf_decode if form == "host" else d.lib.mgpu_pf_decode_device
    rc = int(f(d.ctx, C.byref(a)))
    raw = {}
    for k, (n, size) in sizes.items():
        nb = (n + 2 * GUARD) * size
        raw[k] = host[k] if form == "host" else hip.download(host[k], nb)
        if form != "host":
            hip.free(host[k])
    if d_data is not None:
        hip.free(d_data)
    nm = min(int(outs[2].value), msgs_cap) if rc != pu.MGPU_E_INVAL else 0
    nf = min(int(outs[1].value), frames_cap) if rc != pu.MGPU_E_INVAL else 0
    arrays, intact = {}, True
    for k, (n, size) in sizes.items():
        used = (nm if k in ("msgs", "signal", "frame_of") else nf) if (optional or k == "msgs") else 0
        lo, hi = GUARD * size, (GUARD + used) * size
        intact = intact and bool((raw[k][:lo] == 0xA5).all() and (raw[k][hi:] == 0xA5).all())
        arrays[k] = raw[k][lo:hi].copy().view(dtypes[k])
    res = pu.result_of(binding, rc, arrays, outs, cn)
    res["intact"] = intact
    return res


def same(res, want, what=None):
    """want: a golden entry or a result of pu.host_decode"""
    assert res["rc"] == pu.MGPU_OK and res["intact"], (what, res["rc"], res["intact"])
    if "head" in want:
        pu.compare(res, want, what)
    else:
        pu.same(res, want, what)


def both(ctxs, data, cfg, what=None, ops=(), **kw):
    """The stream through both forms against the sequential walk -> the walk's result."""
    get, hip = ctxs
    f = ru.FilterModel()
    for op in ops:
        f.expire() if op < 0 else f.add(op)
    want = pu.host_decode(get(cfg).lib, data, cfg, f)
    assert want["rc"] == pu.MGPU_OK
    for form in ("device", "host"):
        d = get(cfg)
        prepare(d, ops)
        same(run(d, hip, form, data, cfg, **kw), want, (what, form))
    return want


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("group", pu.GROUPS)
def test_golden_groups(ctxs, golden, group, form):
    """Every golden group under every configuration through the C entry of either form.  After group (d) a second call with one
    Address/Parity frame per prepared address: the context's filter stands where the reference's does.  Group (p) reads past the end."""
    get, hip = ctxs
    for k, cfg in enumerate(pu.CONFIGS[group]):
        d = get(cfg)
        prepare(d, pu.ops_of(group))
        res = run(d, hip, form, golden[pu.key(group, cfg)]["stream"], cfg, data_off=5 * k)
        same(res, golden[pu.key(group, cfg)], (group, cfg))
        assert res["counters"]["past_end"] == (1 if group == "p" else 0)
        if group == "d":
            same(run(d, hip, form, golden[pu.key("d2", cfg)]["stream"], cfg), golden[pu.key("d2", cfg)], ("d2", cfg))


def placed(first, traffic, what, total=3 * pu.TILE + 100):
    """Traffic (a list of frames) with `what` starting at stream position `first`, zeros between, traffic again up to `total` bytes."""
    head, at, k = [], 0, 0
    while at + len(traffic[k]) <= first:
        head.append(traffic[k])
        at += len(traffic[k])
        k += 1
    head.append(bytes(first - at))
    s = b"".join(head) + what
    while len(s) < total:
        s += traffic[k]
        k += 1
    return s


def test_tile_edges(ctxs):
    """The frame whose decode reaches furthest placed so that each of its bytes in turn is the first byte of the second tile, in both
    forms (in the device form the misalignment of the data going round 0..15 with it), and across the end of the second tile at every
    misalignment; a DLE as a tile's last byte, and as a lane's, with ETX, DLE and an ordinary byte behind it, searching and in a frame."""
    get, hip = ctxs
    cfg = (1, 1, 1)
    traffic = pu.pad_to([], 3 * pu.TILE + 400, np.random.default_rng(31))
    for k in range(len(MAXIMAL)):
        s = placed(pu.TILE - k, traffic, MAXIMAL)
        assert s[pu.TILE - k: pu.TILE - k + len(MAXIMAL)] == MAXIMAL and 3 * pu.TILE < len(s)
        want = pu.host_decode(get(cfg).lib, s, cfg)
        at = want["off"].tolist().index(pu.TILE - k)
        assert want["cls"][at] in (pu.ACCEPT, pu.UNKNOWN, pu.BAD) and want["counters"]["past_end"] == 0
        same(run(get(cfg), hip, "device", s, cfg, data_off=k % 16), want, ("edge", k))
        same(run(get(cfg), hip, "host", s, cfg), want, ("edge host", k))
    s = placed(2 * pu.TILE - 1, traffic, MAXIMAL)
    want = pu.host_decode(get(cfg).lib, s, cfg)
    for off in range(16):
        same(run(get(cfg), hip, "device", s, cfg, data_off=off), want, ("misalignment", off))
    for edge in (pu.TILE, pu.TILE + 7 * pu.CHUNK, 2 * pu.TILE):
        for behind in (E, D, b"\xc1", b"\x00"):
            for opened in (b"", D + b"\x41" + bytes(9), D + b"\xc1" + bytes(9)):             # searching; inside a frame of another id; of this one
                what = opened + D + behind + GOOD + D + E + GOOD
                s = placed(edge - len(opened) - 1, traffic, what, total=edge + 600)
                assert s[edge - 1: edge + 1] == D + behind
                both(ctxs, s, cfg, ("DLE at", edge, behind, opened), data_off=3)


def test_state_carried_far(ctxs):
    """A frame of another packet id whose body spans more than one tile without an event, more than one tile of stuffed DLE DLE x only,
    and more than 64 tiles with frame starts of this id inside it, which must give nothing; each also with the opening DLE removed, so
    that what it hid is framed; and 300 tiles of such frames, so that a thread of the tiles' scan carries a state over several tiles."""
    cfg = (1, 1, 1)
    inner = GOOD[:-2]                                                                         # a frame's start and body without its end: an event that is ignored in a frame
    bodies = {"no event": bytes(pu.TILE + 700), "stuffed": (D + D + b"x") * ((pu.TILE + 700) // 3),
              "starts inside": (inner + bytes(100)) * (66 * pu.TILE // (len(inner) + 100))}
    for name, body in bodies.items():
        s = GOOD * 5 + D + b"\x41" + body + D + E + GOOD * 7
        want = both(ctxs, s, cfg, name)
        assert (want["nframes"], want["counters"]["nskipped"], want["consumed"]) == (12, 1, len(s)), name
        s = GOOD * 5 + b"\x41" + body + D + E + GOOD * 7                                      # the opening DLE removed
        want = both(ctxs, s, cfg, (name, "opened"))
        # (behind a stuffed DLE DLE the x is a packet id: that frame runs to the same end)
        assert want["consumed"] == len(s) and want["nframes"] == (13 if name == "starts inside" else 12) and want["counters"]["nskipped"] == (1 if name == "stuffed" else 0), name
    # ... and cut in front of its end: consumed stays in front of the frame that is open, however far back
    s = GOOD * 5 + D + D + E + b"zz" + D + b"\x41" + bodies["starts inside"]
    want = both(ctxs, s, cfg, "open at the end")
    assert (want["nframes"], want["consumed"]) == (5, 5 * len(GOOD) + 2)
    unit = D + b"\x41" + bytes(3 * pu.TILE + 11) + inner + D + E + GOOD + D + E + D + b"\xc1" + bytes(2 * pu.TILE - 5) + D + D + E
    s = unit * (300 * pu.TILE // len(unit))
    want = both(ctxs, s, cfg, "300 tiles")
    assert want["nframes"] == 2 * (len(s) // len(unit)) and want["counters"]["nskipped"] == len(s) // len(unit) and want["consumed"] == len(s)


def test_the_four_byte_frame_and_the_end(ctxs):
    """DLE c1 DLE ETX: its decode runs through its own end into what lies behind it — in front of a tile edge into the next tile, in
    front of the end of the stream behind the buffer, where every byte counts as 0 and past_end counts the call; in the host form's
    passes only the real end counts."""
    get, hip = ctxs
    cfg = (1, 1, 1)
    traffic = pu.pad_to([], 2 * pu.TILE + 400, np.random.default_rng(33))
    for k in range(1, 8):
        s = placed(pu.TILE - k, traffic, pu.TINY * 2, total=pu.TILE + 300)
        want = both(ctxs, s, cfg, ("tiny at the edge", k), data_off=k)
        assert pu.TILE - k in want["off"].tolist() and want["counters"]["past_end"] == 0
    for tail in range(0, 56, 5):
        s = placed(pu.TILE + 77, traffic, GOOD + pu.TINY + bytes(tail), total=0)
        want = both(ctxs, s, cfg, ("tiny at the end", tail))
        assert want["counters"]["past_end"] == (1 if tail < 11 else 0), tail             # it reads 15 bytes from its start: 11 behind its own four
        d = get(cfg)
        same(run(d, hip, "host", s, cfg, pass_bytes=1000), want, ("passes", tail))
    want = both(ctxs, GOOD + pu.TINY, (1, 1, 0), "mode_ac off returns in front of the reads")
    assert want["counters"]["past_end"] == 0 and want["cls"].tolist() == [pu.ACCEPT, pu.MODEAC_OFF]


def test_short_streams(ctxs):
    """Streams of 0 to 4 bytes over the framer's bytes; all DLE; all DLE ETX."""
    cfg = (1, 1, 1)
    for n in range(5):
        for code in range(4 ** n):
            s = bytes((0x10, 0x03, 0xC1, 0x00)[(code >> (2 * k)) & 3] for k in range(n))
            both(ctxs, s, cfg, s)
    for n in (1, 31, 32, 33, pu.TILE - 1, pu.TILE, pu.TILE + 1, 2 * pu.TILE + 5):
        want = both(ctxs, D * n, cfg, ("all DLE", n))
        assert (want["consumed"], want["nframes"]) == (n, 0)
        want = both(ctxs, (D + E) * n, cfg, ("all DLE ETX", n))
        assert (want["consumed"], want["nframes"]) == (2 * n - 1, 0)


def filter_state(d, hip, addrs):
    """Which of the addresses the context's filter holds, asked with Address/Parity frames (which add nothing)."""
    stream = b"".join(pu.frame_of_df(ru.ap(4, int(a), k)) for k, a in enumerate(addrs))
    return run(d, hip, "device", stream, (1, 1, 0))["cls"].tolist()


@pytest.mark.parametrize("form", ["host", "device"])
def test_filter_order_growth_and_state(ctxs, golden, form):
    """The raw input's order cases carried over as Planefinder frames (group c: a conditional frame in front of and behind its adder, in
    the same lane's bytes and in the next tile); a foreign add (mgpu_filter_add between two calls); the growth of the table (group d:
    the reference's classes around L*); afterwards the context's filter agrees with the reference's, asked address by address."""
    get, hip = ctxs
    cfg = (1, 1, 0)
    d = get(cfg)
    same(run(d, hip, form, golden[pu.key("c", cfg)]["stream"], cfg), golden[pu.key("c", cfg)], "c")
    # a conditional frame and its adder in one lane's 32 bytes: short frames are 22 bytes, the pair starts a chunk
    a = 0x51A2B3
    f1, f2, f3 = pu.frame_of_df(ru.ap(5, a, 1)), pu.frame_of_df(ru.df11(a)), pu.frame_of_df(ru.ap(5, a, 2))
    s = bytes(pu.CHUNK * 3) + f1 + bytes(2 * pu.CHUNK - len(f1)) + f2 + f3
    res = run(get(cfg), hip, form, s, cfg)
    assert len(f2) < pu.CHUNK and res["cls"].tolist() == [pu.UNKNOWN, pu.ACCEPT, pu.ACCEPT] and res["off"].tolist() == [96, 160, 160 + len(f2)]
    d = get(cfg)
    foreign = 0x7B1234
    probe = pu.frame_of_df(ru.ap(4, foreign, 1)) + pu.frame_of_df(ru.ap(20, foreign, 2))
    assert run(d, hip, form, probe, cfg)["cls"].tolist() == [pu.UNKNOWN, pu.UNKNOWN]
    d.filter_add(foreign)
    assert run(d, hip, form, probe, cfg)["cls"].tolist() == [pu.ACCEPT, pu.ACCEPT]
    d = get(cfg)
    prepare(d, pu.ops_of("d"))
    g = golden[pu.key("d", cfg)]
    parts, lstar, lstar2, probes = pu.group_d_info()
    inactive = set(int(x) for x in ru.D_INACTIVE)
    assert sum(1 for ln, a, ok in probes if a in inactive and ln < lstar and ok) >= 10 and sum(1 for ln, a, ok in probes if a in inactive and ln > lstar and not ok) >= 20
    res = run(d, hip, form, g["stream"], cfg)
    same(res, g, "d")
    assert all(res["cls"][ln] == (pu.ACCEPT if ok else pu.UNKNOWN) for ln, a, ok in probes)
    asked = np.concatenate([ru.D_INACTIVE[:12], ru.D_ACTIVE[:4], ru.D_NEW[:12]])
    assert filter_state(d, hip, asked) == [pu.UNKNOWN] * 7 + [pu.ACCEPT] + [pu.UNKNOWN] * 3 + [pu.ACCEPT] + [pu.ACCEPT] * 16


def test_the_demodulator_sees_planefinder_learnt_addresses(ctxs):
    """The pre-screen, as tests/test_gpu_raw_in.py checks it: one capture with DF4 / DF5 frames of an address learnt only from the
    Planefinder feed (a clean DF17, in either form), demodulated after the call, is accepted by mgpu_feed_iq; the same capture on a
    fresh context is not, nor after a call that overflowed (the filter and the pre-screen stay where they stood)."""
    import filter_util
    import frames_util as fr
    import readsb_amd
    get, hip = ctxs
    addr = 0x4CA2D6
    frames = fr.ap_frames(np.array([4, 4, 5]), addr, payload_seed=5)
    iq = filter_util.modulate_buffers([(frames, np.full(3, 56))])
    stream = pu.frame_of_df(ru.es(addr, 1)) + GOOD
    got = {}
    for how in ("fresh", "overflow", "host", "device"):
        d = readsb_amd.Demodulator(startup_time_ms=helpers.STARTUP_MS, max_samples=8 * helpers.BUF_SAMPLES, filter_clock=EXTERNAL)
        try:
            if how == "overflow":
                res = run(d, hip, "device", stream, (1, 1, 0), msgs_cap=1)
                assert res["rc"] == pu.MGPU_E_OVERFLOW and res["nmsgs"] == 2 and res["intact"]
            elif how != "fresh":
                res = run(d, hip, how, stream, (1, 1, 0))
                assert res["rc"] == pu.MGPU_OK and res["cls"].tolist() == [pu.ACCEPT, pu.ACCEPT]
            got[how] = d.demodulate_capture(iq)[0]
        finally:
            d.close()
    assert len(got["fresh"]) == 0 and len(got["overflow"]) == 0
    for how in ("host", "device"):
        assert len(got[how]) == 3 and (got[how]["addr"] == addr).all() and got[how]["msg"].tobytes() == frames[:, :14].tobytes(), how


def test_modeac_off_leaves_no_record_and_counts_nothing(ctxs):
    s = pu.frame(b"\x77\x00") + GOOD + pu.frame(b"\x12\x34", sig=0x10) + pu.frame(b"\x00\x00", type_=0xF0) + pu.frame(LONG, type_=7)
    want = both(ctxs, s, (1, 1, 0), "mode_ac off")
    assert want["cls"].tolist() == [pu.MODEAC_OFF, pu.ACCEPT, pu.MODEAC_OFF, pu.MODEAC_OFF, pu.TYPE] and want["nmsgs"] == 1
    assert want["counters"]["remote_received_modeac"] == 0 and want["counters"]["remote_received_modes"] == 1
    want = both(ctxs, s, (1, 1, 1), "mode_ac on")
    assert want["cls"].tolist() == [pu.MODEAC, pu.ACCEPT, pu.MODEAC, pu.MODEAC, pu.TYPE] and want["nmsgs"] == 4 and want["counters"]["remote_received_modeac"] == 3


@pytest.mark.parametrize("form", ["host", "device"])
def test_capacities_one_short(ctxs, golden, form):
    """msgs_cap and the frame capacity exact, then each one short: MGPU_E_OVERFLOW with the needed counts, the canaries intact, nothing
    stored at or beyond a capacity, the filter untouched; then the same call with room gives the golden.  The optional arrays left out."""
    get, hip = ctxs
    cfg = (1, 1, 0)
    g = golden[pu.key("d", cfg)]
    need, nframes = len(g["msgs"]), len(g["cls"])
    asked = np.concatenate([ru.D_INACTIVE[:12], ru.D_ACTIVE[:4], ru.D_NEW[:12]])
    d = get(cfg)
    prepare(d, pu.ops_of("d"))
    state0 = filter_state(d, hip, asked)
    assert state0 == [pu.ACCEPT] * 16 + [pu.UNKNOWN] * 12
    for kw in (dict(msgs_cap=need - 1), dict(frames_cap=nframes - 1), dict(msgs_cap=7, frames_cap=3), dict(msgs_cap=need // 2, pass_bytes=9000)):
        if "pass_bytes" in kw and form == "device":
            continue
        res = run(d, hip, form, g["stream"], cfg, **{**dict(msgs_cap=need, frames_cap=nframes), **kw})
        assert res["rc"] == pu.MGPU_E_OVERFLOW and res["intact"], kw
        assert (res["nmsgs"], res["nframes"], res["consumed"]) == (need, nframes, int(g["head"][0])), kw
        assert res["msgs"].tobytes() == g["msgs"][: len(res["msgs"])].tobytes() and res["signal"].tobytes() == g["signal"][: len(res["signal"])].tobytes(), kw
        assert res["cls"].tobytes() == g["cls"][: len(res["cls"])].tobytes() and res["off"].tobytes() == g["off"][: len(res["off"])].tobytes(), kw
        assert filter_state(d, hip, asked) == state0, kw                                     # the filter is where it stood
    res = run(d, hip, form, g["stream"], cfg, msgs_cap=need, frames_cap=nframes, optional=False)
    assert res["rc"] == pu.MGPU_OK and res["intact"] and res["msgs"].tobytes() == g["msgs"].tobytes()
    d = get(cfg)
    prepare(d, pu.ops_of("d"))
    same(run(d, hip, form, g["stream"], cfg, msgs_cap=need, frames_cap=nframes), g, "exact")


def test_host_passes_and_bad_arguments(ctxs, golden):
    """The host form with pass_bytes that cut inside frames, between a DLE and the byte behind it and inside a handler call's reads
    (down to 1: every pass grows until it reaches a som) gives the bytes of one call; the binding's pf_decode gives the golden;
    MGPU_E_INVAL as documented."""
    from readsb_amd import binding
    get, hip = ctxs
    cfg = (1, 1, 1)
    g = golden[pu.key("a", cfg)]
    for pass_bytes in (len(g["stream"]) // 3 + 1, pu.TILE, 1000):
        same(run(get(cfg), hip, "host", g["stream"], cfg, pass_bytes=pass_bytes), g, pass_bytes)
    part = g["stream"][:1500]
    same(run(get(cfg), hip, "host", part, cfg, pass_bytes=1), pu.host_decode(get(cfg).lib, part, cfg), 1)
    p = golden[pu.key("p", cfg)]
    same(run(get(cfg), hip, "host", p["stream"], cfg, pass_bytes=777), p, "p in passes")
    d = get(cfg)
    res = d.pf_decode(g["stream"], now_ms=pu.NOW_MS)
    assert res["msgs"].tobytes() == g["msgs"].tobytes() and res["frame_class"].tobytes() == g["cls"].tobytes() and res["frame_off"].tobytes() == g["off"].tobytes()
    assert res["signal_level"].tobytes() == g["signal"].tobytes() and res["consumed"] == int(g["head"][0]) and res["counters"]["past_end"] == 0
    buf = np.frombuffer(GOOD * 3, dtype=np.uint8)
    for form in ("host", "device"):
        f = d.lib.mgpu_pf_decode if form == "host" else d.lib.mgpu_pf_decode_device
        arrays, outs, cn = pu.new_arrays(buf.size), pu.new_outs(), binding.PfInCounters()
        dp = buf.ctypes.data if form == "host" else hip.upload(buf)
        dev = {k: hip.malloc(v.nbytes) for k, v in arrays.items()} if form == "device" else None

        def args(**kw):
            a = pu.pf_args(binding, dp, buf.size, arrays, outs, cn, pointers=dev)
            for k, v in kw.items():
                setattr(a, k, v)
            return C.byref(a)
        assert f(d.ctx, args()) == pu.MGPU_OK and int(outs[2].value) == 3
        assert f(None, None) == pu.MGPU_E_INVAL and f(d.ctx, None) == pu.MGPU_E_INVAL
        for kw in (dict(size=C.sizeof(binding.PfInArgs) - 8), dict(size=0), dict(data=None), dict(msgs=None), dict(counters=None), dict(consumed=None), dict(nframes=None),
                   dict(nmsgs=None), dict(frame_class=None, frame_off=None), dict(now_ms=-1), dict(now_ms=253402300800000), dict(nbytes=1 << 32)):
            assert f(d.ctx, args(**kw)) == pu.MGPU_E_INVAL, (form, kw)
        if form == "device":
            assert f(d.ctx, args(msgs=dev["msgs"] + 4)) == pu.MGPU_E_INVAL                      # records off their alignment
            hip.free(dp)
            for q in dev.values():
                hip.free(q)
        assert f(d.ctx, args(nbytes=0, data=None)) == pu.MGPU_OK and [int(x.value) for x in outs] == [0, 0, 0]


def test_command_line_against_the_library(ctxs, golden):
    """readsb_gpu_pf_in as a child process on a golden stream: its output equals the beast encoder's over the expected records, with a
    block smaller than the stream so that the remainder, the filter and the counters are carried between calls; the counters on stderr."""
    get, hip = ctxs
    for g, cfg, flags, block in (("a", (1, 1, 1), ["--fix", "--mode-ac"], 3000), ("p", (1, 1, 1), ["--mode-ac", "--verbatim"], 1 << 20), ("c", (1, 1, 0), [], 700)):
        e = golden[pu.key(g, cfg)]
        stream = e["stream"]
        want = pu.host_decode(get(cfg).lib, stream, cfg)
        enc = bytes(get(cfg).beast_encode_ex(want["msgs"], verbatim="--verbatim" in flags)[0])
        r = subprocess.run([CLI, *flags, "--now", str(pu.NOW_MS), "--block", str(block)], input=stream, capture_output=True, timeout=120)
        assert r.returncode == 0, r.stderr[-500:]
        assert r.stdout == enc, (g, cfg, len(r.stdout), len(enc))
        words = r.stderr.decode().split()
        assert words[:4] == ["frames", str(want["nframes"]), "messages", str(want["nmsgs"])] and words[words.index("nskipped") + 1] == str(want["counters"]["nskipped"])
        assert words[words.index("past_end") + 1] == str(want["counters"]["past_end"]) and words[words.index("consumed") + 1] == str(want["consumed"])
