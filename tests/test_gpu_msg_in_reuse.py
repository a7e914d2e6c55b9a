"""-m gpu: ONE context through the three message inputs in turn (include/modes_gpu.h: mgpu_raw_decode, mgpu_beast_decode, mgpu_pf_decode
and their `_device` forms), at stream sizes that grow, shrink and grow again.  The inputs share the ICAO filter, the filter passes'
candidate arrays, the host forms' staging buffers and the tile scratch by role (the Planefinder input frames in the beast input's
buffers), and one host core drives all three (behind_in.cpp): what one call leaves in any of them must change nothing in the next.

The same streams are walked by mgpu_raw_decode_host / mgpu_beast_decode_host / mgpu_pf_decode_host over ONE FilterModel carried from
call to call, and every call's result — messages, signal bit patterns, index-of, receiver ids, class, offset, counts and counters — is
compared bytewise with its counterpart in that walk; the canaries around every array must be intact.  One call mid-sequence ends in
MGPU_E_OVERFLOW (msgs_cap one short): the calls behind it show that the filter and the tables stood where they were.

Shapes: a tile is 8192 bytes, a beast group 64 tiles.  One frame; about 3 tiles; about 66 tiles (a second beast group, a second round
of the scans' threads); about 1 tile.  Each host form runs once with a pass_bytes that cuts inside frames, directly behind a `_device`
call of another format.  Every stream opens with traffic of a few addresses nobody has heard of and of those the three calls in front
of it — most of them of other formats — introduced: the filter state carried across formats decides classes, and the walk asserts
that it does."""
import copy
import functools

import numpy as np
import pytest

import beast_in_util as bu
import beast_util as hu
import helpers
import pf_in_util as pu
import raw_in_util as ru

pytestmark = pytest.mark.gpu

EXTERNAL = 2                                     # MGPU_FILTER_CLOCK_EXTERNAL: the filter starts empty, as the models do
CFG = (1, 1, 1)                                  # nfix_crc, fixDF, mode_ac (beast: and net_ingest 0)
ONE, T1, T3, T66 = 0, ru.TILE + 333, 3 * ru.TILE + 517, 66 * ru.TILE + 1029
# (format, form, size, pass_bytes, msgs_cap one short)
CALLS = (("raw", "device", ONE, 0, False),
         ("beast", "device", T3, 0, False),
         ("pf", "host", T3, 3001, False),         # behind a `_device` call of another format, cut inside frames
         ("beast", "device", T66, 0, False),
         ("pf", "device", T1, 0, False),          # small Planefinder in the buffers a large beast call framed in
         ("raw", "host", T3, 2999, False),
         ("pf", "device", T66, 0, False),
         ("beast", "host", T1, 5003, False),      # ... and the reverse
         ("raw", "device", T66, 0, False),
         ("beast", "device", T1, 0, True),        # small calls on the candidate arrays and the staging of a large raw call; this one overflows
         ("pf", "device", ONE, 0, False),
         ("beast", "host", T3, 0, False))
NEW = (0x700000 + 0x010203 * np.arange(8 * len(CALLS))).astype(np.uint32).reshape(len(CALLS), 8)   # the addresses call k introduces
UTIL = dict(raw=ru, beast=bu, pf=pu)


def _cfg(fmt):
    return CFG + (0,) if fmt == "beast" else CFG


def _streams(lib):
    """The calls' streams: in front the traffic of the addresses this call and the three before it introduce, behind it drawn traffic of
    the format (one draw of about a tile per format, repeated: at no multiple of a tile, so every repetition meets the tiles anew)."""
    rng = np.random.default_rng(20261)
    base = dict(raw=ru.stream_of(ru.filler(rng, 330, ru.POOL)), beast=bu.cut_at_stop(lib, bu.draw_stream(rng, 420, 0.05), _cfg("beast")), pf=pu.draw_stream(rng, 360, 0.05))
    assert all(ru.TILE < len(b) < 2 * ru.TILE and len(b) % 32 for b in base.values()), [len(b) for b in base.values()]
    out = []
    for k, (fmt, form, size, pass_bytes, short) in enumerate(CALLS):
        u = UTIL[fmt]
        if size == ONE:                          # one frame: the first adder of all, or a reply of an address the call before last introduced
            f = ru.es(int(NEW[0][0]), 0) if k == 0 else ru.ap(4, int(NEW[k - 2][0]), k)
            out.append(ru.avr(f) if fmt == "raw" else u.frame_of_df(f))
            continue
        pool = np.concatenate(NEW[max(0, k - 3): k + 1])
        lead = u.stream_of(u.filler(rng, 80, pool))
        out.append(lead + (base[fmt] * (size // len(base[fmt]) + 1))[: size - len(lead)])
    return out


@functools.lru_cache(maxsize=None)
def walked(lib):
    """-> [(stream, what the sequential walk gives for it)]: the calls in order over one FilterModel.  The call that overflows is walked
    with room on a copy of the model, which stays where it stood.  Asserts what the sequence is meant to show."""
    model, alone = ru.FilterModel(), dict(raw=ru.FilterModel(), beast=ru.FilterModel(), pf=ru.FilterModel())
    out = []
    for k, (stream, (fmt, form, size, pass_bytes, short)) in enumerate(zip(_streams(lib), CALLS)):
        u, cfg = UTIL[fmt], _cfg(fmt)
        want = u.host_decode(lib, stream, cfg, copy.deepcopy(model) if short else model)
        assert want["rc"] == ru.MGPU_OK and want["nmsgs"] > 0, (k, want["rc"])
        assert size == ONE or abs(len(stream) - size) < 64, (k, len(stream))
        if fmt == "beast":
            assert want["stop"] == bu.STOP_END, k
        # the same stream against what this format's own calls alone have taught a filter: frames of addresses that only a call of
        # ANOTHER format introduced are rejected there and accepted here
        other = u.host_decode(lib, stream, cfg, copy.deepcopy(alone[fmt]) if short else alone[fmt])
        assert len(other["cls"]) == len(want["cls"])
        if k:
            assert np.count_nonzero((want["cls"] == ru.ACCEPT) & (other["cls"] == ru.UNKNOWN)) >= 1, (k, "no frame is decided by another format's adds")
        out.append((stream, want))
    assert model.bits > 8                         # (the table grew on the way)
    return out


def test_the_three_inputs_in_turn_on_one_context(built):
    import readsb_amd
    import test_gpu_beast_in as tb
    import test_gpu_pf_in as tp
    import test_gpu_raw_in as tr
    d = readsb_amd.Demodulator(nfix_crc=CFG[0], fix_df=CFG[1], mode_ac=CFG[2], startup_time_ms=helpers.STARTUP_MS, max_samples=131072, filter_clock=EXTERNAL)
    hip = hu.Hip()
    try:
        for k, ((stream, want), (fmt, form, size, pass_bytes, short)) in enumerate(zip(walked(d.lib), CALLS)):
            what = (k, fmt, form, len(stream))
            cap = dict(msgs_cap=want["nmsgs"] - 1) if short else {}
            if fmt == "raw":
                res = tr.run(d, hip, form, stream, pass_bytes=pass_bytes, **cap)
            else:
                res = (tb if fmt == "beast" else tp).run(d, hip, form, stream, _cfg(fmt), pass_bytes=pass_bytes, **cap)
            if not short:
                (tr if fmt == "raw" else tb if fmt == "beast" else tp).same(res, want, what)
                continue
            # what is needed, nothing at or beyond the capacity, everything below it; the filter goes back (the calls behind show it)
            assert res["rc"] == ru.MGPU_E_OVERFLOW and res["intact"], what
            for key in ("consumed", "nframes", "nmsgs", "stop", "stop_off", "id_out", "counters"):
                assert res[key] == want[key], (what, key)
            for key in ("msgs", "ids", "signal", "frame_of", "cls", "off"):
                assert res[key].tobytes() == want[key][: len(res[key])].tobytes(), (what, key)
            assert len(res["msgs"]) == want["nmsgs"] - 1 and len(res["cls"]) == want["nframes"]
    finally:
        hip.free_all()
        d.close()
