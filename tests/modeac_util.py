"""A Mode A/C reply builder for tests, the case sets built with it, and the two checkers they are run against
(tests/test_gpu_modeac_built.py under -m gpu, tests/test_modeac_reference.py on the CPU).

tools/synth_iq.c draws its replies; here a test says exactly where a reply starts, down to the cycle of the demodulator's virtual
60 MHz clock (demodulate2400AC, demod_2400.c): one 2.4 MHz sample = 25 cycles, one pulse slot = 87 cycles of which the first 27 are
on, 20 slots F1 C1 A1 C2 A2 C4 A4 X B1 D1 B2 D2 B4 D4 F2 X X SPI X X.  A sample's value is the amplitude times the part of it an
on-period covers.  The case sets put replies where the product's scan (k_modeac: tiles of 2048 positions with 80 samples of
look-ahead, a queue of 1024 candidates per tile, 64 output lists) and the host's skip over an accepted reply have their edges.

Two levels.  Magnitude level: a case set is an iterable of (data, length, noise_level, tag), one struct mag_buf each: data = 326
trailing samples of the buffer before, then `length` new ones; the buffer's mean_level is 0 and its mean_power the one that makes the
reference's noise_level exactly the integer asked for.  The checker is the restatement (oracle/modes_oracle.c), one buffer at a
time; tests/test_modeac_reference.py pins it to the reference's own objects on the IQ-level sets.  IQ level: a capture whose
converted magnitudes are the wanted ones as nearly as the format allows; the checker is helpers.reference_run.

thresholds() recomputes the reference's clock estimate and slot thresholds in numpy.  It only says where to put a sample so that it
sits at, below or above a threshold: what the demodulator makes of the buffer is always the checker's word."""
import ctypes as C
import functools
import types

import numpy as np

import frames_util
import helpers

B, TR = helpers.BUF_SAMPLES, helpers.TRAILING
SAMPLE, SLOT, ON = 25, 87, 27
F1F2 = 0x80020
FLOOR = 20
SPACING = 140                # samples between the F1s of replies that must not see each other (a reply and its look-ahead span 70)
AMPLITUDE, NOISE = 20000, 3000
TILE = 2048                  # k_modeac's positions per workgroup

PULSES = ("F1", "C1", "A1", "C2", "A2", "C4", "A4", "X", "B1", "D1", "B2", "D2", "B4", "D4", "F2", "X", "X", "SPI", "X", "X")
CODE_BIT = {"A4": 0x4000, "A2": 0x2000, "A1": 0x1000, "B4": 0x0400, "B2": 0x0200, "B1": 0x0100, "SPI": 0x0080,
            "C4": 0x0040, "C2": 0x0020, "C1": 0x0010, "D4": 0x0004, "D2": 0x0002, "D1": 0x0001}


def code_of(index, spi=0):
    """The 12-bit index ABCD (four octal digits) as the 16-bit word 0AAA 0BBB SCCC 0DDD of a Mode A/C message."""
    index = np.asarray(index, dtype=np.int64)
    return ((index >> 9 & 7) << 12) | ((index >> 6 & 7) << 8) | ((index >> 3 & 7) << 4) | (index & 7) | (np.asarray(spi, dtype=np.int64) << 7)


def bits20_of(code):
    """The 20 slots of a reply carrying `code`, slot 0 (F1) in bit 19: 0x80020 | data."""
    code = np.asarray(code, dtype=np.int64)
    bits = np.full(code.shape, F1F2, dtype=np.int64)
    for slot, name in enumerate(PULSES):
        if name in CODE_BIT:
            bits |= np.where(code & CODE_BIT[name], 1 << (19 - slot), 0)
    return bits


def replies(m, start_cycle, bits20, amplitude):
    """Write the on-slots of many replies into the uint16 magnitude array m (max-combined with what is there)."""
    start = np.asarray(start_cycle, dtype=np.int64).reshape(-1)
    bits = np.broadcast_to(np.asarray(bits20, dtype=np.int64).reshape(-1), start.shape)
    amp = np.broadcast_to(np.asarray(amplitude, dtype=np.int64).reshape(-1), start.shape)
    assert (start >= 0).all() and (amp >= 0).all() and (amp <= 65535).all()
    for slot in range(20):
        on = (bits >> (19 - slot)) & 1 != 0
        c0 = start[on] + SLOT * slot
        c1 = c0 + ON
        for k in range(3):                                        # 27 cycles touch two or three samples
            s = c0 // SAMPLE + k
            overlap = np.minimum(c1, (s + 1) * SAMPLE) - np.maximum(c0, s * SAMPLE)
            keep = overlap > 0
            np.maximum.at(m, s[keep], (amp[on][keep] * overlap[keep] // SAMPLE).astype(m.dtype))
    return m


def reply(m, start_cycle, bits20, amplitude):
    """One reply: a slot is on for 27 cycles of every 87 from start_cycle = 25 * f1 + phase."""
    return replies(m, [start_cycle], [bits20], [amplitude])


def layout(length, f1, phase=0, code=0, amplitude=AMPLITUDE, floor=FLOOR):
    """struct mag_buf.data of `length` new samples: replies with F1 at data[f1] (at least SPACING apart, or overlapping on purpose)
    over a constant floor."""
    data = np.full(TR + length, floor, dtype=np.uint16)
    f1 = np.asarray(f1, dtype=np.int64).reshape(-1)
    if len(f1):
        assert f1.min() >= 0 and f1.max() + 75 <= TR + length
        replies(data, SAMPLE * f1 + np.asarray(phase, dtype=np.int64), bits20_of(code), amplitude)
    return data


# ---- the reference's numbers, for placing samples only --------------------------------------------------------------------------

def noise_level(mean_level, mean_power):
    sd = np.sqrt(np.float64(mean_power) - np.float64(mean_level) * np.float64(mean_level))
    return int((np.float64(mean_power) + sd) * 65535 + 0.5)


@functools.lru_cache(maxsize=None)
def power_for_noise(n):
    """A mean_power (with mean_level 0, so never below mean_level squared) whose noise_level is exactly n."""
    t = n / 65535.0
    x = (np.sqrt(1.0 + 4.0 * t) - 1.0) / 2.0
    p = float(x * x)
    for _ in range(64):
        got = noise_level(0.0, p)
        if got == n:
            return p
        p = float(np.nextafter(p, np.inf if got < n else 0.0))
    raise AssertionError(f"no mean_power for noise level {n}")


def f1_clock_of(f1, m0, m1):
    a, b = np.float32(m0) * np.float32(m0), np.float32(m1) * np.float32(m1)
    fraction = np.float32(b / np.float32(a + b))
    at = np.float32(np.float32(f1) + np.float32(fraction * fraction))
    return int(np.float64(np.float32(np.float32(25) * at)) + 0.5)


def thresholds(m, f1, noise):
    """f1_clock, f2_clock, f2_sample, the two levels and the two slot thresholds of a candidate at m[f1]."""
    m0, m1 = int(m[f1]), int(m[f1 + 1])
    f1_clock = f1_clock_of(f1, m0, m1)
    f2_clock = f1_clock + SLOT * 14
    f2 = f2_clock // SAMPLE
    f1_level, f2_level = (m0 + m1) // 2, (int(m[f2]) + int(m[f2 + 1])) // 2
    midpoint = np.sqrt(np.float32(np.uint32(noise * max(f1_level, f2_level) & 0xffffffff)))
    return types.SimpleNamespace(
        f1_clock=f1_clock, f2_clock=f2_clock, f2_sample=f2, f1_level=f1_level, f2_level=f2_level,
        signal=int(np.float64(midpoint) * np.sqrt(2.0) + 0.5), noise=int(np.float64(midpoint) / np.sqrt(2.0) + 0.5),
        slot=lambda k: (f1_clock + SLOT * k) // SAMPLE)


# ---- magnitude level: the checker and the product, one struct mag_buf at a time ---------------------------------------------------

def _clock(done):
    st = done * 5
    return st, st // 12000 + helpers.STARTUP_MS


def mag_check(bufs):
    """The restatement on a case set -> (the messages of every buffer, a list of arrays; the counters at the end)."""
    lib = helpers.oracle_lib()
    lib.modes_oracle_set_mode_ac(1)
    lib.modes_oracle_set_filter_clock(0)
    cfg = helpers.OracleCfg(0, 1, 1, 58)
    lib.modes_oracle_stream_begin(C.byref(cfg), helpers.STARTUP_MS)
    out, stats, done = [], np.zeros(1, dtype=helpers.ORACLE_STATS), 0
    try:
        for data, length, noise, _tag in bufs:
            assert data.dtype == np.uint16 and data.flags["C_CONTIGUOUS"] and data.size >= TR + length
            st, sys_ms = _clock(done)
            lib.modes_oracle_stream_mag_buf(data.ctypes.data, length, st, sys_ms, 0.0, power_for_noise(noise))
            done += length
            ptr = C.c_void_p()
            n = lib.modes_oracle_stream_take(C.byref(ptr), stats.ctypes.data)
            msgs = np.zeros(n, dtype=helpers.ORACLE_MSG)
            if n:
                C.memmove(msgs.ctypes.data, ptr.value, n * helpers.ORACLE_MSG.itemsize)
            lib.modes_oracle_free(ptr)
            out.append(msgs)
    finally:
        lib.modes_oracle_set_mode_ac(0)
    return out, stats[0]


def mag_run(d, bufs):
    """The product (a Demodulator with mode_ac=1) on the same case set -> (messages, counters)."""
    d.reset()
    done = 0
    for data, length, noise, _tag in bufs:
        st, sys_ms = _clock(done)
        d.demod_mag_buf_ac(data, length, st, sys_ms, 0.0, power_for_noise(noise))
        done += length
    return d.collect()


def verdict(msgs):
    """What the checker made of a buffer, as something to compare: (timestamp, code) of every reply."""
    ac = msgs[msgs["msgtype"] == 77]
    return tuple((int(t), int(a) << 8 | int(b)) for t, a, b in zip(ac["timestamp"], ac["msg"][:, 0], ac["msg"][:, 1]))


def codes_seen(msgs):
    ac = msgs[msgs["msgtype"] == 77]
    return set((ac["msg"][:, 0].astype(np.int64) << 8 | ac["msg"][:, 1]).tolist())


# ---- the case sets ----------------------------------------------------------------------------------------------------------------
# Each is a function -> generator of (data, length, noise_level, tag).  A generator may hand out the same array again after changing
# it: use a buffer before asking for the next.  tag[0] names the set, tag[1] says how many clean, isolated replies the buffer holds
# (None where that is not the point), the rest identifies the case.

TILE_J = range(-2, 71)


def tile_edges(phases=range(25)):
    """F1 at 2048 k - j, k = 1 .. 63: j = 70 .. 1 puts F2 and the later slots into the next tile (the scan's look-ahead), j = 0, -1,
    -2 the F1 edge itself.  Every (j, phase) once, 63 to a buffer.  Then the same again with one loud sample among each reply's last ten
    (f1 + 60 .. f1 + 69, the quiet slots X4 and X5): what a scan that read anything but the sample itself there would not notice."""
    combos = [(j, p) for j in TILE_J for p in phases]
    for spoiled in (False, True):
        for lo in range(0, len(combos), 63):
            part = combos[lo:lo + 63]
            k = 1 + np.arange(len(part))
            f1 = TILE * k - np.array([j for j, _ in part])
            idx = (lo + np.arange(len(part))) * 37 % 4096
            data = layout(B, f1, [p for _, p in part], code_of(idx, idx & 1))
            if spoiled:
                data[f1 + 60 + (lo + np.arange(len(part))) % 10] = AMPLITUDE
            yield data, B, NOISE, ("tile", None if spoiled else len(part), lo, spoiled)


EDGE_LENGTHS = (B, 1, 2, 70, 327, 2047, 2049)
EDGE_PHASES = (0, 7, 13, 19, 24)


def buffer_edges():
    """One reply per buffer with F1 at the first positions (0 is never scanned), at the last ones (F2 and the bits then lie in what the
    next buffer will carry as its trailing samples) and at `length` itself (not this buffer's), for full and short buffers."""
    for mlen in EDGE_LENGTHS:
        f1s = sorted(set([0, 1, 2, 3, mlen - 2, mlen - 1, mlen] + list(range(mlen - 70, mlen - 59))))
        for f1 in f1s:
            if 0 <= f1 <= mlen:
                for p in EDGE_PHASES:
                    yield layout(mlen, [f1], p, code_of((f1 * 5 + p) % 4096)), mlen, NOISE, ("edge", 1 if 0 < f1 < mlen else None, mlen, f1, p)


SKIP_D = range(60, 81)
SKIP_LEN = 2 * TILE


def skip():
    """Two replies d samples apart: inside a tile, either side of a tile edge (two workgroups, two output lists), either side of a
    buffer edge (two calls: the skip does not carry over); and trains of eight.  An accepted reply hides the next 69 positions."""
    for p in (0, 12):
        for d in SKIP_D:
            yield layout(SKIP_LEN, [1000, 1000 + d], p, [code_of(0o1234), code_of(0o4321)]), SKIP_LEN, NOISE, ("skip", None, "mid", p, d)
            yield layout(SKIP_LEN, [TILE - 30, TILE - 30 + d], p, [code_of(0o1234), code_of(0o4321)]), SKIP_LEN, NOISE, ("skip", None, "tile", p, d)
            stream = layout(2 * SKIP_LEN, [SKIP_LEN - 30, SKIP_LEN - 30 + d], p, [code_of(0o1234), code_of(0o4321)])
            yield stream[:TR + SKIP_LEN].copy(), SKIP_LEN, NOISE, ("skip", None, "buffer", p, d, 0)
            yield stream[SKIP_LEN:].copy(), SKIP_LEN, NOISE, ("skip", None, "buffer", p, d, 1)
        for d in (69, 70, 71):
            f1 = TILE - 200 + d * np.arange(8)
            yield layout(SKIP_LEN, f1, p, code_of(0o1111 * (1 + np.arange(8) % 7))), SKIP_LEN, NOISE, ("skip", None, "train", p, d)


TIE_LEN, TIE_F1 = 512, 100
TIE_CODE = 0x1110            # A1 B1 C1: slots 1, 2 and 8 on; 3, 4, 5, 6 off
TIE_BASES = [(a, n) for a in (20000, 40000) for n in (2000, 3000, 5000)]


def ties():
    """One accepted reply, then one sample at a time at T - 1, T, T + 1 for every comparison of the loop body.  tag = ("tie", None,
    group, variant): the three variants of a group differ in that one sample only."""
    def group(name, a, n, data, noise, idx, t):
        for v in (-1, 0, 1):
            x = data.copy()
            x[idx] = t + v
            yield x, TIE_LEN, noise, ("tie", None, (name, a, n), v)

    for a, n in TIE_BASES:
        def base(phase):
            data = layout(TIE_LEN, [TIE_F1], phase, TIE_CODE, a)
            return data, thresholds(data, TIE_F1, n)
        f = TIE_F1
        # the three edge tests of F1: m[f-1] < m[f]; m[f+2] > m[f] (first pulse sample small: late phase); m[f+2] > m[f+1] (early phase)
        data, th = base(0)
        yield from group("f1 rising", a, n, data, n, f - 1, int(data[f]))
        yield from group("f1 quiet against second", a, n, data, n, f + 2, int(data[f + 1]))
        data, th = base(22)
        yield from group("f1 quiet against first", a, n, data, n, f + 2, int(data[f]))
        # the same of F2, 1218 cycles = 48 samples and 18 cycles later
        # (a reply whose F2 starts early in its sample is not accepted as built: the clock estimate is biased late.  So F2's second
        # sample is lowered by hand for the test against it.)
        data, th = base(12)
        f2 = th.f2_sample
        yield from group("f2 rising", a, n, data, n, f2 - 1, int(data[f2]))
        data[f2], data[f2 + 1] = a, 2000
        yield from group("f2 quiet against second", a, n, data, n, f2 + 2, 2000)
        data, th = base(4)
        f2 = th.f2_sample
        yield from group("f2 quiet against first", a, n, data, n, f2 + 2, int(data[f2]))
        # 6 dB: the noise level is half the pulse's level (the other framing pulse a little stronger), the level 2 noise - 1, 2 noise,
        # 2 noise + 1 by the pulse's second sample
        for name, at_f2 in (("f1 6 dB", False), ("f2 6 dB", True)):
            data, th = base(0)
            p, o = (th.f2_sample, f) if at_f2 else (f, th.f2_sample)
            data[o] += 8
            data[o + 1] += 8
            half = (int(data[p]) + int(data[p + 1])) // 4
            for v in (-1, 0, 1):
                x = data.copy()
                x[p + 1] = 4 * half + 2 * v - int(data[p])
                yield x, TIE_LEN, half, ("tie", None, (name, a, n), v)
        # a data slot that is on (A1, slot 2): its first sample at signal_threshold, its second out of the way
        data, th = base(0)
        s = th.slot(2)
        data[s + 1] = FLOOR
        yield from group("on slot", a, n, data, n, s, th.signal)
        data[s] = FLOOR
        yield from group("on slot, second sample", a, n, data, n, s + 1, th.signal)
        # a data slot that is off (A2, slot 4): both samples above noise_threshold is "uncertain"
        data, th = base(0)
        s = th.slot(4)
        data[s] = th.noise + 5
        yield from group("off slot", a, n, data, n, s + 1, th.noise)
        data[s + 1] = th.noise + 5
        yield from group("off slot, first sample", a, n, data, n, s, th.noise)
        # the third sample of an off slot (C2, slot 3) at signal_threshold is "noisy"
        data, th = base(0)
        yield from group("quiet third", a, n, data, n, th.slot(3) + 2, th.signal)


GRID_F1 = (5, 70001, 130900)
GRID_M0 = (1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 31, 32, 33, 100, 101, 255, 256, 257, 999, 1000, 1001, 2047, 2048, 2049, 4095, 4096, 4097,
           5792, 5793, 8191, 8192, 8193, 11585, 11586, 16383, 16384, 16385, 20000, 20001, 23170, 23171, 30000, 30001, 32767, 32768, 32769,
           40000, 40001, 46340, 46341, 50000, 50001, 60000, 60001, 65279, 65280, 65281, 65532, 65533, 65534, 65535, 12345)
GRID_M1 = (0,) + GRID_M0[:-1]
assert len(GRID_M0) == len(set(GRID_M0)) == 64 and len(GRID_M1) == 64


def phase_grid(f1):
    """The first pulse's two samples over a 64 x 64 grid with F1 at f1 (the buffer ends right behind it): the clock estimate
    25 (f1 + fraction^2) + 0.5 is float arithmetic, whose steps are 2^-7 at f1 >= 65536 and whose product has steps of 1/8 and 1/4 at
    the two large f1.  The other 19 slots stand where the estimate puts them, over a floor of zero."""
    mlen = f1 + 1
    data = np.zeros(TR + mlen, dtype=np.uint16)
    rest = bits20_of(code_of(0o5252)) & 0x7FFFF
    for m0 in GRID_M0:
        for m1 in GRID_M1:
            replies(data, [f1_clock_of(f1, m0, m1)], [rest], [max(m0, m1)])
            data[f1], data[f1 + 1] = m0, m1
            yield data, mlen, (m0 + m1) // 12, ("grid", None, f1, m0, m1)
            data[f1 - 1:f1 + 80] = 0


CODES_PER_BUFFER = (B - 200) // SPACING


def codes():
    """All 4096 codes, SPI off and on."""
    for lo in range(0, 8192, CODES_PER_BUFFER):
        i = np.arange(lo, min(lo + CODES_PER_BUFFER, 8192))
        yield layout(B, 30 + SPACING * np.arange(len(i)), 0, code_of(i % 4096, i // 4096)), B, NOISE, ("codes", len(i), lo)


QUEUE_PATTERN = (1000, 2000, 3000, 1500)
QUEUE_NOISE = 100


def full_queue():
    """The period-4 pattern passes the cheap F1 tests at 2 of every 4 positions: 1024 of a tile's 2048, the most there can be, in every
    tile (position 0, never scanned, holds a value that would not pass).  Then the same with a genuine reply in a cleared stretch of
    140 samples inside a tile, and with one across a tile edge."""
    pattern = np.tile(np.array(QUEUE_PATTERN, dtype=np.uint16), (TR + B) // 4 + 1)[:TR + B]
    yield pattern.copy(), B, QUEUE_NOISE, ("queue", None, "pattern")
    for name, lo in (("inside", 5 * TILE + 700), ("across", 9 * TILE - 70)):
        data = pattern.copy()
        data[lo:lo + SPACING] = FLOOR
        reply(data, SAMPLE * (lo + 30), bits20_of(code_of(0o7070)), AMPLITUDE)
        yield data, B, QUEUE_NOISE, ("queue", 1, name)


def cheap_passes(data, length, noise):
    """How many positions 1 .. length - 1 pass the three cheap F1 tests (for the full-queue set's own premise), per tile."""
    m = data.astype(np.int64)
    f = np.arange(1, length)
    ok = (m[f - 1] < m[f]) & (m[f + 2] <= m[f]) & (m[f + 2] <= m[f + 1]) & (noise * 2 <= (m[f] + m[f + 1]) // 2)
    return np.bincount(f[ok] // TILE, minlength=-(-length // TILE))


MAG_SETS = {"tile": tile_edges, "edge": buffer_edges, "skip": skip, "tie": ties, "codes": codes, "queue": full_queue,
            **{f"grid{f1}": functools.partial(phase_grid, f1) for f1 in GRID_F1}}


@functools.lru_cache(maxsize=None)
def mag_expected(name):
    """The checker's word on a magnitude-level set, computed once: (tags, per-buffer messages, counters, per-buffer f2_clock / 5)."""
    tags, lengths = [], []

    def walk():
        for buf in MAG_SETS[name]():
            tags.append(buf[3])
            lengths.append(buf[1])
            yield buf
    per_buffer, stats = mag_check(walk())
    rel, done = [], 0
    for msgs, length in zip(per_buffer, lengths):
        rel.append(msgs["timestamp"][msgs["msgtype"] == 77] - done * 5)
        done += length
    return tags, per_buffer, stats, rel


def check_mag_conditions(name):
    """What makes a set worth running, asserted on the checker's output alone (so it holds wherever the set is used)."""
    tags, per_buffer, stats, rel = mag_expected(name)
    nac = [int((m["msgtype"] == 77).sum()) for m in per_buffer]
    assert int(stats["demod_modeac"]) == sum(nac)
    clean = [(t[1], n) for t, n in zip(tags, nac) if t[1] is not None]
    if clean:
        built, found = sum(c for c, _ in clean), sum(n for _, n in clean)
        assert 2 * found >= built, f"{name}: the checker accepts {found} of {built} clean replies"
    if name == "tile":
        clean_found, spoiled_found = (sum(n for t, n in zip(tags, nac) if t[3] == s) for s in (False, True))
        assert 2 * spoiled_found <= clean_found, f"tile: {spoiled_found} replies accepted with a loud sample in a quiet slot, {clean_found} without"
    if name == "edge":
        for t, n in zip(tags, nac):
            if t[3] == 0 and t[4] == 0:
                assert n == 0, f"a reply found at position 0 of a buffer ({t})"
        for mlen in EDGE_LENGTHS:                              # something is found at the last position of every buffer long enough to have one
            if mlen > 1:
                assert any(n for t, n in zip(tags, nac) if t[2] == mlen and t[3] == mlen - 1), f"nothing found at the last position, length {mlen}"
    if name == "skip":
        count = {}
        for t, n in zip(tags, nac):
            count[t[2:5]] = count.get(t[2:5], 0) + n
        for kind in ("mid", "tile", "train"):
            for p in (0, 12):
                assert count[(kind, p, 69)] != count[(kind, p, 70)], f"skip {kind} phase {p}: 69 and 70 apart give the same count"
        assert all(count[("buffer", p, d)] == 2 for p in (0, 12) for d in (69, 70, 71)), "a reply behind a buffer edge is not hidden"
    if name == "tie":
        groups = {}
        for t, msgs in zip(tags, per_buffer):
            groups.setdefault(t[2], []).append(verdict(msgs))
        for g, vs in groups.items():
            assert len(vs) == 3 and len(set(vs)) >= 2, f"tie group {g}: the same verdict at T - 1, T and T + 1"
    if name.startswith("grid"):
        f1 = int(name[4:])
        offsets = set()
        for r in rel:
            offsets.update((r * 5 - SLOT * 14 - SAMPLE * f1).tolist())
        assert len(offsets) >= 3, f"{name}: clock offsets {sorted(offsets)}"
        assert sum(nac) >= 64 * 64 // 4, f"{name}: only {sum(nac)} of the grid's replies accepted"
    if name == "codes":
        seen = set().union(*(codes_seen(m) for m in per_buffer))
        want = set(code_of(np.arange(4096), 0).tolist()) | set(code_of(np.arange(4096), 1).tolist())
        assert want <= seen, f"{len(want - seen)} codes never seen"
    if name == "queue":
        for data, length, noise, tag in full_queue():
            per_tile = cheap_passes(data, length, noise)
            if tag[2] == "pattern":
                assert (per_tile == 1024).all()
            else:
                assert per_tile.max() == 1024 and (per_tile == 1024).sum() >= len(per_tile) - 2


# ---- IQ level ---------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _uc8_inverse():
    lut = np.ctypeslib.as_array(helpers.oracle_lib().modes_oracle_uc8_lut(), shape=(65536,)).astype(np.int64)
    order = np.argsort(lut, kind="stable")
    return lut[order], order


def uc8_of(mag):
    """The UC8 capture whose converted magnitudes are nearest the wanted ones: for each, the (I, Q) byte pair with the nearest entry of
    the converter's table."""
    values, order = _uc8_inverse()
    mag = np.asarray(mag, dtype=np.int64)
    hi = np.clip(np.searchsorted(values, mag), 1, len(values) - 1)
    pick = np.where(mag - values[hi - 1] <= values[hi] - mag, hi - 1, hi)
    return order[pick].astype("<u2").view(np.uint8)


def capture(mag, fmt):
    uc8 = uc8_of(mag)
    return uc8 if fmt == 0 else frames_util.to_sc16(uc8, q11=fmt == 2)


IQ_FLOOR = 400               # (the UC8 table's smallest entry is 363)
IQ_SAMPLES = 3 * B + 5000
IQ_VARIANTS = range(5)


def iq_magnitudes(variant):
    """The delayed magnitude stream (what the buffers' data[] arrays are cut from: 326 zeros, then the capture) of a capture of three
    buffers and a short tail.  Variant v = 0 .. 4 holds: a reply with F1 at delayed position B + v - 2 (data[v - 2] of buffer 1: -2 and
    -1 are buffer 0's last positions, 0 is never scanned) and one at 3 B + v - 2; a pair 69 + v % 3 apart across 2 B; a fifth of the
    tile-edge sweep (phases 0, 6, 12, 18, 24) and of 512 codes.  -> (stream, clean replies built)."""
    m = np.full(TR + IQ_SAMPLES, IQ_FLOOR, dtype=np.uint16)
    f1, phase, code = [B + variant - 2, 3 * B + variant - 2], [0, 13], [0o1234, 0o4321]
    f1 += [2 * B - 30, 2 * B - 30 + 69 + variant % 3]
    phase += [0, 0]
    code += [0o1111, 0o2222]
    taken = np.array(f1)
    combos = [(j, p) for j in TILE_J for p in (0, 6, 12, 18, 24)][variant::5]
    k = 0
    for j, p in combos:                                      # tile edges inside the buffers, clear of the replies above
        while True:
            k += 1
            at = TILE * k - j
            if at + 200 < TR + IQ_SAMPLES - 3000 and np.abs(taken - at).min() > 300:
                break
        f1.append(at), phase.append(p), code.append((k * 37) % 4096)
    assert k < 3 * B // TILE
    ncodes = 0
    at = TILE // 2
    for i in range(variant, 512, 5):                          # codes in the middle of tiles
        f1.append(at), phase.append(0), code.append((i * 8 + variant) % 4096)
        at += TILE
        ncodes += 1
    assert at < 3 * B
    replies(m, SAMPLE * np.array(f1) + np.array(phase), bits20_of(code_of(np.array(code), np.array(code) & 1)), AMPLITUDE)
    m[:TR] = 0
    return m, len(f1)


def iq_capture(variant, fmt):
    m, built = iq_magnitudes(variant)
    return capture(m[TR:], fmt), built


def found_positions(msgs):
    """Delayed positions of the F1s of the replies in a message list, for replies built at phase 0 (f2_clock = 25 f1 + 1218; the
    timestamp is the buffer's plus f2_clock / 5, and a buffer's data[i] is delayed position buffer start + i)."""
    ac = msgs[msgs["msgtype"] == 77]
    return set(((ac["timestamp"] - 243) // 5).tolist())


def check_iq_conditions(variant, msgs, built):
    nac = int((msgs["msgtype"] == 77).sum())
    assert 2 * nac >= built, f"the checker accepts {nac} of {built} replies"
    found = found_positions(msgs)
    assert (B + variant - 2 in found) == (variant != 2), "F1 at a buffer's data[0] is never scanned; its neighbours are"
    assert 2 * B - 30 in found and 2 * B - 30 + 69 + variant % 3 in found, "a reply behind a buffer edge is not hidden"


def check_capacity_conditions(msgs):
    nac = int((msgs["msgtype"] == 77).sum())
    assert nac >= CAPACITY_SAMPLES // 70 // 2, f"only {nac} replies in the capacity capture"


CAPACITY_SAMPLES = 64 * B - 1000


@functools.lru_cache(maxsize=None)
def capacity_capture():
    """Replies 70 samples apart over a whole chunk of 64 buffers (the last one short), UC8: as dense as accepted replies get.  On the
    IQ entry the noise level comes from the buffer's own mean level and power, so the replies carry few pulses (code 0, every fourth
    a code of one pulse): with more of them on the air the framing pulses are no longer 6 dB above that level."""
    m = np.full(CAPACITY_SAMPLES, IQ_FLOOR, dtype=np.uint16)
    f1 = np.arange(10, CAPACITY_SAMPLES - 100, 70)
    i = f1 // 70
    one_pulse = np.array(sorted(v for k, v in CODE_BIT.items() if k != "SPI"))
    replies(m, SAMPLE * f1, bits20_of(np.where(i % 4 == 0, one_pulse[i // 4 % 12], 0)), AMPLITUDE)
    return uc8_of(m)
