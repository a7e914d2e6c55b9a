"""A frame modulator for tests, and the CRC-repair matrix capture built with it (tests/test_gpu_repair_matrix.py under -m gpu,
tests/test_oracle_repair_matrix.py on the CPU).

tools/synth_iq.c draws its traffic; here a test says exactly which frames are on the air, where and how strong: a list of (frame
bytes, 56 or 112 bits, start time in 12 MHz ticks, amplitude) becomes a UC8 capture, and SC16 / SC16Q11 by exact scaling.  The
envelope is synth_iq.c's (and SURVEY §8(d)'s): preamble pulses at 0, 1.0, 3.5 and 4.5 us, PPM data from 8 us, 0.5 us pulses on the
12 MHz tick grid, every 2.4 MSps sample the mean of its five ticks.  The signal is on I only, over a constant floor; noise-free unless
asked.  A start tick modulo 5 of 0..4 gives the five sub-sample alignments the reference's five slice_phase correlators are for.

numpy only; frames are sealed with fields_util (crc24_vec / seal) and cpr_util (position_frames / ident_frames)."""
import functools
import os

import numpy as np

import fields_util as fu
import helpers

TICKS = 5                    # 12 MHz ticks per 2.4 MSps sample
PULSE = 6                    # 0.5 us
PREAMBLE = (0, 12, 42, 54)   # 0, 1.0, 3.5, 4.5 us
DATA = 96                    # 8 us
FLOOR = 2.0                  # I at rest = 127.5 + FLOOR (+0.5 rounding) -> 130; Q stays at 128
SPACING = 360                # samples between frame starts in a capture of isolated frames (a long frame is 288)
LEAD = 400                   # samples before the first frame


def modulate(frames, nbits=None, start_tick=None, amplitude=None, nsamples=None, noise_lsb=0.0, seed=1):
    """frames: a list of (bytes, nbits, start_tick, amplitude), or an (n, 14) uint8 array with the three columns as arrays.
    -> the UC8 capture (uint8, I and Q interleaved).  Frames must not overlap (a pulse overwrites, it does not add).
    noise_lsb > 0: seeded uniform noise of +-noise_lsb LSB on I and on Q, as synth_iq.c adds it."""
    if nbits is None:
        lst = list(frames)
        fr = np.zeros((len(lst), 14), dtype=np.uint8)
        for i, f in enumerate(lst):
            b = np.frombuffer(bytes(f[0]), dtype=np.uint8)
            fr[i, :len(b)] = b
        nbits, start_tick, amplitude = (np.array([f[k] for f in lst]) for k in (1, 2, 3))
        frames = fr
    frames = np.ascontiguousarray(frames, dtype=np.uint8).reshape(-1, 14)
    nbits, start_tick = np.asarray(nbits, dtype=np.int64), np.asarray(start_tick, dtype=np.int64)
    amplitude = np.broadcast_to(np.asarray(amplitude, dtype=np.int64), nbits.shape)
    assert len(frames) == len(nbits) == len(start_tick) and ((nbits == 56) | (nbits == 112)).all()
    assert (amplitude > 0).all() and (amplitude + FLOOR + 128 <= 255).all() and (start_tick >= 0).all()
    order = np.argsort(start_tick, kind="stable")
    ends = start_tick[order] + DATA + 12 * nbits[order]
    assert (start_tick[order][1:] >= ends[:-1]).all(), "frames overlap"
    last = int(ends.max()) if len(ends) else 0
    if nsamples is None:
        nsamples = last // TICKS + LEAD
    assert nsamples * TICKS >= last + PULSE
    env = np.zeros(nsamples * TICKS, dtype=np.uint8)              # the envelope on the tick grid, in LSB
    for nb in (56, 112):
        idx = np.nonzero(nbits == nb)[0]
        if not len(idx):
            continue
        bits = np.unpackbits(frames[idx], axis=1)[:, :nb].astype(np.int64)
        data = DATA + 12 * np.arange(nb, dtype=np.int64)[None, :] + np.where(bits != 0, 0, 6)    # a 1 pulses in the first half of its bit
        pulses = start_tick[idx, None] + np.concatenate([np.broadcast_to(np.array(PREAMBLE), (len(idx), 4)), data], axis=1)
        amp = np.broadcast_to(amplitude[idx, None].astype(np.uint8), pulses.shape)
        for w in range(PULSE):
            env[pulses + w] = amp
    level = env.reshape(nsamples, TICKS).sum(axis=1, dtype=np.int64) / float(TICKS)              # box average over the sample's ticks
    vi = 127.5 + FLOOR + level
    vq = np.full(nsamples, 127.5 + 0.5)
    if noise_lsb > 0:
        rng = np.random.default_rng(seed)
        vi = vi + (rng.random(nsamples) * 2.0 - 1.0) * noise_lsb
        vq = vq + (rng.random(nsamples) * 2.0 - 1.0) * noise_lsb
    out = np.empty(2 * nsamples, dtype=np.uint8)
    out[0::2] = np.clip(np.floor(vi + 0.5), 0, 255).astype(np.uint8)
    out[1::2] = np.clip(np.floor(vq), 0, 255).astype(np.uint8)
    return out


def to_sc16(uc8, q11=False):
    """The same capture as SC16 (full scale 32768) or SC16Q11 (2048): (u - 127.5) * 256 or * 16, exact in 16 bits."""
    u = np.asarray(uc8, dtype=np.uint8).astype(np.int32)
    v = u * 16 - 2040 if q11 else u * 256 - 32640
    return v.astype("<i2").view(np.uint8)


def flip(frames, *bit_columns):
    """A copy of frames (n, 14) with frame bit b (0 = MSB of byte 0) of every row flipped, for each array of bits given (-1: none)."""
    out = np.array(frames, dtype=np.uint8, copy=True)
    rows = np.arange(len(out))
    for b in bit_columns:
        b = np.broadcast_to(np.asarray(b, dtype=np.int64), (len(out),))
        sel = b >= 0
        out[rows[sel], b[sel] >> 3] ^= (0x80 >> (b[sel] & 7)).astype(np.uint8)
    return out


def ap_frames(df, addr, nbits=None, payload_seed=0):
    """Address/Parity frames: random payload, parity = CRC XOR addr over nbits (default: 112 where bit 4 of the DF is set, else 56 —
    DF 0 4 5 / 16 20 21; any other DF value and length can be sealed the same way)."""
    df, addr = (np.atleast_1d(x).astype(np.uint32) for x in np.broadcast_arrays(df, addr))
    nbits = np.where(df >= 16, 112, 56) if nbits is None else np.broadcast_to(nbits, df.shape)
    rng = np.random.default_rng(1000 + payload_seed)
    fr = rng.integers(0, 256, size=(len(df), 14), dtype=np.uint8)
    fr[:, 0] = (df << 3) | (fr[:, 0] & 7)
    for nbytes in (7, 14):
        idx = np.nonzero(nbits == 8 * nbytes)[0]
        if not len(idx):
            continue
        sub = fr[idx]
        sub[:, nbytes - 3:] = 0
        par = fu.crc24_vec(sub, nbytes) ^ addr[idx]
        sub[:, nbytes - 3], sub[:, nbytes - 2], sub[:, nbytes - 1] = par >> 16, (par >> 8) & 0xFF, par & 0xFF
        fr[idx] = sub
    return fr


def df11_frames(addr, iid=0, ca=5):
    addr, iid, ca = (np.atleast_1d(x).astype(np.uint32) for x in np.broadcast_arrays(addr, iid, ca))
    fr = np.zeros((len(addr), 14), dtype=np.uint8)
    fr[:, 0] = (11 << 3) | ca
    fr[:, 1], fr[:, 2], fr[:, 3] = addr >> 16, (addr >> 8) & 0xFF, addr & 0xFF
    return fu.seal(fr, iid)


# ---- the repair matrix ----

TABLES = np.load(os.path.join(helpers.GOLDEN_DIR, "tables.npz"))     # the reference's own dump: rows (syndrome, nerrors, bit0, bit1)

# True addresses of the damaged frames (all primed into the ICAO filter first): AA bytes 0x00, 0xff and mixed, so that a repair inside
# AA meets 0 and 1 bits: four pairs of complements (an entry's frames at alignments 0 and 1 carry the two addresses of one pair).
# NEIGHBOUR == KNOWN[0] ^ 1: an Address/Parity frame of either with its last bit flipped passes as the other.
KNOWN = np.array([0x4B172A, 0xB4E8D5, 0x00FF5A, 0xFF00A5, 0xA5C300, 0x5A3CFF, 0x0000FF, 0xFFFF00], dtype=np.uint32)
NEIGHBOUR = 0x4B172B
PRIMED = np.concatenate([KNOWN, np.array([NEIGHBOUR], dtype=np.uint32)])
UNKNOWN_REPAIR = 0x3C66E1    # never sent clean: a repair inside AA that leads here stays outside the filter (mode_s.c:560)
UNKNOWN_GRID = 0x781234      # clean frames of an address the filter has not seen (its DF11 / DF17 then add it)
AMPLITUDES = np.array([48, 64, 90, 118])
ALIGNMENTS = 5

KINDS = ("primer", "long", "long_unknown", "short", "short2", "miss", "three", "dfbit", "dfbit2", "ap_flip", "grid")


def table_entries(name):
    """The entries of one reference table as a set of bit tuples: (b0,) or (b0, b1)."""
    return {(int(b0),) if n == 1 else (int(b0), int(b1)) for _, n, b0, b1 in TABLES[name]}


def _es_frames(n, first, addr, df18):
    """n DF17 frames (DF18 where df18), ME content rotating: airborne / surface positions over varying words, and identification."""
    import cpr_util
    k = first + np.arange(n, dtype=np.uint64)
    fr = cpr_util.position_frames(addr, (k * np.uint64(7919)) & np.uint64(0x1FFFF), (k * np.uint64(104729) + np.uint64(0x15555)) & np.uint64(0x1FFFF),
                                  k & np.uint64(1), (k % np.uint64(3)) == 0, df=np.where(df18, 18, 17), low3=np.where(df18, k % np.uint64(7), 5),
                                  movement=k % np.uint64(125))
    ident = (k % np.uint64(5)) == 4
    ident &= ~np.asarray(df18, dtype=bool)
    if ident.any():
        fr[ident] = cpr_util.ident_frames(np.broadcast_to(addr, (n,))[ident])
    return fr


class Matrix:
    """frames (n, 14), nbits, align, amplitude, kind (index into KINDS), entry (row of the table the frame was damaged by, or -1) in
    transmission order; .uc8 / .sc16 / .sc16q11 the captures."""

    def __init__(self, parts):
        self.frames = np.concatenate([p[0] for p in parts])
        n = len(self.frames)
        self.nbits = np.concatenate([np.broadcast_to(p[1], (len(p[0]),)) for p in parts]).astype(np.int64)
        self.align = np.concatenate([np.broadcast_to(p[2], (len(p[0]),)) for p in parts]).astype(np.int64)
        self.kind = np.concatenate([np.full(len(p[0]), KINDS.index(p[3])) for p in parts])
        self.entry = np.concatenate([np.broadcast_to(p[4], (len(p[0]),)) for p in parts]).astype(np.int64)
        self.amplitude = AMPLITUDES[np.arange(n) % len(AMPLITUDES)]
        self.start_tick = (LEAD + SPACING * np.arange(n, dtype=np.int64)) * TICKS + self.align
        self.nsamples = LEAD + SPACING * n + LEAD
        self.uc8 = modulate(self.frames, self.nbits, self.start_tick, self.amplitude, nsamples=self.nsamples)

    @functools.cached_property
    def sc16(self):
        return to_sc16(self.uc8)

    @functools.cached_property
    def sc16q11(self):
        return to_sc16(self.uc8, q11=True)

    def iq(self, fmt):
        return (self.uc8, self.sc16, self.sc16q11)[fmt]


@functools.lru_cache(maxsize=None)
def repair_matrix(nfix=2, drop_long_entry=None):
    """The capture for the nfix table (1: the one-bit tables, 2: --aggressive's; 0 has no table and takes 1's).  Every damaged frame is a
    valid frame of a KNOWN address with exactly the bits of one table entry flipped; see the module docstring of
    tests/test_gpu_repair_matrix.py for the order.  drop_long_entry: leave one row of the long table out (the sensitivity check)."""
    nfix = max(int(nfix), 1)
    tlong, tshort = TABLES[f"nfix{nfix}_112"], TABLES[f"nfix{nfix}_56"]
    rng = np.random.default_rng(20240 + nfix)
    parts = []            # (frames, nbits, align, kind, entry)
    nk = len(KNOWN)

    # primers: one clean DF17 and one clean DF11 (IID 0) per true address
    npr = len(PRIMED)
    parts.append((_es_frames(npr, 0, PRIMED, np.zeros(npr, dtype=bool)), 112, np.arange(npr) % ALIGNMENTS, "primer", -1))
    parts.append((df11_frames(PRIMED), 56, (np.arange(npr) + 2) % ALIGNMENTS, "primer", -1))

    # the long table: every entry at every alignment; every 8th entry DF18; address and ME rotate over entry and alignment
    rows = np.arange(len(tlong))
    if drop_long_entry is not None:
        rows = rows[rows != drop_long_entry]
    b0, b1 = tlong[rows, 2], np.where(tlong[rows, 1] == 2, tlong[rows, 3], -1)
    for a in range(ALIGNMENTS):
        addr = KNOWN[((2 * rows + 2 * (a // 2)) % nk) ^ (a & 1)]
        clean = _es_frames(len(rows), 10000 * a + 17, addr, (rows % 8) == 7)
        parts.append((flip(clean, b0, b1), 112, a, "long", rows))
    # ... and of an address the filter does not hold: a repair inside AA (bits 8..31) leads nowhere (every one-bit entry there, every
    # 8th two-bit one), a repair outside AA is accepted as it is (every 32nd of those, every 4th one-bit one)
    in_aa = ((b0 >= 8) & (b0 <= 31)) | ((b1 >= 8) & (b1 <= 31))
    sel = np.nonzero((in_aa & ((b1 < 0) | (rows % 8 == 3))) | (~in_aa & ((rows % 32 == 5) | ((b1 < 0) & (b0 % 4 == 0)))))[0]
    clean = _es_frames(len(sel), 77, np.full(len(sel), UNKNOWN_REPAIR, dtype=np.uint32), (rows[sel] % 8) == 7)
    parts.append((flip(clean, b0[sel], b1[sel]), 112, sel % ALIGNMENTS, "long_unknown", rows[sel]))

    # the short table: every one-bit entry in DF11, at every alignment, with IID 0, 1, 64, 127 (a nonzero IID moves the syndrome off the entry)
    one = np.nonzero(tshort[:, 1] == 1)[0]
    for iid in (0, 1, 64, 127):
        for a in range(ALIGNMENTS):
            addr = KNOWN[(one + a + iid) % nk]
            parts.append((flip(df11_frames(addr, iid, ca=(one + a) % 8), tshort[one, 2]), 56, a, "short", one))
    # DF11 with two flipped bits: dropped even where the table has the pair (2-bit errors are ambiguous in DF11)
    two = np.nonzero(tshort[:, 1] == 2)[0]
    if len(two):
        two = two[:: max(1, len(two) // 100)]
        pair = tshort[two, 2:4]
    else:
        pair = np.stack([5 + np.arange(40), 16 + np.arange(40)], axis=1)
    parts.append((flip(df11_frames(KNOWN[np.arange(len(pair)) % nk]), pair[:, 0], pair[:, 1]), 56, np.arange(len(pair)) % ALIGNMENTS, "short2", -1))
    # the two-bit entries of the other nfix: at nfix 1 (and 0) a sample of --aggressive's pairs, which must miss
    if nfix == 1:
        t2 = TABLES["nfix2_112"]
        miss = np.nonzero(t2[:, 1] == 2)[0][::12]
        clean = _es_frames(len(miss), 4242, KNOWN[miss % nk], (miss % 8) == 7)
        parts.append((flip(clean, t2[miss, 2], t2[miss, 3]), 112, miss % ALIGNMENTS, "miss", -1))

    # outside the tables: 300 DF17 frames with three flipped bits
    trip = np.sort(np.stack([rng.permutation(107)[:3] + 5 for _ in range(300)]), axis=1)
    clean = _es_frames(300, 31337, KNOWN[np.arange(300) % nk], np.zeros(300, dtype=bool))
    parts.append((flip(clean, trip[:, 0], trip[:, 1], trip[:, 2]), 112, np.arange(300) % ALIGNMENTS, "three", -1))
    # DF17 with one flip in bits 0..4 (fixDF17msgtype's case) at every alignment, known and unknown address; and with a second flip elsewhere
    j = np.repeat(np.arange(5), 2 * ALIGNMENTS)
    al = np.tile(np.repeat(np.arange(ALIGNMENTS), 2), 5)
    addr = np.where(np.arange(len(j)) % 2 == 0, KNOWN[j % nk], UNKNOWN_REPAIR).astype(np.uint32)
    clean = _es_frames(len(j), 555, addr, np.zeros(len(j), dtype=bool))
    parts.append((flip(clean, j), 112, al, "dfbit", -1))
    parts.append((flip(clean, j, 5 + (np.arange(len(j)) * 13) % 107), 112, al, "dfbit2", -1))
    # Address/Parity frames with one flip: a different address, which meets the filter (unknown, or — last bit, KNOWN[0] <-> KNOWN[1] — known)
    dfs = np.array([0, 4, 5, 16, 20, 21])
    for df in dfs:
        nb = 112 if df >= 16 else 56
        bits = np.concatenate([np.array([nb - 1, nb - 1]), 5 + (np.arange(8) * 11 + df) % (nb - 6)])
        addr = np.concatenate([[KNOWN[0], NEIGHBOUR], KNOWN[np.arange(8) % nk]])
        parts.append((flip(ap_frames(np.full(len(bits), df), addr, payload_seed=200 + int(df)), bits), nb, np.arange(len(bits)) % ALIGNMENTS, "ap_flip", -1))

    # the classification grid, clean, known and unknown address, every alignment
    for addr in (int(KNOWN[2]), UNKNOWN_GRID):
        for a in range(ALIGNMENTS):
            # every DF value 0..31 sealed as Address/Parity at its own length (bit 4 of the DF), and as if short and as if long
            alldf = np.arange(32)
            parts.append((ap_frames(alldf, addr, payload_seed=a), np.where(alldf >= 16, 112, 56), a, "grid", -1))
            parts.append((ap_frames(alldf[16:], addr, nbits=56, payload_seed=40 + a), 56, a, "grid", -1))
            parts.append((ap_frames(alldf[:16], addr, nbits=112, payload_seed=80 + a), 112, a, "grid", -1))
            # ... and with parity = CRC (syndrome 0), the DFs that are no format at all included
            parts.append((ap_frames(alldf, 0, payload_seed=120 + a), np.where(alldf >= 16, 112, 56), a, "grid", -1))
            # the frames that leave the parity field to a PI: DF11 (IID 0 and 5), DF17, DF18
            parts.append((df11_frames(np.full(2, addr, dtype=np.uint32), np.array([0, 5])), 56, a, "grid", -1))
            parts.append((_es_frames(2, 9 + a, np.full(2, addr, dtype=np.uint32), np.array([False, True])), 112, a, "grid", -1))
            # a DF11 whose only error lies inside the IID bits (49..55)
            parts.append((flip(df11_frames(np.full(7, addr, dtype=np.uint32)), 49 + np.arange(7)), 56, a, "grid", -1))
    # the all-zero frames
    parts.append((np.zeros((ALIGNMENTS, 14), dtype=np.uint8), 56, np.arange(ALIGNMENTS), "grid", -1))
    parts.append((np.zeros((ALIGNMENTS, 14), dtype=np.uint8), 112, np.arange(ALIGNMENTS), "grid", -1))
    return Matrix(parts)


# ---- what the reference made of it: one run per (nfix, fix_df, format, mode_ac) for the whole test session ----

@functools.lru_cache(maxsize=None)
def reference(nfix, fixdf=1, fmt=0, mode_ac=0):
    return helpers.reference_run(repair_matrix(nfix).iq(fmt), fmt, nfix, fixdf, 58, mode_ac=mode_ac)


def repaired_bits(msgs):
    """msg ^ raw of every message as a tuple of frame bit numbers."""
    x = np.unpackbits(np.ascontiguousarray(msgs["msg"]) ^ np.ascontiguousarray(msgs["raw"]), axis=1)
    return [tuple(np.nonzero(r)[0].tolist()) for r in x]


def coverage(msgs):
    """The coverage condition, from a message list alone.  -> (long entries found, short entries found): the repairs of the accepted
    DF17/18 messages with correctedbits 1 or 2 and of the accepted DF11 messages with correctedbits 1, as sets of bit tuples,
    without the repairs of fixDF17msgtype (one bit inside the DF field, bits 0..4, which no table holds)."""
    bits = repaired_bits(msgs)
    es = ((msgs["msgtype"] == 17) | (msgs["msgtype"] == 18)) & (msgs["correctedbits"] >= 1)
    s11 = (msgs["msgtype"] == 11) & (msgs["correctedbits"] == 1)
    for k in np.nonzero(es | s11)[0]:
        assert len(bits[k]) == msgs["correctedbits"][k], f"message {k}: correctedbits {msgs['correctedbits'][k]} but msg ^ raw = {bits[k]}"
    found_long = {bits[k] for k in np.nonzero(es)[0] if bits[k][0] >= 5}
    found_short = {bits[k] for k in np.nonzero(s11)[0]}
    return found_long, found_short


def frame_of(matrix, msgs):
    """Index (transmission order) of the frame each message was demodulated from: a message's timestamp is its frame's start plus
    8 + 56 us plus the 326 samples of overlap a buffer starts with (demod_2400.c:406 counts from there), give or take a few ticks,
    and frames start SPACING samples apart."""
    return (msgs["timestamp"] - (64 * 12 + 326 * TICKS) - LEAD * TICKS + SPACING * TICKS // 2) // (SPACING * TICKS)


# One-bit entries of the short table that no stream can reach, in the reference or anywhere: the syndromes of frame bits 49..55 are
# 0x40 .. 0x01, inside the seven IID bits, and DF11 — the only format that consults the short table — takes a syndrome with nothing
# outside those bits for an interrogator id, not for damage (mode_s.c: `if (crc & 0xffff80)` before modesChecksumDiagnose).  So a DF11
# with one of these bits flipped is accepted UNREPAIRED (correctedbits 0, IID = the syndrome), which check_coverage asserts in their
# place.  7 entries: 0.53 % of --aggressive's short table (1326), the table the 1 % allowance below is taken of.
SHORT_UNREACHABLE = [(49,), (50,), (51,), (52,), (53,), (54,), (55,)]
LONG_UNREACHABLE = []


def check_coverage(nfix, msgs, stats, long_entries=None, short_entries=None):
    """The coverage condition of the repair matrix on the REFERENCE's list for the nfix capture (never the product's): every entry of
    the long table (nfix 1: its 107 one-bit entries, nfix 2: all 3831) repaired in an accepted DF17/18, every one-bit entry of the
    short table repaired in an accepted DF11 — exactly those sets, nothing else — and every try-phase at least 10 % of the accepted."""
    assert nfix in (1, 2)
    m = repair_matrix(nfix)
    if long_entries is None:
        long_entries = table_entries(f"nfix{nfix}_112")
    if short_entries is None:
        short_entries = {e for e in table_entries(f"nfix{nfix}_56") if len(e) == 1}
    assert len(SHORT_UNREACHABLE) * 100 <= len(TABLES["nfix2_56"]) and len(LONG_UNREACHABLE) * 100 <= len(TABLES["nfix2_112"])
    found_long, found_short = coverage(msgs)
    want_long, want_short = long_entries - set(LONG_UNREACHABLE), short_entries - set(SHORT_UNREACHABLE)
    assert found_long == want_long, (f"long table: {len(want_long - found_long)} entries never repaired {sorted(want_long - found_long)[:8]}, "
                                     f"{len(found_long - want_long)} repairs outside the table {sorted(found_long - want_long)[:8]}")
    assert found_short == want_short, f"short table: never repaired {sorted(want_short - found_short)}, outside the table {sorted(found_short - want_short)}"
    accepted = int(np.sum(stats["demod_accepted"]))
    assert accepted == len(msgs) and (np.asarray(stats["demod_bestPhase"]) * 10 >= accepted).all(), stats["demod_bestPhase"]
    # the unreachable short entries: their frames (IID 0) come through as clean DF11 with the syndrome for an interrogator id
    idx = frame_of(m, msgs)
    own = np.isin(m.kind[idx], [KINDS.index(k) for k in ("primer", "long", "long_unknown", "short")])
    assert (m.nbits[idx] == msgs["msgbits"])[own].all()          # (elsewhere a short frame and the silence behind it can pass for a long one)
    sel = (m.kind[idx] == KINDS.index("short")) & (msgs["correctedbits"] == 0) & (msgs["msgtype"] == 11)
    got = {}
    for k in np.nonzero(sel)[0]:
        got.setdefault(int(m.entry[idx[k]]), set()).add(int(m.align[idx[k]]))
        assert (msgs["msg"][k] == msgs["raw"][k]).all()
    tshort = TABLES[f"nfix{nfix}_56"]
    for e in SHORT_UNREACHABLE:
        row = int(np.nonzero((tshort[:, 1] == 1) & (tshort[:, 2] == e[0]))[0][0])
        assert got.get(row) == set(range(ALIGNMENTS)), f"DF11 with bit {e[0]} flipped: accepted unrepaired at alignments {got.get(row)}"
    return len(found_long), len(found_short)
