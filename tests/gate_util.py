"""The first-stage tracking gate: inputs from a message list, the oracle's verdicts, the goldens."""
import ctypes as C
import os

import numpy as np

import fields_util as fu
import helpers

BUF = 131072
F_CPR_VALID = 1 << 10
CASES = {   # name -> (synth kwargs, oracle options): tests/golden/make_gate_golden.py
    "uc8_fix_2s": (dict(seconds=2.0, seed=99, rate=1500.0), dict(nfix=1, mode_ac=0)),
    "uc8_aggressive_modeac_3s": (dict(seconds=3.0, seed=98, rate=700.0, dense=2), dict(nfix=2, mode_ac=1)),
    "uc8_fix_200ac_60s": (dict(seconds=60.0, seed=4242, rate=2000.0), dict(nfix=1, mode_ac=0)),
    "uc8_fix_30000ac_130s": (dict(seconds=130.0, seed=777, rate=2500.0, naircraft=30000), dict(nfix=1, mode_ac=0)),
}


def golden_forwarded(name):
    z = np.load(os.path.join(helpers.GOLDEN_DIR, f"gate_{name}.npz"))
    n = int(z["n"])
    return np.unpackbits(z["forwarded"])[:n].astype(bool)


def oracle_messages(name):
    kw, opt = CASES[name]
    iq = helpers.synth(threads=8, **kw)
    msgs, _ = helpers.oracle_run(iq, 0, opt["nfix"], 1, 58, mode_ac=opt["mode_ac"])
    fields = fu.oracle_fields(np.ascontiguousarray(msgs["msg"]), msgs["msgbits"].astype(np.int32))
    return iq, msgs, fields


def oracle_gate(msgs, fields, state=None):
    """modes_oracle_gate_run on an oracle message list (+ its field records) -> verdict bytes."""
    lib = helpers.oracle_lib()
    lib.modes_oracle_gate_new.restype = C.c_void_p
    lib.modes_oracle_gate_free.argtypes = [C.c_void_p]
    lib.modes_oracle_gate_run.argtypes = [C.c_void_p, C.c_uint64] + [C.c_void_p] * 8
    n = len(msgs)
    own = state is None
    g = lib.modes_oracle_gate_new() if own else state
    arr = dict(msgtype=msgs["msgtype"].astype(np.uint8), addr=np.ascontiguousarray(fields["addr"], dtype=np.uint32), iid=np.ascontiguousarray(fields["IID"], dtype=np.uint8),
               cb=msgs["correctedbits"].astype(np.uint8), cpr=((fields["flags"] & F_CPR_VALID) != 0).astype(np.uint8),
               now=(msgs["sys_rel_ms"].astype(np.int64) + helpers.STARTUP_MS), buffer=(((msgs["timestamp"].astype(np.int64) - 772) // 5) // BUF).astype(np.uint64))
    out = np.zeros(n, dtype=np.uint8)
    lib.modes_oracle_gate_run(g, n, *[C.c_void_p(arr[k].ctypes.data) for k in ("msgtype", "addr", "iid", "cb", "cpr", "now", "buffer")], C.c_void_p(out.ctypes.data))
    if own:
        lib.modes_oracle_gate_free(g)
    return out


def oracle_gate_new():
    lib = helpers.oracle_lib()
    lib.modes_oracle_gate_new.restype = C.c_void_p
    return lib.modes_oracle_gate_new()


def oracle_gate_free(state):
    lib = helpers.oracle_lib()
    lib.modes_oracle_gate_free.argtypes = [C.c_void_p]
    lib.modes_oracle_gate_free(state)


def oracle_gate_raw(msgtype, addr, iid, cb, cpr, now_ms, buffer, state=None):
    """modes_oracle_gate_run on plain arrays (a fresh table; state: a table from oracle_gate_new, carried from call to call)."""
    lib = helpers.oracle_lib()
    lib.modes_oracle_gate_new.restype = C.c_void_p
    lib.modes_oracle_gate_free.argtypes = [C.c_void_p]
    lib.modes_oracle_gate_run.argtypes = [C.c_void_p, C.c_uint64] + [C.c_void_p] * 8
    arrs = [np.ascontiguousarray(msgtype, dtype=np.uint8), np.ascontiguousarray(addr, dtype=np.uint32), np.ascontiguousarray(iid, dtype=np.uint8),
            np.ascontiguousarray(cb, dtype=np.uint8), np.ascontiguousarray(cpr, dtype=np.uint8), np.ascontiguousarray(now_ms, dtype=np.int64),
            np.ascontiguousarray(buffer, dtype=np.uint64)]
    n = len(arrs[0])
    out = np.zeros(n, dtype=np.uint8)
    g = lib.modes_oracle_gate_new() if state is None else state
    lib.modes_oracle_gate_run(g, n, *[C.c_void_p(a.ctypes.data) for a in arrs], C.c_void_p(out.ctypes.data))
    if state is None:
        lib.modes_oracle_gate_free(g)
    return out


def oracle_gate_stepped(raw, cuts=()):
    """The restatement over one list in several calls on one table: cuts = the indices at which a new call begins."""
    edges = [0] + [int(c) for c in cuts] + [len(raw["msgtype"])]
    g = oracle_gate_new()
    try:
        parts = [oracle_gate_raw(state=g, **{k: v[a:b] for k, v in raw.items()}) for a, b in zip(edges[:-1], edges[1:]) if b > a]
    finally:
        oracle_gate_free(g)
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)


def synthetic_list(n, seconds, naircraft, seed, startup_ms=helpers.STARTUP_MS if hasattr(helpers, "STARTUP_MS") else 0, cpr_unreliable=0.0):
    """A message list that never saw a sample: what the gate reads of mgpu_msg / mgpu_fields (timestamp on the ifile grid, sysTimestamp,
    msgtype, correctedbits; addr, IID, the CPR flag) for `naircraft` aircraft over `seconds` — long gaps, hours of life, non-ICAO
    addresses, Address/Parity formats with address 0, bursts of more than 256 messages in a buffer.
    cpr_unreliable: the share of the messages WITHOUT a reliable address (DF4 / DF20, DF11 with IID != 0) that carry the CPR flag all
    the same — the field decode never sets it there, mgpu_track_gate_device takes the records from the caller."""
    import readsb_amd
    rng = np.random.default_rng(seed)
    pos = np.sort(rng.integers(0, int(seconds * 2.4e6), size=n)).astype(np.int64)
    pos[n // 3: n // 3 + 700] = pos[n // 3]                                           # one buffer with three batches and a bit
    pos = np.sort(pos)
    ac = rng.integers(0, naircraft, size=n)
    quiet = rng.random(naircraft) < 0.3                                              # aircraft that go silent for long stretches
    keep = ~(quiet[ac] & ((pos // int(400 * 2.4e6)) % 2 == 1))
    pos, ac = pos[keep], ac[keep]
    n = len(pos)
    addr = (0x400000 + ac).astype(np.uint32)
    addr[ac % 17 == 3] |= 1 << 24                                                     # MODES_NON_ICAO_ADDRESS
    addr[ac == 5] = 0
    kind = rng.integers(0, 100, size=n)
    msgtype = np.select([kind < 45, kind < 60, kind < 75, kind < 90], [17, 11, 4, 20], 0).astype(np.uint8)
    iid = np.where((msgtype == 11) & (rng.random(n) < 0.3), rng.integers(1, 16, size=n), 0).astype(np.uint8)
    cpr = ((msgtype == 17) & (rng.random(n) < 0.6)).astype(np.uint8)
    cpr[(ac % 5 == 0) & (msgtype == 17)] = 1                                          # aircraft whose every DF17 is a position message
    cb = np.select([rng.random(n) < 0.85, rng.random(n) < 0.7], [0, 1], 2).astype(np.uint8)
    msgs = np.zeros(n, dtype=readsb_amd.MSG_DTYPE)
    msgs["timestamp"] = pos * 5 + 768 + rng.integers(4, 9, size=n)
    if cpr_unreliable:                                                                # (drawn last: the lists without it stay what they were)
        cpr[((msgtype == 4) | (msgtype == 20) | ((msgtype == 11) & (iid != 0))) & (rng.random(n) < cpr_unreliable)] = 1
    msgs["sysTimestamp"] = startup_ms + msgs["timestamp"] // 12000
    msgs["msgtype"], msgs["correctedbits"], msgs["msgbits"], msgs["addr"] = msgtype, cb, np.where(msgtype >= 16, 112, 56), addr
    fields = np.zeros(n, dtype=readsb_amd.FIELDS_DTYPE)
    fields["addr"], fields["IID"], fields["flags"], fields["msgtype"] = addr, iid, cpr.astype(np.uint32) * F_CPR_VALID, msgtype
    raw = dict(msgtype=msgtype, addr=addr, iid=iid, cb=cb, cpr=cpr, now_ms=msgs["sysTimestamp"].astype(np.int64), buffer=(pos // BUF).astype(np.uint64))
    return msgs, fields, raw


def check_against_golden(verdict, forwarded, max_deferred_share):
    """Every verdict that is not `deferred` must be what the whole reference program did."""
    v = verdict & 3
    certain = v != 2
    wrong = np.nonzero(certain & ((v == 1) != forwarded))[0]
    assert len(wrong) == 0, f"{len(wrong)} certain verdicts differ from the reference program's, first at message {wrong[:5]}"
    share = float((~certain).sum()) / max(1, len(v))
    assert share <= max_deferred_share, f"deferred share {share:.4f}"
    return share


# ---- built lists: which message sits where (tests/test_oracle_gate_built.py, tests/test_gpu_gate_built.py) ----
START = helpers.STARTUP_MS
MS = 2400                                # samples per millisecond of the stream's clock


class ListBuilder:
    """Rows (sample position, now_ms, msgtype, addr, IID, CPR flag, correctedbits, phase) in any order -> (msgs, fields, raw) in
    synthetic_list's form, sorted stably by position.  timestamp = position * 5 + 768 + phase (4..8); sysTimestamp = now_ms, which
    must not decrease along the list.  add() / at() return the row's serial number; index[serial] is its place in the built list."""

    def __init__(self):
        self.rows = []
        self._at = {}
        self.index = None

    def add(self, pos, now_ms, msgtype, addr, iid=0, cpr=0, cb=0, phase=4):
        assert 4 <= phase <= 8 and pos >= 0
        self.rows.append((int(pos), int(now_ms), int(msgtype), int(addr), int(iid), int(cpr), int(cb), int(phase)))
        return len(self.rows) - 1

    def at(self, now_ms, msgtype, addr, iid=0, cpr=0, cb=0):
        """A row on the stream's own clock: the k-th row asked for at now_ms sits at sample (now_ms - START) * 2400 + k."""
        k = self._at.get(now_ms, 0)
        assert k < MS and now_ms >= START
        self._at[now_ms] = k + 1
        return self.add((now_ms - START) * MS + k, now_ms, msgtype, addr, iid, cpr, cb, 4 + k % 5)

    def build(self):
        import readsb_amd
        n = len(self.rows)
        r = np.array(self.rows, dtype=np.int64).reshape(n, 8)
        order = np.argsort(r[:, 0], kind="stable")
        self.index = np.empty(n, dtype=np.int64)
        self.index[order] = np.arange(n)
        r = r[order]
        pos, now, msgtype, addr, iid, cpr, cb, phase = (r[:, k] for k in range(8))
        assert (np.diff(now) >= 0).all(), "sysTimestamp decreases along the list"
        msgs = np.zeros(n, dtype=readsb_amd.MSG_DTYPE)
        msgs["timestamp"], msgs["sysTimestamp"] = pos * 5 + 768 + phase, now
        msgs["msgtype"], msgs["correctedbits"], msgs["addr"] = msgtype, cb, addr
        msgs["msgbits"] = np.where(msgtype == 77, 16, np.where(msgtype >= 16, 112, 56))
        fields = np.zeros(n, dtype=readsb_amd.FIELDS_DTYPE)
        fields["addr"], fields["IID"], fields["flags"], fields["msgtype"] = addr, iid, cpr.astype(np.uint32) * F_CPR_VALID, msgtype
        raw = dict(msgtype=msgtype.astype(np.uint8), addr=addr.astype(np.uint32), iid=iid.astype(np.uint8), cb=cb.astype(np.uint8),
                   cpr=cpr.astype(np.uint8), now_ms=now.copy(), buffer=(pos // BUF).astype(np.uint64))
        return msgs, fields, raw


class Case:
    """A built list, the calls it is handed over in (cuts: at buffer boundaries only), and the verdicts (bits 0-1) written by hand
    from the reference's lines for some of its messages: expect = [(index, verdict, what)]."""

    def __init__(self, builder, expect=(), cuts=(), mixed=False, note=None):
        self.msgs, self.fields, self.raw = builder.build()
        self.expect = [(int(builder.index[s]), v, what) for s, v, what in expect]
        self.cuts = [int(c) for c in cuts]
        self.mixed = mixed
        self.note = note or {}
        self.index = builder.index
        buf = self.raw["buffer"]
        for c in self.cuts:
            assert 0 < c < len(buf) and buf[c - 1] != buf[c], "a call begins inside a buffer"

    def row(self, i):
        r = self.raw
        return (f"message {i}: msgtype {r['msgtype'][i]} addr {int(r['addr'][i]):07x} IID {r['iid'][i]} cpr {r['cpr'][i]} correctedbits {r['cb'][i]} "
                f"now {int(r['now_ms'][i])} buffer {int(r['buffer'][i])}")


# -- the threshold pairs (part 2 of the issue): two aircraft, one with the tested message AT the limit, the other 1 ms beyond --
# kind -> (limit in ms, the referred message is a position message, the tested message (msgtype, correctedbits), verdict at the
# limit, verdict beyond it, bit 24 of the address).  Derived from the reference:
#   ttl_lo: two clean DF17 identification messages, the second at t: a->seen = t, a->messages = 2.  A DF4 (crc = the address != 0, so
#           not forwarded on its own) at t + 45000: `now - a->seen > 45 s` (track.c:1933) is false, a->messages++, forwarded; at
#           t + 45001 mm->aircraft stays NULL: not forwarded.
#   ttl_hi: the last message with a reliable address is a POSITION message at t; if the position tracker rolled it back, a->seen is the
#           identification message's of t - 1000.  The DF4 at t + 45000 is counted if the position stood and dropped if it did not
#           (46000 > 45000): deferred; at t + 45001 both say dropped: not forwarded.
#   remove: a DF17 with one corrected bit at t + 300000 behind a silence: `a->seen < now - 5 min` (track.c:2856-2864) is false, the
#           aircraft cannot have been deleted, a->messages > 1: forwarded; at t + 300001 it may have been, then a->messages = 1: deferred.
#   pos / pos_nonicao: one position message at t, clean identification messages every four minutes.  A reliable position can be that
#           of t at the earliest; removeStaleRange deletes the aircraft once it is older than an hour (30 minutes with bit 24 of the
#           address set, track.c:2835-2867).  At t + limit it cannot have: forwarded; 1 ms later it may have: deferred.
#   pos_again: the same with a second position message 1 s before the limit.  Had the tracker judged that one bad, the reliable position
#           would still be the first one's: the same verdicts — the timeout counts from the aircraft's FIRST position message.
KINDS = {
    "ttl_lo": (45000, 0, (4, 0), 1, 0, 0),
    "ttl_hi": (45000, 1, (4, 0), 2, 0, 0),
    "remove": (300000, 0, (17, 1), 1, 2, 0),
    "pos": (3600000, 1, (17, 1), 1, 2, 0),
    "pos_nonicao": (1800000, 1, (17, 1), 1, 2, 1),
    "pos_again": (3600000, 1, (17, 1), 1, 2, 0),
}
LEADS = (0, 1, 63)
BETWEENS = (0, 1, 62, 63, 64, 127)
KEEPALIVE_FIRST, KEEPALIVE_EVERY = 60000, 240000


def keepalives(kind):
    """(ms behind the referred message, CPR flag) of the identification messages that keep a position-timeout aircraft from the
    5-minute rule — t + 60 s, then every four minutes — and of pos_again's second position message."""
    limit = KINDS[kind][0]
    keep = [(dt, 0) for dt in range(KEEPALIVE_FIRST, limit, KEEPALIVE_EVERY)] if kind.startswith("pos") else []
    return keep + ([(limit - 1000, 1)] if kind == "pos_again" else [])


def pair_aircraft(b, kind, addr, beyond, t, lead, between):
    """One aircraft of a pair: `lead` messages before the referred one (a clean DF17 identification message 1 s earlier, then
    neutral DF4 1 ms before it), the referred message at t, `between` messages between it and the tested one (the keep-alive
    messages of the position timeout count among them — there cannot be fewer — the rest neutral DF4 at t), the tested message at
    t + limit + beyond.  -> (serial of the referred message, serial of the tested one, lead, between as built)."""
    limit, ref_is_pos, (t_type, t_cb), _, _, nonicao = KINDS[kind]
    addr |= nonicao << 24
    if lead:
        b.at(t - 1000, 17, addr)
    for _ in range(lead - 1):
        b.at(t - 1, 4, addr)
    ref = b.at(t, 17, addr, cpr=ref_is_pos)
    keep = keepalives(kind)
    for _ in range(max(0, between - len(keep))):
        b.at(t, 4, addr)
    for dt, cpr in keep:
        b.at(t + dt, 17, addr, cpr=cpr)
    tested = b.at(t + limit + beyond, t_type, addr, cb=t_cb)
    return ref, tested, lead, max(between, len(keep))


def pair_rows(b, kind, addr, t, lead=1, between=0):
    """Both aircraft of a pair (addr, addr + 1) -> the expectations of the two tested messages, the serials of the referred ones."""
    _, _, _, v_at, v_beyond, _ = KINDS[kind]
    ra, ta, _, _ = pair_aircraft(b, kind, addr, 0, t, lead, between)
    rb, tb, lead, between = pair_aircraft(b, kind, addr + 1, 1, t, lead, between)
    what = f"{kind} lead {lead} between {between}"
    return [(ta, v_at, what + " at the limit"), (tb, v_beyond, what + " 1 ms beyond")], (ra, rb), (ta, tb)


T_PAIRS = START + 400000


def case_pairs():
    """All five pairs in one list."""
    b, expect = ListBuilder(), []
    for k, kind in enumerate(KINDS):
        expect += pair_rows(b, kind, 0x4a0000 + 16 * k, T_PAIRS + 100 * k)[0]
    b.at(T_PAIRS, 4, 0x4affff)                           # an aircraft never heard with a reliable address: no aircraft at all
    return Case(b, expect, mixed=True)


def case_lanes(kind):
    """The lane matrix of one pair: every (lead, between) on an address pair of its own, all in one list."""
    b, expect, note = ListBuilder(), [], {}
    for c, (lead, between) in enumerate((l, w) for l in LEADS for w in BETWEENS):
        e, refs, tested = pair_rows(b, kind, 0x4b0000 + 2 * c, T_PAIRS + 10 * c, lead, between)
        expect += e
        note[(lead, between)] = (refs, tested)
    case = Case(b, expect, note=note)
    case.note = {k: (tuple(int(case.index[s]) for s in r), tuple(int(case.index[s]) for s in t)) for k, (r, t) in note.items()}
    return case


def case_pair_cut(kind):
    """A pair with the referred message the last of one call and the tested message the first of the next."""
    b = ListBuilder()
    expect, refs, tested = pair_rows(b, kind, 0x4c0000, T_PAIRS)
    b.build()
    cuts = sorted({int(b.index[refs[1]]) + 1, int(b.index[tested[0]])})
    return Case(b, expect, cuts=cuts)


# -- the batch cut: drainMessageBuffer takes a buffer's Mode S messages 256 at a time --
POOL = [(17, 0, 0, 0), (17, 0, 0, 1), (17, 0, 0, 2), (11, 0, 0, 0), (11, 5, 0, 0), (11, 0, 0, 1), (4, 0, 0, 0), (4, 0, 0, 1), (20, 0, 0, 0),
        (20, 0, 0, 2), (18, 0, 0, 1), (11, 9, 0, 2)]        # (msgtype, IID, CPR flag, correctedbits)
BATCH_CASES = [(255, (253, 254)), (256, (254, 255)), (257, (254, 255)), (257, (255, 256)), (512, (254, 255)), (512, (255, 256)), (513, (254, 255)),
               (513, (255, 256)), (513, (511, 512))]
BATCH_ADDR, BATCH_BUFFER = 0x4d1234, 3


def case_batch(n, ranks):
    """Buffer 3 holds n Mode S messages and five Mode A/C replies behind them; BATCH_ADDR's only two messages (DF17, one corrected
    bit) sit at `ranks`.  Around them: aircraft of every kind, 0x4d2222 with position messages only (a->messages in [0, 2])."""
    b = ListBuilder()
    base = BATCH_BUFFER * BUF
    now = lambda pos: START + pos // MS
    b.add(base - 5, now(base - 5), 17, 0x4d0001)                                 # the buffer before
    pair = []
    for r in range(n):
        pos = base + 7 * r
        if r in ranks:
            pair.append(b.add(pos, now(pos), 17, BATCH_ADDR, cb=1, phase=4 + r % 5))
        elif r in (10, 11):
            b.add(pos, now(pos), 17, 0x4d2222, cpr=1, cb=1)
        elif r == 12:
            b.add(pos, now(pos), 4, 0x4d2222)
        else:
            mt, iid, cpr, cb = POOL[(r * 7) % len(POOL)]
            b.add(pos, now(pos), mt, 0x4d0000 + r % 61, iid, cpr, cb, phase=4 + r % 5)
    ac = [b.add(base + 7 * n + j, now(base + 7 * n + j), 77, 0) for j in range(5)]
    b.add(base + BUF + 9, now(base + BUF + 9), 17, 0x4d0001, cb=1)               # the buffer behind
    inside = ranks[0] // 256 == ranks[1] // 256
    expect = [(pair[0], 1 if inside else 0, "the pair's first"), (pair[1], 1, "the pair's second")] + [(s, 1, "Mode A/C") for s in ac]
    return Case(b, expect, mixed=True, note=dict(inside=inside, pair=pair))


# -- buffers: the buffer a message is counted in --
BUFFER_KS = (1, 2, 3, 4096, 200000)


def case_buffers():
    """Per k three aircraft with two DF17 (one corrected bit) each: across the boundary (k * 131072 - 1 with phase 8, k * 131072 with
    phase 4: two buffers, two batches, the first sees a->messages == 1), both before it, both behind it."""
    b, expect = ListBuilder(), []
    now = lambda pos: START + pos // MS
    for j, k in enumerate(BUFFER_KS):
        for a, places in enumerate([((k * BUF - 1, 8), (k * BUF, 4)), ((k * BUF - 3, 8), (k * BUF - 2, 8)), ((k * BUF + 1, 4), (k * BUF + 2, 8))]):
            s = [b.add(pos, now(pos), 17, 0x4e0000 + 16 * j + a, cb=1, phase=ph) for pos, ph in places]
            expect += [(s[0], 0 if a == 0 else 1, f"k {k} places {places} first"), (s[1], 1, f"k {k} places {places} second")]
    return Case(b, expect)


# -- runs: one address with a chosen number of messages --
RUN_LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 192)
RUN_VARIANTS = {   # name -> (position messages at, (index, gap before it in ms), the last message is a position message)
    "a": ((0, 1), {63: 301000}, False),                   # first position message in lane 0, two in one step, a dead message in lane 63
    "b": ((63, 70, 71), {64: 301000, 128: 300001}, False),   # first position message in lane 63, a dead message in lane 0 of the next steps
    "c": ((), {60: 301000, 125: 45001}, True),            # a dead message in the step before, the first position message is the last message
}
T_RUNS = START + 1000000


def run_rows(b, addr, length, t, seed, variant, pool=POOL):
    """One address's messages: kinds drawn from `pool` (seeded), 0.2 to 3 s apart, now and then exactly 45000 / 45001 / 300000 /
    300001 ms; position messages and long gaps where the variant puts them."""
    pos_at, gap_at, last_pos = RUN_VARIANTS[variant]
    rng = np.random.default_rng(seed)
    for k in range(length):
        gap = int(rng.integers(200, 3000))
        if rng.random() < 0.06:
            gap = int(rng.choice([45000, 45001, 300000, 300001]))
        t += gap_at.get(k, gap)
        mt, iid, cpr, cb = pool[int(rng.integers(len(pool)))]
        if k in pos_at or (last_pos and k == length - 1):
            mt, iid, cpr, cb = 17, 0, 1, int(rng.integers(0, 3))
        b.at(t, mt, addr, iid, cpr, cb)


def case_run(length, variant):
    b = ListBuilder()
    run_rows(b, 0x4f0000 + length, length, T_RUNS, 100 + length, variant)
    return Case(b)


def case_runs(variant, pool=POOL, base=0x4f1000):
    """The nine lengths on nine addresses, interleaved."""
    b = ListBuilder()
    for j, length in enumerate(RUN_LENGTHS):
        run_rows(b, base + 256 * j, length, T_RUNS + 37 * j, 200 + length, variant, pool)
    b.at(T_RUNS, 4, base + 0xfff)                        # no aircraft at all
    return Case(b, mixed=True)


PRIMES = {   # name -> the earlier call's messages (ms before the run starts, msgtype, CPR flag)
    "alive": ((-10000, 17, 0), (-9000, 17, 0)),           # known, counted twice, heard 9 s ago
    "stale": ((-400000, 17, 0), (-399000, 17, 1)),        # known for certain, silent for more than 5 minutes, a position message on record
}


def case_primed(length, variant, prime):
    b = ListBuilder()
    addr = 0x4f8000 + length
    for dt, mt, cpr in PRIMES[prime]:
        b.at(T_RUNS + dt, mt, addr, cpr=cpr)
    run_rows(b, addr, length, T_RUNS, 300 + length, variant)
    return Case(b, cuts=[len(PRIMES[prime])])


# -- addresses and the sort --
SORT_BASE = 0x4840d6
ADDRESSES = [0x000000, 0x000001, 0x0000ff, 0x000100, 0xffffff, 0x1000000, 0x1000001, 0x1ffffff, SORT_BASE, SORT_BASE ^ 0x01, SORT_BASE ^ 0x80,
             SORT_BASE ^ 0x0100, SORT_BASE ^ 0x8000, SORT_BASE ^ 0x010000, SORT_BASE ^ 0x800000, SORT_BASE ^ 0x1000000, 0x4800d6, 0x48ffd6]
SORT_SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 8191, 8192, 8193, 16385)
SORT_LARGE = (100000, 5000)
SORT_POOL = POOL + [(17, 0, 1, 0), (17, 0, 1, 1), (4, 0, 0, 0), (20, 0, 0, 0)]


def case_addresses(n, naddr=None, seed=None):
    """n messages of the edge addresses and drawn ones (each address once before any twice), shuffled in time: 0 to 11 ms apart, now
    and then 301 s."""
    rng = np.random.default_rng(1000 + n if seed is None else seed)
    naddr = max(len(ADDRESSES), n // 4) if naddr is None else naddr
    extra = np.setdiff1d(rng.integers(0, 1 << 25, size=naddr + 64), ADDRESSES)[:naddr - len(ADDRESSES)]
    pool = np.concatenate([np.array(ADDRESSES, dtype=np.int64), rng.permutation(extra).astype(np.int64)])
    more = pool[rng.integers(0, len(pool), size=max(0, n - len(pool)))]
    edge = rng.random(len(more)) < 0.02                                            # a few messages for each edge address in a large list, too
    more[edge] = pool[rng.integers(0, len(ADDRESSES), size=int(edge.sum()))]
    addr = rng.permutation(np.concatenate([pool[:n], more]))
    gap = rng.integers(0, 12, size=n)
    gap[rng.random(n) < 0.0005] = 301000
    now = T_RUNS + np.cumsum(gap)
    kind = rng.integers(0, len(SORT_POOL), size=n)
    zero = np.nonzero(addr == 0)[0]
    kind[zero] = np.array([6, 8, 0, 7, 3, 9])[np.arange(len(zero)) % 6]              # address 0: Address/Parity formats (crc = 0) among its messages
    b = ListBuilder()
    for k in range(n):
        mt, iid, cpr, cb = SORT_POOL[kind[k]]
        b.at(int(now[k]), mt, int(addr[k]), iid, cpr, cb)
    return Case(b, mixed=n >= 8191)


# -- call cuts --
def case_callcut(seed=7):
    """About 40 000 messages over three hours in 2 500 buffers: 30 aircraft, bit 24 of the address on every fifth, every third silent for
    6 minutes out of 18, every fourth with position messages in its first minute only, every fourth with them throughout, one heard
    with a reliable address only now and then.  Handed over in one call, in two, and buffer by buffer."""
    rng = np.random.default_rng(seed)
    nbuf = 3 * 3600 * MS * 1000 // BUF
    bufs = np.sort(rng.choice(nbuf, size=2500, replace=False))
    b = ListBuilder()
    for bi in bufs:
        m = int(rng.integers(8, 25))
        offs = np.sort(rng.choice(BUF, size=m, replace=False))
        for off in offs:
            pos = int(bi) * BUF + int(off)
            t = pos // MS                                                         # ms since the start
            a = int(rng.integers(0, 30))
            if a % 3 == 1 and (t // 360000 + a) % 3 == 0:
                continue
            mt, iid, cpr, cb = POOL[int(rng.integers(len(POOL)))]
            if a % 7 == 6 and rng.random() < 0.9:
                mt, iid = 4, 0
            if mt == 17 and rng.random() < 0.5 and (a % 4 == 1 or (a % 4 == 0 and t < 60000)):
                cpr = 1
            b.add(pos, START + t, mt, 0x3c0000 + a + ((1 << 24) if a % 5 == 4 else 0), iid, cpr, cb, phase=4 + int(off) % 5)
    case = Case(b, mixed=True)
    buf = case.raw["buffer"]
    starts = np.nonzero(np.diff(buf) != 0)[0] + 1
    case.note = dict(two=[int(starts[len(starts) // 2])], each=[int(s) for s in starts])
    return case


# -- the host form: the same kind of list as sealed frames --
HOST_POOL = [p for p in POOL if p[0] != 18]


def case_host():
    return case_runs("b", HOST_POOL, base=0x471000)


def frames_of(case):
    """Sealed frames that decode to the case's rows: cpr_util.position_frames / ident_frames, frames_util.ap_frames / df11_frames."""
    import cpr_util as cu
    import frames_util as fr
    r = case.raw
    n = len(r["msgtype"])
    frames = np.zeros((n, 14), dtype=np.uint8)
    k = np.arange(n, dtype=np.uint64)
    for sel, make in [((r["msgtype"] == 17) & (r["cpr"] == 1), lambda s: cu.position_frames(r["addr"][s], (k[s] * 37) & 0x1ffff, (k[s] * 91) & 0x1ffff, k[s] & 1, 0)),
                      ((r["msgtype"] == 17) & (r["cpr"] == 0), lambda s: cu.ident_frames(r["addr"][s])),
                      ((r["msgtype"] == 4) | (r["msgtype"] == 20), lambda s: fr.ap_frames(r["msgtype"][s], r["addr"][s])),
                      (r["msgtype"] == 11, lambda s: fr.df11_frames(r["addr"][s], r["iid"][s]))]:
        if sel.any():
            frames[sel] = make(sel)
    assert ((frames[:, 0] >> 3) == r["msgtype"]).all()
    return frames


# -- every built list by name --
def built_cases():
    """name -> a function that builds the case (cached: a case is built once per process and never changed)."""
    c = {"pairs": case_pairs, "buffers": case_buffers, "callcut": case_callcut, "host": case_host}
    for kind in KINDS:
        c[f"lanes_{kind}"] = (lambda kind=kind: case_lanes(kind))
        c[f"cut_{kind}"] = (lambda kind=kind: case_pair_cut(kind))
    for n, ranks in BATCH_CASES:
        c[f"batch_{n}_{ranks[0]}"] = (lambda n=n, ranks=ranks: case_batch(n, ranks))
    for v in RUN_VARIANTS:
        c[f"runs_{v}"] = (lambda v=v: case_runs(v))
        for length in RUN_LENGTHS:
            c[f"run_{length}_{v}"] = (lambda length=length, v=v: case_run(length, v))
    for j, length in enumerate(RUN_LENGTHS):
        for prime in PRIMES:
            c[f"primed_{length}_{prime}"] = (lambda length=length, j=j, prime=prime: case_primed(length, "abc"[j % 3], prime))
    for n in SORT_SIZES:
        c[f"addr_{n}"] = (lambda n=n: case_addresses(n))
    c[f"addr_{SORT_LARGE[0]}"] = lambda: case_addresses(*SORT_LARGE)
    return c


_built = {}


def built_case(name):
    if name not in _built:
        _built[name] = built_cases()[name]()
    return _built[name]


def first_difference(case, got, want):
    bad = np.nonzero(got != want)[0]
    if not len(bad):
        return None
    i = int(bad[0])
    return f"{len(bad)} of {len(got)} verdicts differ, first at {case.row(i)}: got {got[i]:#04x} want {want[i]:#04x}"


def coverage_gaps(v):
    """What a list that mixes cases must hold: verdicts 0, 1 and 2; each of bits 2, 3 and 4 both set and clear."""
    gaps = [f"no verdict {k}" for k in (0, 1, 2) if not ((v & 3) == k).any()]
    gaps += [f"bit {bit} never {'set' if want else 'clear'}" for bit in (2, 3, 4) for want in (0, 1) if not (((v >> bit) & 1) == want).any()]
    return gaps
