"""Filter scripts: captures in which the ICAO filter decides, driven the way a host that keeps its own filter drives the library
(mgpu_filter_expire / mgpu_filter_add).  tests/test_oracle_filter_script.py pins the two CPU checkers to each
other on them and checks that every one separates what it claims; tests/test_gpu_filter_clock.py runs them through the library.

A script is a list of ("feed", iq) / ("expire",) / ("add", addr) in stream order (helpers.oracle_stream) with a clock mode
(mgpu_config.filter_clock).  Every scenario here is noise-free UC8, one frame per 360 samples with the five sub-sample alignments
rotating, at most 8 buffers of 131072 samples, the last one short.  A scenario's `without` is the same capture under the script
with the operation in question taken out: what the per-feed message counts must differ from."""
import functools

import numpy as np

import frames_util as fr
import helpers

B = helpers.BUF_SAMPLES
SHOW_ONLY = helpers.SHOW_ONLY
AP_DFS = np.array([0, 4, 5, 16, 20, 21])
PER_BUFFER = (B - 2 * fr.LEAD) // fr.SPACING          # frames a buffer has room for: none comes near a buffer's edge
FOREIGN, HEARD = 0x3C4A5B, 0x4B1801                   # FOREIGN is never on the air as DF11 / DF17: only the host adds it
BIG = 0x01000000 | 0x2A5A5A                           # an address >= 2^24: no frame carries it, but it takes a bucket of the table


def _none():
    return np.zeros((0, 14), dtype=np.uint8), np.zeros(0, dtype=np.int64)


def cat(*parts):
    """parts of (frames (n, 14), nbits) -> one buffer's frames in transmission order."""
    parts = [(np.asarray(f, dtype=np.uint8).reshape(-1, 14), np.broadcast_to(nb, (len(f),)).astype(np.int64)) for f, nb in parts]
    return np.concatenate([p[0] for p in parts] or [_none()[0]]), np.concatenate([p[1] for p in parts] or [_none()[1]])


def ap(addrs, dfs=AP_DFS, seed=0):
    """Address/Parity frames: every DF of dfs for every address, address-major."""
    addrs = np.atleast_1d(np.asarray(addrs, dtype=np.uint32))
    df = np.tile(np.asarray(dfs), len(addrs))
    return fr.ap_frames(df, np.repeat(addrs, len(dfs)), payload_seed=seed), np.where(df >= 16, 112, 56)


def df11(addrs, iid=0):
    addrs = np.atleast_1d(np.asarray(addrs, dtype=np.uint32))
    return fr.df11_frames(addrs, iid), np.full(len(addrs), 56)


def df17(addrs, first=0):
    addrs = np.atleast_1d(np.asarray(addrs, dtype=np.uint32))
    return fr._es_frames(len(addrs), first, addrs, np.zeros(len(addrs), dtype=bool)), np.full(len(addrs), 112)


def modulate_buffers(buffers):
    """buffers: [(frames, nbits)] -> the UC8 capture: buffer b's frame i starts LEAD + 360 * i samples into the buffer at alignment
    (i + b) % 5; every buffer but the last is 131072 samples, the last ends LEAD samples behind its last frame."""
    frames, nbits, start, amp = [], [], [], []
    for b, (f, nb) in enumerate(buffers):
        n = len(f)
        assert n <= PER_BUFFER
        i = np.arange(n, dtype=np.int64)
        frames.append(f)
        nbits.append(nb)
        start.append((b * B + fr.LEAD + fr.SPACING * i) * fr.TICKS + (i + b) % fr.ALIGNMENTS)
        amp.append(fr.AMPLITUDES[(i + b) % len(fr.AMPLITUDES)])
    nlast = len(buffers[-1][0])
    nsamples = (len(buffers) - 1) * B + 2 * fr.LEAD + fr.SPACING * nlast
    assert nlast <= PER_BUFFER - 1                        # (ends short)
    return fr.modulate(np.concatenate(frames), np.concatenate(nbits), np.concatenate(start), np.concatenate(amp), nsamples=nsamples)


class Scenario:
    """spec: [("feed", [buffer, ...]) | ("expire",) | ("add", addr)], a buffer = (frames, nbits).  .ops = the script over the
    modulated capture, .without = dict of name -> the script with some operations / frames taken out (same buffer grid)."""

    def __init__(self, name, clock, spec, without=None, note=""):
        self.name, self.clock, self.spec, self.note = name, clock, spec, note
        self.without_spec = without or {}
        buffers = [b for op in spec if op[0] == "feed" for b in op[1]]
        assert 0 < len(buffers) <= 8
        self.nbuffers = len(buffers)

    @staticmethod
    def _script(spec):
        buffers = [b for op in spec if op[0] == "feed" for b in op[1]]
        iq = modulate_buffers(buffers)
        ops, k = [], 0
        for op in spec:
            if op[0] == "feed":
                ops.append(("feed", iq[2 * k * B:2 * (k + len(op[1])) * B]))
                k += len(op[1])
            else:
                ops.append(tuple(op))
        return ops

    @functools.cached_property
    def ops(self):
        return self._script(self.spec)

    @functools.cached_property
    def without(self):
        return {k: self._script(v) for k, v in self.without_spec.items()}

    def nfeeds(self):
        return sum(1 for op in self.spec if op[0] == "feed")


def in_format(ops, fmt):
    """The same script with every feed's UC8 samples as SC16 (1) or SC16Q11 (2)."""
    if fmt == 0:
        return ops
    return [("feed", fr.to_sc16(op[1], q11=fmt == 2)) if op[0] == "feed" else op for op in ops]


def drop(spec, *indices):
    """spec without the operations at these indices (none of them a feed)."""
    assert all(spec[i][0] != "feed" for i in indices)
    return [op for i, op in enumerate(spec) if i not in indices]


def counts(result):
    """Per-feed message counts of a checker's result."""
    return [len(m) for m, _ in result]


# ---- the scenarios ----

def _foreign_add():
    b0 = cat(df11(HEARD), ap(HEARD, seed=1), ap(FOREIGN, seed=2))
    both = [cat(ap(FOREIGN, seed=3 + k), ap(HEARD, seed=6 + k)) for k in range(3)]
    spec = [("add", SHOW_ONLY), ("feed", [b0]), ("add", FOREIGN), ("feed", [both[0]]), ("expire",), ("feed", [both[1]]), ("expire",),
            ("feed", [both[2]])]
    return Scenario("foreign_add", 2, spec, {"no_add": drop(spec, 2)})


def _foreign_add_late():
    b0 = cat(df11(HEARD), ap(FOREIGN, seed=11), ap(HEARD, seed=12))
    both = [cat(ap(FOREIGN, seed=13 + k), ap(HEARD, seed=17 + k)) for k in range(4)]
    spec = [("add", SHOW_ONLY), ("feed", [b0]), ("feed", [both[0]]), ("expire",), ("feed", [both[1]]), ("add", FOREIGN), ("feed", [both[2]]),
            ("expire",), ("feed", [both[3]])]
    return Scenario("foreign_add_late", 2, spec, {"no_add": drop(spec, 5)})


GEN = np.array([0x40621D, 0x4840D6, 0xA1B2C3, 0x780A0B], dtype=np.uint32)   # heard once / re-heard (DF17) / repaired DF11 / DF11 IID 5
REPAIRED_BIT = 36                                                           # (in the PI field: a one-bit entry of the short table)


def _generations():
    two = np.array([4, 20])
    b0 = cat(df11(GEN))

    def b1(rehear):
        parts = [ap(GEN, two, seed=21)]
        if rehear:
            parts.append(df17(GEN[1], first=3))
        parts += [(fr.flip(fr.df11_frames(GEN[2:3]), REPAIRED_BIT), 56), df11(GEN[3], iid=5)]
        return cat(*parts)
    b2, b3 = cat(ap(GEN, two, seed=22)), cat(ap(GEN, two, seed=23))

    def spec(rehear):
        return [("add", SHOW_ONLY), ("feed", [b0]), ("expire",), ("feed", [b1(rehear)]), ("expire",), ("feed", [b2]), ("expire",), ("feed", [b3])]
    return Scenario("generations", 2, spec(True), {"no_rehear": spec(False)})


GROW_A = (0x500000 + 0x0101 * np.arange(30)).astype(np.uint32)
GROW_NEW = (0x600000 + 0x0203 * np.arange(90)).astype(np.uint32)


def _grow_buffers():
    return cat(df11(GROW_A)), cat(df11(GROW_NEW[:80]), ap(GROW_A, [4], seed=31), df11(GROW_NEW[80:]), ap(GROW_A, [20], seed=32))


def _grow():
    b0, b1 = _grow_buffers()
    spec = [("add", SHOW_ONLY), ("feed", [b0]), ("expire",), ("feed", [b1])]
    return Scenario("grow", 2, spec, {"no_expire": drop(spec, 2), "two_expires": spec[:3] + [("expire",)] + spec[3:]})


SHRINK_C = (0x700000 + 0x0307 * np.arange(60)).astype(np.uint32)
SHRINK_D = (0x710000 + 0x0409 * np.arange(60)).astype(np.uint32)
SHRINK_E = (0x720000 + 0x050B * np.arange(90)).astype(np.uint32)


def _shrink():
    """After grow the table has 512 buckets.  The third expire comes after 20 inserts (C), fewer than 512 / 9, and halves it again;
    the fourth, after 60 (D), finds it at 256, where it cannot shrink.  So the 86th insert of the last buffer (E) grows it once more
    and drops the inactive generation (D), which a table still at 512 would have kept: `no_shrink`, where C has 60 addresses and the
    third expire leaves the table alone, accepts D's last frames.  `one_expire_fewer` keeps C known into the last buffer."""
    b0, b1 = _grow_buffers()

    def spec(nc):
        b2 = cat(df11(SHRINK_C[:nc]))
        b3 = cat(df11(SHRINK_D), ap(SHRINK_C[:20], [5], seed=41), ap(GROW_NEW[:10], [0], seed=42))
        b4 = cat(ap(SHRINK_D, [16], seed=43), ap(SHRINK_C[:20], [21], seed=44), df11(SHRINK_E), ap(SHRINK_D, [4], seed=45), ap(SHRINK_E[:5], [20], seed=46))
        return [("add", SHOW_ONLY), ("feed", [b0]), ("expire",), ("feed", [b1]), ("expire",), ("feed", [b2]), ("expire",), ("feed", [b3]), ("expire",),
                ("feed", [b4])]
    return Scenario("shrink", 2, spec(20), {"one_expire_fewer": drop(spec(20), 8), "no_shrink": spec(60)})


def _before_first(clock):
    b0, b1 = _grow_buffers()
    return Scenario(f"before_first_clock{clock}", clock, [("feed", [b0]), ("feed", [b1])])


def _fuzz(seed, clock):
    rng = np.random.default_rng(7000 + seed)
    pool = rng.choice(np.arange(1, 1 << 24), size=300, replace=False).astype(np.uint32)
    spoken = pool[:150]                                   # the rest is never sent as DF11 / DF17: known only where the host adds it
    favoured = pool[150:162]                              # ... and of it, the addresses the host adds most often
    buffers = []
    for b in range(8):
        n = int(rng.integers(150, 320)) if b < 7 else int(rng.integers(40, 200))
        kind = rng.choice(4, size=n, p=[0.25, 0.10, 0.60, 0.05])       # DF11 / DF17 / Address-Parity / DF11 with IID != 0
        anyone = np.where(rng.random(n) < 0.2, favoured[rng.integers(0, len(favoured), size=n)], pool[rng.integers(0, 300, size=n)])
        who = np.where(kind == 2, anyone, spoken[rng.integers(0, 150, size=n)]).astype(np.uint32)
        df = AP_DFS[rng.integers(0, 6, size=n)]
        iid = rng.integers(1, 64, size=n)
        frames, nbits = np.zeros((n, 14), dtype=np.uint8), np.full(n, 56)
        for k in range(4):
            sel = np.nonzero(kind == k)[0]
            if not len(sel):
                continue
            if k == 0:
                frames[sel] = fr.df11_frames(who[sel])
            elif k == 1:
                frames[sel], nbits[sel] = df17(who[sel], first=17 * b)
            elif k == 2:
                frames[sel], nbits[sel] = fr.ap_frames(df[sel], who[sel], payload_seed=100 * seed + b), np.where(df[sel] >= 16, 112, 56)
            else:
                frames[sel] = fr.df11_frames(who[sel], iid[sel])
        buffers.append((frames, nbits))
    # feeds of 1-3 buffers (redrawn until there are four of them at least, one of them longer than a buffer), 0-3 operations between
    # two feeds; a script whose draws left it with fewer than two expires (clock 2) or three adds gets them behind seeded feeds
    sizes = []
    while len(sizes) < 4 or max(sizes) < 2:
        sizes = []
        while sum(sizes) < 8:
            sizes.append(min(int(rng.integers(1, 4)), 8 - sum(sizes)))

    def add():
        return ("add", int(favoured[rng.integers(0, 12)] if rng.random() < 0.7 else pool[rng.integers(0, 300)]))
    spec, b = [("add", SHOW_ONLY)] if clock == 2 else [], 0
    for k, nb in enumerate(sizes):
        spec.append(("feed", buffers[b:b + nb]))
        b += nb
        for _ in range(int(rng.integers(0, 4)) if k + 1 < len(sizes) else 0):
            what = rng.choice(4, p=[0.45, 0.30, 0.10, 0.15])
            if what == 0 and clock == 2:
                spec.append(("expire",))
            elif what <= 1:
                spec.append(add())
            elif what == 2:
                spec.append(("add", SHOW_ONLY))
            else:
                spec.append(("add", BIG + int(rng.integers(0, 3))))

    def behind_a_feed(op):
        feeds = [i for i, o in enumerate(spec) if o[0] == "feed"][:-1]
        spec.insert(feeds[int(rng.integers(0, len(feeds)))] + 1, op)
    while clock == 2 and sum(1 for op in spec if op[0] == "expire") < 2:
        behind_a_feed(("expire",))
    while sum(1 for op in spec[1:] if op[0] == "add" and op[1] < (1 << 24)) < 3:
        behind_a_feed(add())
    return Scenario(f"fuzz{seed}", clock, spec)


TABLE = ("foreign_add", "foreign_add_late", "generations", "grow", "shrink", "before_first_clock0", "before_first_clock1")
FUZZ_SEEDS = (0, 1, 2, 3, 4, 5)
FUZZ_CLOCK = {0: 2, 1: 2, 2: 2, 3: 2, 4: 0, 5: 1}       # (clocks 0 and 1 take no expire from outside: their scripts only add)


@functools.lru_cache(maxsize=None)
def scenario(name):
    if name.startswith("fuzz"):
        return _fuzz(int(name[4:]), FUZZ_CLOCK[int(name[4:])])
    if name.startswith("before_first_clock"):
        return _before_first(int(name[-1]))
    return {"foreign_add": _foreign_add, "foreign_add_late": _foreign_add_late, "generations": _generations, "grow": _grow, "shrink": _shrink}[name]()


ALL = TABLE + tuple(f"fuzz{s}" for s in FUZZ_SEEDS)

# Per-feed message counts of the reference's own objects (oracle/_ref) on the table's scenarios: the scenario's own script, then each
# `without` script.  Recorded constants: they hold whichever checker a test run has at hand.
RECORDED = {
    "foreign_add": ([7, 12, 12, 0], {"no_add": [7, 6, 6, 0]}),
    "foreign_add_late": ([7, 6, 6, 12, 6], {"no_add": [7, 6, 6, 6, 0]}),
    "generations": ([4, 11, 2, 0], {"no_rehear": [4, 10, 0, 0]}),
    "grow": ([30, 120], {"no_expire": [30, 150], "two_expires": [30, 90]}),
    "shrink": ([30, 120, 20, 80, 155], {"one_expire_fewer": [30, 120, 20, 80, 235], "no_shrink": [30, 120, 60, 80, 215]}),
    "before_first_clock0": ([30, 120], {}),
    "before_first_clock1": ([30, 150], {}),
}
# demod_rejected_unknown_icao at the end of the two before_first runs (with the totals above: 150 / 180 messages).  The counter also
# counts the losing phases and neighbouring preamble positions of a frame, so it depends on payloads and alignments, not only on how
# many frames met an unknown address; these are the values of this capture.
RECORDED_UNKNOWN = {"before_first_clock0": 204, "before_first_clock1": 130}


@functools.lru_cache(maxsize=None)
def reference(name, fmt=0, nfix=1, mode_ac=0, which=None):
    """What the checker (helpers.reference_run) makes of a scenario's script, or of its `without` script named by which: computed
    once per test session.  -> [(messages, counters)] per feed."""
    s = scenario(name)
    ops = s.ops if which is None else s.without[which]
    return helpers.reference_run(None, fmt, nfix, 1, 58, mode_ac=mode_ac, ops=in_format(ops, fmt), filter_clock=s.clock)
