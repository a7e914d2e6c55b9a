"""The beast wire encoder's checker and its inputs: a plain numpy reference of modesSendBeastOutput / netTimestamp
(net_io.c:1620-1714) with the forwarding rule of mgpu_beast_encode_gated* (the comment above k_beast_size, net_io.c:5846-5872)
on top, and seeded generators of record lists that no sample ever produced.  tests/test_beast_reference.py pins the reference
(CPU); tests/test_gpu_beast_records.py compares the kernels with it, byte for byte.

sig_len == 0 is the one input class no generator produces: the level is then an infinity or a NaN, whose conversion to int is
undefined in the reference's C, and include/modes_gpu.h documents sig_len as 134 or 268."""
import ctypes as C

import numpy as np

from readsb_amd.binding import DEFERRED_DTYPE as DEFERRED, MSG_DTYPE as MSG

BLOCK = 256                                    # messages per workgroup of k_beast_size / k_beast_write
SCAN_THREADS = 1024                            # threads of k_beast_scan
MGPU_E_OVERFLOW = -5
SIG_LENS = (1, 134, 268, 65535)
OTHER_MSGBITS = (0, 8, 24, 120, 255)           # lengths the format does not carry


def scan_per(n):
    """Entries per thread of k_beast_scan for a list of n messages."""
    blocks = -(-n // BLOCK)
    return -(-blocks // SCAN_THREADS)


def signal_byte(sumsq, sig_len):
    """net_io.c:1696-1700 on mm->signalLevel = sum / 65535 / 65535 / samples (demod_2400.c:447-448): IEEE double division, sqrt and
    round-half-even are what the C does.  -> (byte, the double it was rounded from)"""
    level = np.asarray(sumsq).astype(np.float64) / 65535.0 / 65535.0 / np.asarray(sig_len).astype(np.float64)
    x = np.sqrt(level) * 255
    sig = np.rint(x)
    sig = np.where((level > 0) & (sig < 1), 1.0, sig)
    sig = np.minimum(sig, 255.0)
    return sig.astype(np.uint8), x


def beast_reference(msgs, verdict=None, net_rule=False):
    """-> (stream bytes, frame length per message (0: no frame), deferred[] {index, offset})"""
    n = len(msgs)
    msg_len = msgs["msgbits"].astype(np.int64) // 8
    typ = np.select([msg_len == 7, msg_len == 14, msg_len == 2], [ord("2"), ord("3"), ord("1")], 0).astype(np.uint8)
    carried = typ != 0
    emit, deferred = carried.copy(), np.zeros(n, dtype=bool)
    if verdict is not None:
        v = np.asarray(verdict).astype(np.uint8) & 3
        wire_ok = (msgs["correctedbits"] < 2) if net_rule else np.ones(n, dtype=bool)
        emit = carried & (v == 1) & wire_ok
        deferred = carried & (v == 2) & wire_ok
    # the 21 payload bytes: timestamp, signal, message
    ts = msgs["timestamp"].astype(np.int64) & ((1 << 48) - 1)
    pay = np.zeros((n, 21), dtype=np.uint8)
    for k in range(6):
        pay[:, k] = (ts >> (40 - 8 * k)) & 0xFF
    pay[:, 6] = signal_byte(msgs["sig_sumsq"], msgs["sig_len"])[0]
    pay[:, 7:] = msgs["msg"]
    used = np.arange(21)[None, :] < (7 + msg_len)[:, None]
    esc = used & (pay == 0x1A)
    at = 2 + np.arange(21)[None, :] + np.cumsum(esc, axis=1) - esc          # where payload byte k goes: behind the doubled ones before it
    length = np.where(emit, 2 + 7 + msg_len + esc.sum(axis=1), 0)
    rows = np.zeros((n, 44), dtype=np.uint8)
    rows[:, 0], rows[:, 1] = 0x1A, typ
    r = np.broadcast_to(np.arange(n)[:, None], (n, 21))
    rows[r[used], at[used]] = pay[used]
    rows[r[esc], at[esc] + 1] = 0x1A
    stream = rows[np.arange(44)[None, :] < length[:, None]].tobytes()
    start = np.cumsum(length) - length
    out = np.zeros(int(deferred.sum()), dtype=DEFERRED)
    out["index"], out["offset"] = np.nonzero(deferred)[0], start[deferred]
    return stream, length, out


# ---- generators --------------------------------------------------------------------------------------------------------------------

def _sumsq_for(byte):
    """A (sig_sumsq, sig_len) pair whose signal byte is `byte`, by the reference's own rule."""
    s = int(round((byte / 255.0) ** 2 * 65535.0 ** 2 * 268)) if byte else 0
    assert int(signal_byte(np.uint64(s), np.uint16(268))[0]) == byte
    return s, 268


def signal_boundaries():
    """(sig_sumsq, sig_len) around every rounding boundary of the signal byte: for each length and each b = s + 0.5, s = 0 .. 254, the
    integers within +-2 of ceil((b / 255)^2 * 65535^2 * len) = ceil((2 s + 1)^2 * 257^2 * len / 4); 0 and 1; the largest sum with
    level <= 1; sums above it up to 2^64 - 1 (the cap, and the conversion of a 64-bit integer to double)."""
    sums, lens = [], []
    for ln in SIG_LENS:
        top = 65535 * 65535 * ln
        vals = {0, 1, top, top + 1, top + 2, 2 * top, (1 << 53) + 1, (1 << 63) - 1, 1 << 63, (1 << 63) + 1025, (1 << 64) - 1025, (1 << 64) - 1}
        for s in range(255):
            c = -(-((2 * s + 1) ** 2 * 257 * 257 * ln) // 4)
            vals.update(max(0, c + d) for d in (-2, -1, 0, 1, 2))
        sums += sorted(vals)
        lens += [ln] * len(vals)
    return np.array(sums, dtype=np.uint64), np.array(lens, dtype=np.uint16)


def signal_records(seed):
    """The boundary sums, one record each, on otherwise ordinary long / short / Mode A/C messages — 3 % of them of a length the
    format does not carry — and the ladder's records behind them."""
    rng = np.random.default_rng(seed)
    sums, lens = signal_boundaries()
    n = len(sums)
    m = np.zeros(n, dtype=MSG)
    m["sig_sumsq"], m["sig_len"] = sums, lens
    m["msgbits"] = np.where(rng.random(n) < 0.03, rng.choice(OTHER_MSGBITS, size=n), rng.choice([56, 112, 16], size=n))
    m["timestamp"] = rng.integers(0, 1 << 48, size=n)
    m["msg"] = rng.integers(0, 256, size=(n, 14))
    return np.concatenate([m, ladder()])


def ladder():
    """For each carried length and each e = 0 .. 7 + msg_len: a record whose first e payload bytes are 0x1a and no other, i.e. one
    frame of every length the format can produce (11 .. 20, 16 .. 30, 23 .. 44)."""
    out = []
    for msgbits in (16, 56, 112):
        msg_len = msgbits // 8
        for e in range(7 + msg_len + 1):
            m = np.zeros(1, dtype=MSG)
            pay = [0x1A if k < e else 0x19 + 2 * (k & 1) for k in range(21)]
            m["timestamp"] = int.from_bytes(bytes(pay[:6]), "big")
            m["sig_sumsq"], m["sig_len"] = _sumsq_for(pay[6])
            m["msg"] = pay[7:]
            m["msgbits"] = msgbits
            out.append(m)
    return np.concatenate(out)


def with_ladder(m):
    """The ladder's records written over records of m, evenly spread (len(m) >= 1024)."""
    lad = ladder()
    assert len(m) >= 1024
    m[(np.arange(len(lad)) * (len(m) // len(lad))) + len(m) // (2 * len(lad))] = lad
    return m


def hostile_records(n, seed):
    """n records of every class at once, the ladder's records spread evenly among them (n >= 1024)."""
    rng = np.random.default_rng(seed)
    m = np.zeros(n, dtype=MSG)
    kind = rng.random(n)
    m["msgbits"] = np.select([kind < 0.40, kind < 0.80, kind < 0.94], [56, 112, 16], rng.choice(OTHER_MSGBITS, size=n))
    # timestamp: uniform over 48 bits | 0x1a in one byte position | in all six | at and above 2^48 | negative
    ts = rng.integers(0, 1 << 48, size=n)
    kind = rng.random(n)
    one = (kind >= 0.40) & (kind < 0.64)
    sh = 8 * rng.integers(0, 6, size=n)
    ts = np.where(one, (ts & ~(np.int64(0xFF) << sh)) | (np.int64(0x1A) << sh), ts)
    ts = np.where((kind >= 0.64) & (kind < 0.72), 0x1A1A1A1A1A1A, ts)
    high = rng.integers(1, 1 << 15, size=n) << 48
    ts = np.where((kind >= 0.72) & (kind < 0.86), ts | high, ts)
    ts = np.where((kind >= 0.86) & (kind < 0.88), 1 << 48, ts)
    ts = np.where(kind >= 0.88, (ts | high) + np.int64(-(1 << 63)), ts)          # negative: bit 63 set, any low 48 bits
    ts = np.where(kind >= 0.99, -1, ts)
    m["timestamp"] = ts
    # msg: random | all 0x1a | 0x1a at one position | its neighbours 0x19 / 0x1b, with and without it
    msg = rng.integers(0, 256, size=(n, 14)).astype(np.uint8)
    kind = rng.random(n)
    msg[(kind >= 0.35) & (kind < 0.50)] = 0x1A
    one = (kind >= 0.50) & (kind < 0.75)
    msg[one, rng.integers(0, 14, size=n)[one]] = 0x1A
    near = rng.choice(np.array([0x19, 0x1B], dtype=np.uint8), size=(n, 14))
    msg[(kind >= 0.75) & (kind < 0.85)] = near[(kind >= 0.75) & (kind < 0.85)]
    near3 = rng.choice(np.array([0x19, 0x1A, 0x1B], dtype=np.uint8), size=(n, 14))
    msg[kind >= 0.85] = near3[kind >= 0.85]
    m["msg"] = msg
    # signal: the boundary sums | sums that give the escaped byte | anything
    sums, lens = signal_boundaries()
    pick = rng.integers(0, len(sums), size=n)
    kind = rng.random(n)
    s26, l26 = _sumsq_for(0x1A)
    m["sig_sumsq"] = np.select([kind < 0.5, kind < 0.7], [sums[pick], np.uint64(s26)], rng.integers(0, 1 << 64, size=n, dtype=np.uint64))
    m["sig_len"] = np.select([kind < 0.5, kind < 0.7], [lens[pick], np.uint16(l26)], rng.choice(np.array(SIG_LENS, dtype=np.uint16), size=n))
    m["correctedbits"] = rng.integers(0, 3, size=n)
    m["msgtype"] = np.where(m["msgbits"] == 16, 77, np.where(m["msgbits"] == 112, 17, 11))
    return with_ladder(m)


def random_verdicts(n, seed):
    """Verdict bytes uniform over 0 .. 255: the bits above the lowest two must be ignored."""
    return np.random.default_rng(seed).integers(0, 256, size=n).astype(np.uint8)


def check_lengths(msgs, length=None):
    """What a generator's list must hold, asserted on the REFERENCE's output (`length`: its frame lengths, where the caller has
    them already): a frame of every length from 11 to 44 and no frame for at least 1 % of the records."""
    if length is None:
        _, length, _ = beast_reference(msgs)
    have = set(np.unique(length).tolist())
    assert set(range(11, 45)) <= have, sorted(set(range(11, 45)) - have)
    assert (length == 0).sum() >= 0.01 * len(msgs)


def check_gated(msgs, verdict, net_rule):
    """... and a gated case: at least 10 % each of frames, deferred and dropped, again by the reference."""
    _, length, deferred = beast_reference(msgs, verdict, net_rule)
    nf, nd = int((length > 0).sum()), len(deferred)
    assert min(nf, nd, len(msgs) - nf - nd) >= 0.10 * len(msgs), (nf, nd, len(msgs))


# ---- plain HIP allocations through the runtime the library itself is linked against ----------------------------------------------------

class Hip:
    def __init__(self):
        self.rt = C.CDLL("libamdhip64.so")
        self.rt.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.rt.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
        self.rt.hipFree.argtypes = [C.c_void_p]
        self.live = []

    def malloc(self, nbytes):
        p = C.c_void_p()
        assert self.rt.hipMalloc(C.byref(p), max(int(nbytes), 1)) == 0
        self.live.append(p.value)
        return p.value

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self.malloc(arr.nbytes)
        if arr.nbytes:
            assert self.rt.hipMemcpy(p, arr.ctypes.data, arr.nbytes, 1) == 0
        return p

    def fill(self, p, byte, nbytes):
        assert self.rt.hipMemset(p, byte, nbytes) == 0

    def download(self, p, nbytes, dtype=np.uint8):
        out = np.empty(int(nbytes) // np.dtype(dtype).itemsize, dtype=dtype)
        if out.nbytes:
            assert self.rt.hipMemcpy(out.ctypes.data, p, out.nbytes, 2) == 0
        return out

    def free(self, p):
        self.live.remove(p)
        self.rt.hipFree(p)

    def free_all(self):
        for p in list(self.live):
            self.free(p)


def encode_raw(d, d_msgs, n, d_out, cap, d_verdict=None, net_rule=False, d_deferred=None, deferred_cap=0):
    """The C entry itself, so that an error's outputs can be looked at: -> (return code, *bytes, *ndeferred)."""
    nb, nd = C.c_uint64(0), C.c_uint64(0)
    if d_verdict is None:
        rc = d.lib.mgpu_beast_encode_device(d.ctx, C.c_void_p(d_msgs), C.c_uint64(n), C.c_void_p(d_out), C.c_uint64(cap), C.byref(nb))
    else:
        rc = d.lib.mgpu_beast_encode_gated_device(d.ctx, C.c_void_p(d_msgs), C.c_void_p(d_verdict), C.c_uint64(n), C.c_uint32(1 if net_rule else 0),
                                                  C.c_void_p(d_out), C.c_uint64(cap), C.byref(nb), C.c_void_p(d_deferred), C.c_uint64(deferred_cap), C.byref(nd))
    return int(rc), int(nb.value), int(nd.value)
