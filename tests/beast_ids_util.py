"""The beast encoder's checker with the aggregator's two options on top of beast_util.beast_reference: --net-verbatim (payload
from raw[], both forwarding tests lifted: net_io.c:1662, 5846, 5869) and --net-receiver-id (the 0x1a 0xe3 prefix of
modesSendBeastOutput, net_io.c:1667-1690), plus a reader that follows readBeast's framing and its 0xe3 case.
tests/test_beast_ids_reference.py pins it (CPU); tests/test_gpu_aggregate.py compares the kernels with it, byte for byte."""
import numpy as np

import beast_util as bu

MASK64 = (1 << 64) - 1
PREFIX_MAX = 18


def prefix_bytes(rid):
    """0x1a 0xe3 + the id as 8 bytes big-endian, 0x1a doubled (net_io.c:1671-1679)."""
    out = bytearray(b"\x1a\xe3")
    for b in int(rid).to_bytes(8, "big"):
        out.append(b)
        if b == 0x1A:
            out.append(b)
    return bytes(out)


def beast_reference(msgs, verdict=None, net_rule=False, verbatim=False, ids=None, last_id=0):
    """-> (stream bytes, bytes per message (prefix + frame; 0: none), deferred[] {index, offset}, the writer's lastReceiverId
    behind the list, prefix bytes per message).

    A message is a CALLER when the reference would call modesSendBeastOutput for it.  verbatim: every message, nothing deferred,
    no correctedbits test.  ids: a caller whose id differs from the caller's before it (the first one: from last_id) gets the
    prefix — unless its length is not carried: it then writes nothing at all, but has moved lastReceiverId (the assignment at
    :1670 comes before the return at :1690)."""
    n = len(msgs)
    if verbatim:
        m = msgs.copy()
        m["msg"] = msgs["raw"]
        verdict = None
    else:
        m = msgs
    stream, length, deferred = bu.beast_reference(m, verdict, net_rule)
    if verdict is None:
        caller = np.ones(n, dtype=bool)
    else:
        wire_ok = (msgs["correctedbits"] < 2) if net_rule else np.ones(n, dtype=bool)
        caller = ((np.asarray(verdict).astype(np.uint8) & 3) == 1) & wire_ok
    plen = np.zeros(n, dtype=np.int64)
    if ids is None:
        return stream, length, deferred, int(last_id), plen
    ids = np.asarray(ids, dtype=np.uint64)
    ci = np.nonzero(caller)[0]
    cid = ids[ci]
    prev = np.concatenate([np.array([last_id], dtype=np.uint64), cid[:-1]])
    need = np.zeros(n, dtype=bool)
    need[ci] = cid != prev
    need &= length > 0
    final = int(cid[-1]) if len(ci) else int(last_id)
    start = np.cumsum(length) - length
    out, at = bytearray(), 0
    for k in np.nonzero(need)[0]:
        out += stream[at:int(start[k])]
        at = int(start[k])
        p = prefix_bytes(ids[k])
        out += p
        plen[k] = len(p)
    out += stream[at:]
    total = length + plen
    new_start = np.cumsum(total) - total
    # a deferred message's offset: where its frame (prefix first) would start — the bytes of everything before it
    d = deferred.copy()
    if len(d):
        before = np.concatenate([[0], np.cumsum(total)])
        d["offset"] = before[d["index"].astype(np.int64)]
    assert len(out) == int(total.sum()) and (not n or new_start[-1] + total[-1] == len(out))
    return bytes(out), total, d, final, plen


def read_beast(stream):
    """readBeast's framing (net_io.c: 0x1a, a type byte, then the type's payload with 0x1a 0x1a read as one byte) with its 0xe3
    case: the 8 id bytes set the receiver id of the frames that follow.  -> [(receiver id, the frame's bytes as sent)]; the id is 0
    until a prefix is seen (a fresh client)."""
    want = {ord("1"): 2, ord("2"): 7, ord("3"): 14, 0xE3: 1}      # message bytes behind timestamp + signal (0xe3: 8 in all)
    out, rid, i, n = [], 0, 0, len(stream)
    while i < n:
        assert stream[i] == 0x1A, (i, stream[i])
        typ = stream[i + 1]
        assert typ in want, (i, typ)
        need = 8 if typ == 0xE3 else 7 + want[typ]
        j, body = i + 2, bytearray()
        while len(body) < need:
            b = stream[j]
            if b == 0x1A:
                assert stream[j + 1] == 0x1A, (j, "unescaped 0x1a inside a frame")
                j += 1
            body.append(b)
            j += 1
        if typ == 0xE3:
            rid = int.from_bytes(bytes(body), "big")
        else:
            out.append((rid, bytes(stream[i:j])))
        i = j
    return out


HOSTILE_IDS = np.array([0, 0x1A1A1A1A1A1A1A1A, MASK64, 0x11, 0x1A00000000000022] + [0x1A << (8 * k) for k in range(8)]
                       + [(0x0102030405060708 & ~(0xFF << (8 * k))) | (0x1A << (8 * k)) for k in range(8)], dtype=np.uint64)


def ids_changing_every(n, every, seed=0):
    """One id per message from HOSTILE_IDS, a new draw (never the same twice in a row) every `every` messages; every <= 0: one id."""
    rng = np.random.default_rng(seed)
    if every <= 0:
        return np.full(n, HOSTILE_IDS[1], dtype=np.uint64)
    runs = -(-n // every)
    pick = rng.integers(0, len(HOSTILE_IDS), size=runs)
    same = np.nonzero(pick[1:] == pick[:-1])[0] + 1
    while len(same):
        pick[same] = (pick[same] + 1 + rng.integers(0, len(HOSTILE_IDS) - 1, size=len(same))) % len(HOSTILE_IDS)
        same = np.nonzero(pick[1:] == pick[:-1])[0] + 1
    return np.repeat(HOSTILE_IDS[pick], every)[:n]


def random_ids(n, seed):
    """Ids drawn freely from HOSTILE_IDS: runs of equal ids of every short length."""
    rng = np.random.default_rng(seed)
    return HOSTILE_IDS[rng.integers(0, len(HOSTILE_IDS), size=n)]
