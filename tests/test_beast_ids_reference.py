"""The checker of the beast encoder's aggregator options (tests/beast_ids_util.py), on the CPU: --net-verbatim pinned against the
whole reference program's streams (tests/golden/beast_verbatim_*.bin), the receiver-id prefix by a round trip through a reader
that follows readBeast."""
import os

import numpy as np
import pytest

import beast_ids_util as biu
import beast_util as bu
import helpers
from helpers import GOLDEN_BEAST
from test_beast_reference import _oracle_as_records


@pytest.mark.parametrize("name,synth_kw,opt", GOLDEN_BEAST)
def test_verbatim_reference_is_the_programs_verbatim_dump(built, name, synth_kw, opt):
    """--dump-beast of the whole reference program with --net-verbatim --net-receiver-id, byte for byte: a frame for EVERY accepted
    message (both forwarding tests lifted), the sliced bytes in place of the corrected ones — and no prefix at all: the messages'
    id is 0, and so is a fresh writer's."""
    gold = open(os.path.join(helpers.GOLDEN_DIR, f"beast_verbatim_{name}.bin"), "rb").read()
    o, _ = helpers.oracle_run(helpers.synth(**synth_kw), 0, opt["nfix"], 1, 58, mode_ac=opt["mode_ac"])
    msgs = _oracle_as_records(o)
    assert (msgs["msg"] != msgs["raw"]).any(axis=1).sum() >= 100            # the flag matters on this capture
    stream, length, deferred, last, plen = biu.beast_reference(msgs, verbatim=True, ids=np.zeros(len(msgs), dtype=np.uint64))
    assert stream == gold, (len(stream), len(gold))
    assert (length > 0).all() and len(deferred) == 0 and last == 0 and not plen.any()
    # verdicts and the network rule decide nothing under the flag
    v = bu.random_verdicts(len(msgs), 5)
    assert biu.beast_reference(msgs, v, net_rule=True, verbatim=True)[0] == gold
    assert bu.beast_reference(msgs)[0] != gold


def _round_trip(msgs, verdict, ids, last_id):
    stream, total, deferred, final, plen = biu.beast_reference(msgs, verdict, ids=ids, last_id=last_id)
    plain, length, _ = bu.beast_reference(msgs, verdict)
    start = np.cumsum(length) - length
    frames = [(k, plain[int(start[k]):int(start[k]) + int(length[k])]) for k in np.nonzero(length)[0]]
    got = biu.read_beast(stream)
    assert len(got) == len(frames)
    assert [f for _, f in got] == [f for _, f in frames]
    caller = np.ones(len(msgs), dtype=bool) if verdict is None else (np.asarray(verdict) & 3) == 1
    # the id the reader attributes a frame to: the id of the last PREFIX before it.  That is the frame's own id except behind a
    # caller that wrote nothing (a length the format does not carry) but moved the writer's id: from there to the next prefix
    rid, writer, shadowed, checked = int(last_id), int(last_id), 0, 0
    it = iter(got)
    for k in range(len(msgs)):
        if not caller[k]:
            assert total[k] == 0 or not length[k]
            continue
        mine = int(ids[k])
        if length[k] == 0:
            if mine != writer:
                shadowed += 1
            writer = mine                                   # nothing written, not even the prefix
            assert total[k] == 0
            continue
        if mine != writer:
            assert plen[k] == len(biu.prefix_bytes(mine))
            rid = writer = mine
        else:
            assert plen[k] == 0                             # ... so a same-id frame behind the quirk's record has no prefix
        seen, _ = next(it)
        if int(last_id) == 0 or checked or plen[k]:         # (before the first prefix the reader knows no id but a fresh client's 0)
            assert seen == rid
        checked += 1
    assert final == writer
    return shadowed, stream


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("gated", [False, True])
def test_prefix_round_trip(seed, gated):
    """The prefix rule rests on reading net_io.c:1667-1690, not on a run of the reference program: no run from an ifile has a non-zero
    receiver id.  So a round trip stands in: a reader that follows readBeast's framing and its 0xe3 case recovers (id, frame) for
    every frame of the checker's stream on hostile records with hostile ids (0, all bytes 0x1a, 0x1a in each position, 2^64 - 1) —
    except exactly behind the reference's quirk, asserted separately: a caller of a length the format does not carry writes nothing
    yet moves the writer's id, so the next frame of that id goes out without a prefix and the reader books it to the id before."""
    msgs = bu.hostile_records(40000, 300 + seed)
    ids = biu.random_ids(len(msgs), seed)
    verdict = bu.random_verdicts(len(msgs), 40 + seed) if gated else None
    shadowed, stream = _round_trip(msgs, verdict, ids, 0)
    assert shadowed >= 20
    # with the quirk's records taken out the round trip is exact for every frame
    carried = np.isin(msgs["msgbits"], (16, 56, 112))
    s2, _ = _round_trip(msgs[carried], None if verdict is None else verdict[carried], ids[carried], 0)
    assert s2 == 0


def test_prefix_bytes_and_fresh_writer():
    assert biu.prefix_bytes(0) == b"\x1a\xe3" + bytes(8)
    assert biu.prefix_bytes(0x1A1A1A1A1A1A1A1A) == b"\x1a\xe3" + b"\x1a" * 16
    assert len(biu.prefix_bytes(0x1A00000000000022)) == 11
    msgs = bu.hostile_records(2048, 9)
    zero = np.zeros(len(msgs), dtype=np.uint64)
    plain = bu.beast_reference(msgs)[0]
    assert biu.beast_reference(msgs, ids=zero)[0] == plain                                   # id 0 from a fresh writer: no prefix
    s, _, _, last, plen = biu.beast_reference(msgs, ids=zero, last_id=7)
    first = int(np.nonzero(bu.beast_reference(msgs)[1])[0][0])
    assert plen.sum() == 10 and last == 0 and len(s) == len(plain) + 10
    assert plen[first] == 10 or not np.isin(msgs["msgbits"][:first], (16, 56, 112)).all()


@pytest.mark.parametrize("cut", [1, 255, 256, 1000])
def test_cut_lists_give_the_bytes_of_one_call(cut):
    msgs = bu.hostile_records(2048, 77)
    ids = biu.ids_changing_every(len(msgs), 3, 1)
    v = bu.random_verdicts(len(msgs), 3)
    whole, _, _, final, _ = biu.beast_reference(msgs, v, ids=ids, last_id=5)
    out, last = bytearray(), 5
    for a in range(0, len(msgs), cut):
        s, _, _, last, _ = biu.beast_reference(msgs[a:a + cut], v[a:a + cut], ids=ids[a:a + cut], last_id=last)
        out += s
    assert bytes(out) == whole and last == final
