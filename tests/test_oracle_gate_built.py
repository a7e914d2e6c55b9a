"""CPU: the built lists of tests/gate_util.py through the restated gate (oracle/modes_oracle_gate.c) — the lists the device is
compared on in tests/test_gpu_gate_built.py say what they claim to say.  Every expectation here is written by hand from the
reference's lines (track.c:1933, 2835-2867, net_io.c:5846-5849, 5924-5940; gate_util.KINDS) and asserted on the restatement's
verdicts alone: threshold pairs at the limit and 1 ms beyond it, the same with the two messages at chosen lanes of the address's
run, the cut of the 256-message batch, the buffer a message is counted in, and what a list that mixes cases has to hold."""
import numpy as np
import pytest

import gate_util as gu

NAMES = list(gu.built_cases())


def verdicts(name):
    case = gu.built_case(name)
    return case, gu.oracle_gate_stepped(case.raw, case.cuts)


def check_expectations(case, v):
    assert case.expect
    for i, want, what in case.expect:
        assert (v[i] & 3) == want, f"{what}: verdict {v[i] & 3}, by hand {want} ({case.row(i)})"


@pytest.mark.parametrize("name", NAMES)
def test_every_built_list_goes_through_the_restatement(name):
    """... in the calls the device gets it in; what is written by hand for it holds; a list that mixes cases holds every verdict and
    every bit both ways."""
    case, v = verdicts(name)
    assert len(v) == len(case.msgs) == len(case.fields) > 0
    ts = case.msgs["timestamp"].astype(np.int64)
    assert (np.diff(ts) >= 0).all() and (np.diff(case.msgs["sysTimestamp"]) >= 0).all()
    assert np.array_equal(((ts - 772) // 5) // gu.BUF, case.raw["buffer"].astype(np.int64))      # the buffer as the device works it out
    phase = ts - 768 - ((ts - 772) // 5) * 5
    assert phase.min() >= 4 and phase.max() <= 8
    if case.expect:
        check_expectations(case, v)
    if case.mixed:
        assert not gu.coverage_gaps(v), gu.coverage_gaps(v)


@pytest.mark.parametrize("kind", list(gu.KINDS))
def test_threshold_pair(kind):
    """Two aircraft with the same history: the tested message at the limit and 1 ms beyond it get different verdicts, the ones
    written by hand — in one call, and with the referred message the last of one call and the tested one the first of the next."""
    limit, _, _, v_at, v_beyond, nonicao = gu.KINDS[kind]
    assert v_at != v_beyond
    for case in (gu.built_case("pairs"), gu.built_case(f"cut_{kind}")):
        v = gu.oracle_gate_stepped(case.raw, case.cuts)
        mine = [(i, want) for i, want, what in case.expect if what.startswith(kind + " lead")]
        assert len(mine) == 2
        (ia, wa), (ib, wb) = mine
        assert (v[ia] & 3, v[ib] & 3) == (v_at, v_beyond) == (wa, wb)
        r = case.raw
        assert r["addr"][ib] == r["addr"][ia] + 1 and r["now_ms"][ib] == r["now_ms"][ia] + 1
        assert bool(r["addr"][ia] >> 24) == bool(nonicao)
        # otherwise identical histories
        ha, hb = (np.nonzero(r["addr"] == r["addr"][i])[0][:-1] for i in (ia, ib))
        assert len(ha) == len(hb) and all(np.array_equal(r[k][ha], r[k][hb]) for k in ("msgtype", "iid", "cb", "cpr", "now_ms"))
    case = gu.built_case(f"cut_{kind}")
    ia = case.expect[0][0]
    assert ia in case.cuts, "the tested message begins a call"
    ref = case.cuts[0] - 1                                   # the last message of the first call: the pair's second referred message
    assert case.raw["now_ms"][ref] == case.raw["now_ms"][ia] - limit


@pytest.mark.parametrize("kind", list(gu.KINDS))
def test_lane_matrix(kind):
    """The pair with `lead` messages before the referred one and `between` between it and the tested one: the two share a step,
    straddle one step boundary or two, the tested message lands in lane 0, 1 and 63 — and the verdicts written by hand stay."""
    _, _, _, v_at, v_beyond, _ = gu.KINDS[kind]
    case, v = verdicts(f"lanes_{kind}")
    check_expectations(case, v)
    nkeep = len(gu.keepalives(kind))
    lanes, steps = set(), set()
    for (lead, between), (refs, tested) in case.note.items():
        between = max(between, nkeep)
        for ref, t, want in zip(refs, tested, (v_at, v_beyond)):
            run = np.nonzero(case.raw["addr"] == case.raw["addr"][t])[0]            # the address's messages, in order: its run
            k_ref, k_t = int(np.searchsorted(run, ref)), int(np.searchsorted(run, t))
            assert (k_ref, k_t) == (lead, lead + 1 + between) and k_t == len(run) - 1
            assert (v[t] & 3) == want
            lanes.add(k_t % 64)
            steps.add(k_t // 64 - k_ref // 64)
    assert {0, 1, 63} <= lanes and {0, 1, 2} <= steps


@pytest.mark.parametrize("n,ranks", gu.BATCH_CASES)
def test_batch_cut(n, ranks):
    """One address's only two messages inside one drainMessageBuffer batch of 256 get the same verdict; across the cut the first
    is judged on a->messages == 1."""
    case, v = verdicts(f"batch_{n}_{ranks[0]}")
    r = case.raw
    s = r["msgtype"] != 77
    assert int((s & (r["buffer"] == gu.BATCH_BUFFER)).sum()) == n
    pair = np.nonzero(r["addr"] == gu.BATCH_ADDR)[0]
    in_buffer = np.nonzero(r["buffer"] == gu.BATCH_BUFFER)[0]
    assert len(pair) == 2 and tuple(int(np.searchsorted(in_buffer, p)) for p in pair) == tuple(ranks)
    assert (r["msgtype"][in_buffer[n:]] == 77).all() and len(in_buffer) == n + 5         # Mode A/C replies behind the Mode S messages
    assert (v[~s] & 3 == 1).all()
    first, second = int(v[pair[0]] & 3), int(v[pair[1]] & 3)
    if ranks[0] // 256 == ranks[1] // 256:
        assert first == second == 1
    else:
        assert first in (0, 2) and second != first and second == 1
    check_expectations(case, v)


def test_buffers():
    """Positions k * 131072 - 1 (phase 8) and k * 131072 (phase 4) are two buffers, so two batches."""
    case, v = verdicts("buffers")
    check_expectations(case, v)
    ts = case.msgs["timestamp"].astype(np.int64)
    for k in gu.BUFFER_KS:
        assert (k * gu.BUF - 1) * 5 + 768 + 8 in ts and k * gu.BUF * 5 + 768 + 4 in ts


def run_events(raw):
    """Per message of a one-address list on a fresh table, from the reference's rules alone: is it dead (more than 5 minutes behind
    the last reliable non-position message), is it the first position message."""
    r = raw
    reliable = (r["msgtype"] == 17) | (r["msgtype"] == 18) | ((r["msgtype"] == 11) & (r["iid"] == 0))
    dead, first_pos, last, seen_pos = [], [], None, False
    for k in range(len(reliable)):
        now, pos = int(r["now_ms"][k]), bool(reliable[k] and r["cpr"][k])
        dead.append(last is None or now - last > 300000)
        first_pos.append(pos and not seen_pos)
        seen_pos |= pos
        if reliable[k] and not pos:
            last = now
    return np.array(dead), np.array(first_pos), reliable & (r["cpr"] == 1)


def test_runs_hold_what_the_walk_can_get_wrong():
    r = gu.built_case("runs_a").raw
    for v in gu.RUN_VARIANTS:
        rr = gu.built_case(f"runs_{v}").raw
        assert sorted(np.unique(rr["addr"], return_counts=True)[1][:-1]) == sorted(gu.RUN_LENGTHS)
    reliable = (r["msgtype"] == 17) | (r["msgtype"] == 18)
    assert (reliable & (r["cpr"] == 1)).any() and (reliable & (r["cpr"] == 0)).any()
    assert ((r["msgtype"] == 11) & (r["iid"] == 0)).any() and ((r["msgtype"] == 11) & (r["iid"] != 0)).any()
    assert (r["msgtype"] == 4).any() and (r["msgtype"] == 20).any() and set(np.unique(r["cb"])) == {0, 1, 2}
    seen = set()
    for v in gu.RUN_VARIANTS:
        for length in gu.RUN_LENGTHS:
            raw = gu.built_case(f"run_{length}_{v}").raw
            assert len(raw["msgtype"]) == length and len(np.unique(raw["addr"])) == 1
            dead, first_pos, pos = run_events(raw)
            k = np.arange(length)
            alive_before = np.concatenate([[False], ~dead[:-1]])                # (a fresh table's first message is dead anyway)
            for name, mask in (("dead in lane 0", dead & alive_before & (k % 64 == 0)), ("dead in lane 63", dead & alive_before & (k % 64 == 63)),
                               ("first position in lane 0", first_pos & (k % 64 == 0)), ("first position in lane 63", first_pos & (k % 64 == 63) & (k < length - 1)),
                               ("first position is the last message", first_pos & (k == length - 1) & (k > 0))):
                if mask.any():
                    seen.add(name)
            if length > 64 and dead[:64].any() and (dead & alive_before)[:64].any():
                seen.add("dead in the step before")
            if any(pos[s:s + 64].sum() >= 2 for s in range(0, length, 64)):
                seen.add("two positions in one step")
    assert seen == {"dead in lane 0", "dead in lane 63", "dead in the step before", "first position in lane 0", "first position in lane 63",
                    "first position is the last message", "two positions in one step"}
    for length in gu.RUN_LENGTHS:
        for prime in gu.PRIMES:
            case = gu.built_case(f"primed_{length}_{prime}")
            assert case.cuts == [2] and len(case.msgs) == length + 2 and len(np.unique(case.raw["addr"])) == 1


def test_addresses():
    want = {0x000000, 0x000001, 0x0000ff, 0x000100, 0xffffff, 0x1000000, 0x1000001, 0x1ffffff}
    for n in gu.SORT_SIZES + (gu.SORT_LARGE[0],):
        case = gu.built_case(f"addr_{n}")
        r = case.raw
        assert len(r["addr"]) == n
        if n >= 63:
            assert want <= set(int(a) for a in np.unique(r["addr"]))
            z = (r["addr"] == 0) & ((r["msgtype"] == 4) | (r["msgtype"] == 20)) & (r["cb"] == 0)
            if n >= 8191:
                assert z.any() and (gu.oracle_gate_stepped(r)[z] & 3 == 1).all()    # Address/Parity with address 0: crc == 0, forwarded
    r = gu.built_case(f"addr_{gu.SORT_LARGE[0]}").raw
    assert len(np.unique(r["addr"])) == gu.SORT_LARGE[1]
    a = np.array(gu.ADDRESSES)
    x = a[:, None] ^ a[None, :]
    for digit in range(4):                                                        # pairs that differ in one sort digit only
        m = 0xff << (8 * digit)
        assert ((x != 0) & ((x & ~m) == 0)).any()


def test_call_cuts():
    """One call, two calls, buffer by buffer: the restatement says the same."""
    case = gu.built_case("callcut")
    r = case.raw
    assert 35000 <= len(r["addr"]) <= 45000 and len(np.unique(r["addr"])) == 30 and (r["addr"] >> 24).any()
    assert r["now_ms"][-1] - r["now_ms"][0] > 2.9 * 3600 * 1000
    assert len(case.note["each"]) > 2000
    one = gu.oracle_gate_stepped(r)
    assert np.array_equal(one, gu.oracle_gate_stepped(r, case.note["two"]))
    assert np.array_equal(one, gu.oracle_gate_stepped(r, case.note["each"]))
    # the rules that only hours bring: a known aircraft's deferred messages far behind its first two
    late = r["now_ms"] > r["now_ms"][0] + 3600 * 1000
    assert ((one[late] & 3) == 2).any() and ((one[late] & 3) == 1).any() and ((one[late] & 3) == 0).any()


def test_host_form_frames_decode_to_the_rows():
    """The sealed frames of the host-form list carry the rows' address, IID and position flag (the CPU field decode)."""
    import fields_util as fu
    case = gu.built_case("host")
    frames = gu.frames_of(case)
    r = case.raw
    f = fu.oracle_fields(frames, np.where(r["msgtype"] >= 16, 112, 56).astype(np.int32))
    assert np.array_equal(f["addr"], r["addr"]) and np.array_equal(f["IID"], r["iid"])
    assert np.array_equal((f["flags"] & gu.F_CPR_VALID) != 0, r["cpr"] != 0)
    assert (r["iid"] == 5).any() and ((r["msgtype"] == 11) & (r["iid"] == 0)).any()
