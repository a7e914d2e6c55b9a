"""The filter scripts of tests/filter_util.py on the CPU: the restatement (helpers.oracle_stream) equals the reference's own objects
(oracle/_ref/ref_demod, driven by the same script) feed by feed, message for message and counter for counter; and every scenario
separates what it claims — on the REFERENCE's output alone, so that tests/test_gpu_filter_clock.py cannot pass on a capture where
the filter never mattered.  The counts below were recorded from oracle/_ref."""
import numpy as np
import pytest

import filter_util as fu
import helpers

needs_ref = pytest.mark.skipif(not helpers.ref_takes_scripts(), reason="oracle/_ref not built (needs the reference tree)")

COUNTS = fu.RECORDED                               # per-feed message counts, recorded from oracle/_ref
BEFORE_FIRST_UNKNOWN = fu.RECORDED_UNKNOWN


def _same(got, want, what):
    assert len(got) == len(want)
    for k, ((gm, gs), (wm, ws)) in enumerate(zip(got, want)):
        assert len(gm) == len(wm), f"{what}, feed {k}: {len(gm)} messages, the reference has {len(wm)}"
        assert gm.tobytes() == wm.tobytes(), f"{what}, feed {k}: messages differ"
        for f in helpers.COUNTER_FIELDS + ["demod_modeac"]:
            assert (np.asarray(gs[f]) == np.asarray(ws[f])).all(), f"{what}, feed {k}: counter {f}: {gs[f]} != {ws[f]}"
        for f in ("signal_power_sum", "noise_power_sum", "peak_signal_power"):
            assert float(gs[f]) == float(ws[f]), f"{what}, feed {k}: {f}: {gs[f]!r} != {ws[f]!r}"


def _restated(s, ops, **kw):
    return helpers.oracle_stream(ops, filter_clock=s.clock, **kw)


def _ref(s, ops, **kw):
    return helpers.ref_run(None, ops=ops, filter_clock=s.clock, **kw)


@needs_ref
@pytest.mark.parametrize("name", fu.ALL)
def test_restatement_equals_reference_on_every_script(built, name):
    s = fu.scenario(name)
    _same(_restated(s, s.ops), _ref(s, s.ops), name)
    for which, ops in s.without.items():
        _same(_restated(s, ops), _ref(s, ops), f"{name} / {which}")


@needs_ref
@pytest.mark.parametrize("name,fmt,nfix,mode_ac", [("foreign_add", 1, 1, 0), ("grow", 2, 1, 0), ("foreign_add", 0, 2, 0), ("grow", 0, 2, 0),
                                                    ("foreign_add", 0, 1, 1), ("grow", 0, 1, 1), ("fuzz1", 2, 2, 1)])
def test_restatement_equals_reference_in_the_other_configurations(built, name, fmt, nfix, mode_ac):
    s = fu.scenario(name)
    ops = fu.in_format(s.ops, fmt)
    kw = dict(fmt=fmt, nfix=nfix, mode_ac=mode_ac)
    _same(_restated(s, ops, **kw), _ref(s, ops, **kw), name)


def _checker(s, ops):
    """The reference where it is built; the restatement (pinned to it above) otherwise."""
    return helpers.reference_run(None, ops=ops, filter_clock=s.clock)


@pytest.mark.parametrize("name", fu.TABLE)
def test_every_scenario_separates_what_it_claims(built, name):
    s = fu.scenario(name)
    own, without = COUNTS[name]
    got = _checker(s, s.ops)
    assert fu.counts(got) == own
    assert set(without) == set(s.without)
    for which, want in without.items():
        assert want != own                                          # (a condition on the inputs)
        assert fu.counts(_checker(s, s.without[which])) == want, which
    if name in BEFORE_FIRST_UNKNOWN:
        assert int(got[-1][1]["demod_rejected_unknown_icao"]) == BEFORE_FIRST_UNKNOWN[name]


def test_before_first_separates_the_two_clocks():
    assert COUNTS["before_first_clock0"][0] != COUNTS["before_first_clock1"][0]
    assert BEFORE_FIRST_UNKNOWN["before_first_clock0"] != BEFORE_FIRST_UNKNOWN["before_first_clock1"]


def test_the_share_of_scenarios_that_fail_to_separate_is_zero(built):
    failed = []
    for name in fu.TABLE:
        s = fu.scenario(name)
        own = fu.counts(_checker(s, s.ops))
        if name.startswith("before_first"):
            other = fu.scenario("before_first_clock1" if name.endswith("0") else "before_first_clock0")
            others = [fu.counts(_checker(other, other.ops))]
        else:
            others = [fu.counts(_checker(s, ops)) for ops in s.without.values()]
        if not others or any(o == own for o in others):
            failed.append(name)
    assert not failed, failed


def test_foreign_add_at_the_boundary(built):
    """foreign_add_late: FOREIGN's frames are rejected in every feed before the add and accepted from the first feed behind it."""
    s = fu.scenario("foreign_add_late")
    nadd = [k for k, op in enumerate(s.ops) if op == ("add", fu.FOREIGN)]
    assert len(nadd) == 1
    feeds_before = sum(1 for op in s.ops[:nadd[0]] if op[0] == "feed")
    per_feed = [int(np.sum(m["addr"] == fu.FOREIGN)) for m, _ in _checker(s, s.ops)]
    assert feeds_before == 3 and per_feed == [0, 0, 0, 6, 6]
    assert [int(np.sum(m["addr"] == fu.FOREIGN)) for m, _ in _checker(s, s.without["no_add"])] == [0] * 5


def test_generations_what_does_not_add_again(built):
    """The repaired DF11 and the DF11 with IID 5 are accepted (their addresses are still known) and do not add: after the next expire
    only the address heard again as DF17 is left."""
    s = fu.scenario("generations")
    got = _checker(s, s.ops)
    m1 = got[1][0]
    rep = m1[(m1["addr"] == fu.GEN[2]) & (m1["msgtype"] == 11)]
    assert len(rep) == 1 and rep["correctedbits"][0] == 1
    iid = m1[(m1["addr"] == fu.GEN[3]) & (m1["msgtype"] == 11)]
    assert len(iid) == 1 and iid["correctedbits"][0] == 0
    assert set(got[2][0]["addr"].tolist()) == {int(fu.GEN[1])}
    assert len(got[3][0]) == 0


@pytest.mark.parametrize("seed", fu.FUZZ_SEEDS)
def test_fuzz_scripts_exercise_the_filter(built, seed):
    """Conditions on the fuzz inputs: frames are accepted and rejected for their address in most feeds, addresses the host alone added
    are accepted, and the table grows (more than 85 inserts between two expiries)."""
    s = fu.scenario(f"fuzz{seed}")
    assert s.nbuffers == 8 and s.clock == fu.FUZZ_CLOCK[seed]
    got = _checker(s, s.ops)
    unknown = np.diff([0] + [int(st["demod_rejected_unknown_icao"]) for _, st in got])
    assert (unknown > 0).sum() >= len(got) - 1 and sum(fu.counts(got)) > 500
    kinds = [op[0] for op in s.ops]
    assert kinds.count("add") >= 3 and (s.clock != 2 or kinds.count("expire") >= 2)
    assert kinds.count("feed") >= 4 and max(len(op[1]) for op in s.spec if op[0] == "feed") >= 2
    # addresses accepted in Address/Parity frames that no DF11 / DF17 of the whole capture carries: known through the host's add alone
    msgs = np.concatenate([m for m, _ in got])
    spoken = set(msgs["addr"][np.isin(msgs["msgtype"], [11, 17])].tolist())
    foreign = set(msgs["addr"][~np.isin(msgs["msgtype"], [11, 17])].tolist()) - spoken
    added = {int(op[1]) for op in s.ops if op[0] == "add"}
    assert foreign and foreign <= added
