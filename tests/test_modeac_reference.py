"""CPU tests: the restatement's Mode A/C demodulator (oracle/modes_oracle.c: demod_buffer_ac) against the reference's own objects
(oracle/_ref) on BUILT replies (tests/modeac_util.py), where tests/test_oracle.py has drawn captures: the tile- and buffer-edge
positions, pairs across a buffer edge, a spread of codes and the densest packing, in every input format.  This is what entitles
tests/test_gpu_modeac_built.py to take the restatement's word, one struct mag_buf at a time, at the edges of the scan.

And the premises of the case sets themselves, on the checker's output alone: that the replies built as clean are mostly accepted,
that every tie group changes the verdict, that 69 and 70 samples apart differ, that the phase grid moves the clock estimate, that
every code is seen, that the full-queue pattern passes the cheap tests at exactly half of every tile's positions."""
import numpy as np
import pytest

import helpers
import modeac_util as mu

needs_ref = pytest.mark.skipif(not helpers.have_ref(), reason="oracle/_ref not built (the reference's sources are not here)")


def _same(a, sa, b, sb):
    assert len(a) == len(b), f"{len(a)} messages against the reference's {len(b)}"
    assert a.tobytes() == b.tobytes()
    assert int(sa["demod_modeac"]) == int(sb["demod_modeac"]) == int((b["msgtype"] == 77).sum())
    for f in helpers.COUNTER_FIELDS:
        assert np.array_equal(np.asarray(sa[f]), np.asarray(sb[f])), f


@needs_ref
@pytest.mark.parametrize("fmt", (0, 1, 2))
@pytest.mark.parametrize("variant", mu.IQ_VARIANTS)
def test_restatement_equals_reference_on_built_captures(built, variant, fmt):
    iq, nbuilt = mu.iq_capture(variant, fmt)
    a, sa = helpers.oracle_run(iq, fmt, 1, 1, 58, mode_ac=1)
    b, sb = helpers.ref_run(iq, fmt, 1, 1, 58, mode_ac=1)
    _same(a, sa, b, sb)
    mu.check_iq_conditions(variant, b, nbuilt)


@needs_ref
def test_restatement_equals_reference_on_the_capacity_capture(built):
    iq = mu.capacity_capture()
    a, sa = helpers.oracle_run(iq, 0, 1, 1, 58, mode_ac=1)
    b, sb = helpers.ref_run(iq, 0, 1, 1, 58, mode_ac=1)
    _same(a, sa, b, sb)
    mu.check_capacity_conditions(b)


@pytest.mark.parametrize("variant", mu.IQ_VARIANTS)
def test_iq_captures_are_worth_running(built, variant):
    """The same premises on the restatement alone, so that they are checked where the reference's objects are missing too."""
    iq, nbuilt = mu.iq_capture(variant, 0)
    mu.check_iq_conditions(variant, helpers.oracle_run(iq, 0, 1, 1, 58, mode_ac=1)[0], nbuilt)


@pytest.mark.parametrize("name", sorted(mu.MAG_SETS))
def test_magnitude_sets_are_worth_running(built, name):
    mu.check_mag_conditions(name)


def test_builder_against_a_hand_computed_reply():
    """reply(): slot k on for cycles [start + 87 k, start + 87 k + 27), a sample = 25 cycles, value = amplitude * overlap / 25."""
    m = np.zeros(80, dtype=np.uint16)
    mu.reply(m, 25 * 2 + 10, 0x80020, 25000)
    want = np.zeros(80, dtype=np.uint16)
    want[2], want[3] = 15000, 12000                       # F1: cycles 60 .. 87 = 15 of sample 2, 12 of sample 3
    want[51], want[52] = 22000, 5000                      # F2: cycles 1278 .. 1305 = 22 of sample 51, 5 of sample 52
    assert np.array_equal(m, want)
    m[:] = 0
    mu.reply(m, 24, 0x80000, 25000)                       # three samples: 1, 25 and 1 cycles
    assert m[:4].tolist() == [1000, 25000, 1000, 0]
    assert int(mu.bits20_of(0)) == 0x80020 and int(mu.bits20_of(0x7777 | 0x80)) == 0xFEFE4
    assert mu.noise_level(0.0, mu.power_for_noise(3000)) == 3000 and mu.power_for_noise(0) == 0.0
