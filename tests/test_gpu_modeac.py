"""-m gpu: Mode A/C replies (demodulate2400AC, demod_2400.c:575-761) beside Mode S, in netUseMessage order
(per buffer: the Mode S messages, then the replies), against the CPU oracle; every input format (the reply threshold
depends on the converter's exact per-buffer sums: integer for UC8, the reference's sequential float sums for SC16 / SC16Q11)."""
import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu


def _run(iq, **kw):
    import readsb_amd
    d = readsb_amd.Demodulator(startup_time_ms=helpers.STARTUP_MS, max_samples=max(len(iq) // 2, 131072), mode_ac=1, **kw)
    try:
        return d.demodulate_capture(iq)
    finally:
        d.close()


@pytest.mark.parametrize("seconds,rate,seed,nfix", [(3.0, 800.0, 404, 1), (2.0, 300.0, 405, 2), (60.0, 700.0, 406, 1)])
def test_mode_ac_beside_mode_s(built, seconds, rate, seed, nfix):
    iq = helpers.synth(seconds=seconds, seed=seed, rate=rate, dense=2, threads=16)
    want, wst = helpers.reference_run(iq, 0, nfix, 1, 58, mode_ac=1)
    got, cnt = _run(iq, nfix_crc=nfix)
    nac = int((want["msgtype"] == 77).sum())
    assert nac > 200 and (want["msgtype"] != 77).sum() > 200
    helpers.assert_same_messages(got, want)
    helpers.assert_same_counters(cnt, wst)
    assert int(cnt["demod_modeac"]) == nac == int(wst["demod_modeac"])


def test_mode_ac_off_is_the_default(built):
    import readsb_amd
    iq = helpers.synth(seconds=2.0, seed=404, rate=800.0, dense=2)
    want, wst = helpers.reference_run(iq)                      # no Mode A/C
    d = readsb_amd.Demodulator(startup_time_ms=helpers.STARTUP_MS, max_samples=len(iq) // 2)
    got, cnt = d.demodulate_capture(iq)
    d.close()
    helpers.assert_same_messages(got, want)
    assert int(cnt["demod_modeac"]) == 0


def test_mag_buf_entry_with_mode_ac(built):
    """demodulate2400(buf) + demodulate2400AC(buf) on host-provided struct mag_buf contents (readsb.c:871-874): the caller
    hands over mean_level and mean_power, the Mode A/C noise floor comes from them (demod_2400.c:579-580)."""
    import numpy as np
    import readsb_amd
    B, TR = 131072, 326
    iq = helpers.synth(nsamples=6 * B + 50000, seed=97, rate=700.0, dense=2)
    want, wst, mag = helpers.reference_run(iq, 0, 1, 1, 58, want_mag=True, mode_ac=1)
    assert (want["msgbits"] == 16).sum() > 20
    n = iq.size // 2
    d = readsb_amd.Demodulator(mode_ac=1, startup_time_ms=helpers.STARTUP_MS, max_samples=B)
    try:
        with pytest.raises(readsb_amd.MgpuError):          # without mean_level the Mode A/C half cannot run: refused, not skipped
            d.demod_mag_buf(mag[: TR + B], B, 0, helpers.STARTUP_MS, 0.01)
        k = 0
        while True:
            length = min(B, n - k * B)
            data = mag[k * B: k * B + TR + length]
            new = data[TR:].astype(np.uint64)
            mean_level = float(new.sum()) / 65536.0 / length                        # convert_uc8_nodc, convert.c:101-107
            mean_power = float((new * new).sum()) / 65535.0 / 65535.0 / length
            st = k * B * 5
            d.demod_mag_buf_ac(data, length, st, st // 12000 + helpers.STARTUP_MS, mean_level, mean_power)
            k += 1
            if length < B:
                break
        got, cnt = d.collect()
    finally:
        d.close()
    helpers.assert_same_messages(got, want)
    helpers.assert_same_counters(cnt, wst)


@pytest.mark.parametrize("fmt,seconds,rate,seed", [(2, 3.0, 800.0, 414), (1, 2.0, 500.0, 415)])
def test_mode_ac_on_the_sc16_formats(built, fmt, seconds, rate, seed):
    """Mode A/C on the IQ entry with SC16Q11 / SC16 input: the reply threshold comes from the buffer's mean level and power, which
    the reference's converters accumulate as sequential FLOAT sums (convert.c:225-249, 342-366) — reproduced bit for bit
    (k_fsum_sc16), so the replies and every counter, the noise power sums included, equal the reference's."""
    iq = helpers.synth(seconds=seconds, seed=seed, rate=rate, dense=2, fmt=fmt, threads=16)
    want, wst = helpers.reference_run(iq, fmt, 1, 1, 58, mode_ac=1)
    got, cnt = _run(iq, fmt=fmt)
    nac = int((want["msgtype"] == 77).sum())
    assert nac > 100 and (want["msgtype"] != 77).sum() > 100
    helpers.assert_same_messages(got, want)
    helpers.assert_same_counters(cnt, wst)
    assert int(cnt["demod_modeac"]) == nac == int(wst["demod_modeac"])
