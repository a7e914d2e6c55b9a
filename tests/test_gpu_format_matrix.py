"""-m gpu: every input format (UC8, SC16, SC16Q11) at the edges, against the reference's own objects (helpers.reference_run), exact:
every message and every counter, the noise power of the SC16 formats (the reference's sequential float sums) included.

The SC16 formats run through kernels of their own (k_sweep_sc16<15> / <11>: converter and sweep in one pass), which stage a chunk's
first step, the carried 326-magnitude tail, the last one or two steps and the unswept steps behind the last scan position sample by
sample (sweep_stage_careful).  The cases below are the places where that staging changes: lengths around one sweep step (1024
positions), around one buffer (131072 samples) and ragged ends; feeds cut into chunks, so that a chunk starts from a carried tail;
the option grid; the ends of the threshold range on clipped samples; and, with Mode A/C on, the unfused path (k_convert_* + k_sweep).
Where a capture is not empty and Mode A/C is off the case also asserts that the fused kernel ran.

One Demodulator per (format, options), shared by the module's cases and reset() between them."""
import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu

B = 131072
FMTS = (0, 1, 2)
MAX_SAMPLES = 8 * B


@pytest.fixture(scope="module")
def contexts(built):
    import readsb_amd
    cache = {}

    def get(fmt, nfix=1, fixdf=1, thr=58, mode_ac=0):
        key = (fmt, nfix, fixdf, thr, mode_ac)
        if key not in cache:
            cache[key] = readsb_amd.Demodulator(fmt=fmt, nfix_crc=nfix, fix_df=fixdf, preamble_threshold=thr, mode_ac=mode_ac,
                                                startup_time_ms=helpers.STARTUP_MS, max_samples=MAX_SAMPLES)
        cache[key].reset()
        return cache[key]

    yield get
    for d in cache.values():
        d.close()


def _demod(d, iq, fmt, chunk_samples=MAX_SAMPLES):
    """Feed in chunks of whole buffers, finish, collect -> (messages, counters, chunks the fused sweep kernel ran on: the timing block
    covers one feed, so it is read after every one)."""
    iq = np.ascontiguousarray(iq).view(np.uint8).reshape(-1)
    bps = helpers.FMT_BYTES[fmt]
    n = iq.size // bps
    assert chunk_samples % B == 0
    fused = 0.0
    for off in range(0, n, chunk_samples):
        d.feed_iq(iq[off * bps: min(off + chunk_samples, n) * bps])
        fused += d.timing()["sweep_fused_chunks"]
    d.finish()
    msgs, cnt = d.collect()
    return msgs, cnt, fused


def _check(contexts, iq, fmt, nfix=1, fixdf=1, thr=58, mode_ac=0, chunk_samples=MAX_SAMPLES):
    want, wst = helpers.reference_run(iq, fmt, nfix, fixdf, thr, mode_ac=mode_ac)
    got, cnt, fused = _demod(contexts(fmt, nfix, fixdf, thr, mode_ac), iq, fmt, chunk_samples)
    helpers.assert_same_messages(got, want)
    helpers.assert_same_counters(cnt, wst, float_tol=0.0)
    if mode_ac:
        assert fused == 0, "Mode A/C takes the converter and k_sweep, not the fused kernel"
        assert int(cnt["demod_modeac"]) == int(wst["demod_modeac"])
    elif len(iq):
        assert fused >= 1, "the capture did not go through the fused sweep kernel"
    return want, wst


LENGTHS = [0, 1, 100, 325, 326, 327, 1023, 1024, 1025, 4095, 4096, B - 1, B, B + 1, 2 * B, 300000, 3 * B + 698]


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("nsamples", LENGTHS)
def test_lengths(contexts, fmt, nsamples):
    """Empty, shorter than the 326-sample overlap, around one sweep step (1024 positions), around one buffer (at exactly one buffer
    the reference appends a zero-length buffer and noise_power_sum is NaN on both sides), several buffers with a ragged end."""
    iq = helpers.synth(nsamples=nsamples, seed=3, rate=4000.0, fmt=fmt)
    want, _ = _check(contexts, iq, fmt)
    if nsamples >= B - 1:
        assert len(want) > 20                                 # (4000 transmissions a second: some 200 in a buffer, a quarter of them decoded)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("dense", [0, 4])
def test_noise_only(contexts, fmt, dense):
    """No transmitter at all: uniform noise, and Gaussian noise (dense bit 2)."""
    iq = helpers.synth(seconds=1.0, seed=9, rate=0.0, dense=dense, fmt=fmt)
    _check(contexts, iq, fmt)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("chunk_buffers", [3, 1])
def test_chunked_feeds(contexts, fmt, chunk_buffers):
    """4 s fed three buffers, and one buffer, per call: every chunk but the first starts from the 326 magnitudes carried over from the
    chunk before (the only way sweep_stage_careful sees a tail that is not zeros) and from the filter state so far."""
    iq = helpers.synth(seconds=4.0, seed=5, fmt=fmt)
    want, _ = _check(contexts, iq, fmt, chunk_samples=chunk_buffers * B)
    assert len(want) > 1000


@pytest.mark.parametrize("fmt", (1, 2))
@pytest.mark.parametrize("nfix,fixdf,thr", [(1, 1, 58), (2, 1, 58), (0, 1, 58), (1, 0, 58), (1, 1, 75), (2, 1, 40)])
def test_options(contexts, fmt, nfix, fixdf, thr):
    """test_gpu_parity.py::test_uc8_options' grid on the SC16 formats."""
    iq = helpers.synth(seconds=3.0, seed=101, fmt=fmt)
    want, _ = _check(contexts, iq, fmt, nfix, fixdf, thr)
    assert len(want) > 1000


def _clipped(fmt):
    """A capture whose strong frames saturate.  UC8: test_gpu_parity.py's.  SC16 / SC16Q11: the 16-bit samples times 2.0 (chosen on
    the CPU: the reference then finds 7 % of the magnitudes at 65535 and 2186 .. 2372 messages over the threshold range), clipped
    to full scale +-32767 for SC16, to +-2600 for SC16Q11, whose nominal range ends at +-2047: values at and beyond it, magnitude
    clamped to 65535."""
    iq = helpers.synth(seconds=2.0, seed=2024, rate=3000.0, fmt=fmt)
    if fmt == 0:
        return np.clip((iq.astype(np.float32) - 127.5) * 2.6 + 127.5, 0, 255).round().astype(np.uint8)
    lim = 32767 if fmt == 1 else 2600
    hot = np.clip(np.rint(iq.view("<i2").astype(np.float32) * 2.0), -lim, lim).astype("<i2")
    assert (np.abs(hot) == lim).mean() > 0.01 and (fmt == 1 or (np.abs(hot) > 2047).mean() > 0.01)
    return hot.view(np.uint8)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("thr", [40, 58, 400])
def test_threshold_range_ends_on_a_clipped_capture(contexts, fmt, thr):
    """The reference's whole --preamble-threshold range on saturating samples: runs of magnitude 65535 through the sweep's and the
    slicer's biased 16-bit arithmetic, in every format's own converter."""
    hot = _clipped(fmt)
    mag = helpers.oracle_convert(hot[: helpers.FMT_BYTES[fmt] * 400000], fmt)[0]
    want, _ = _check(contexts, hot, fmt, 1, 1, thr)
    assert (mag == 65535).mean() > 0.002 and len(want) > 200


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("nsamples", [1025, B + 1])
def test_unfused_path_with_mode_ac(contexts, fmt, nsamples):
    """Mode A/C on: k_convert_* + k_sweep (the Mode A/C scan wants the magnitudes and the sums before the sweep), per format, one step
    plus one position and one buffer plus one sample."""
    iq = helpers.synth(nsamples=nsamples, seed=404 + fmt, rate=1500.0, dense=2, fmt=fmt)
    _check(contexts, iq, fmt, mode_ac=1)
