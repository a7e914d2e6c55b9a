"""-m gpu: Mode A/C (k_modeac, and the skip and merge in build_job) on BUILT replies, exact.  tests/test_gpu_modeac.py runs drawn
captures, where a reply's position is random; tests/modeac_util.py puts replies where the scan has its edges:

  the tile and its look-ahead (a workgroup stages 2048 positions plus 80 samples; F2 and the last slots of a reply whose F1 is among a
  tile's last 70 positions come from the look-ahead), position 0 of a buffer (never scanned), the last positions (F2 and the bits in
  the trailing samples) of full and short buffers, two replies 60 .. 80 samples apart (an accepted reply hides the next 69 positions of
  its own buffer) in one tile, in two, in two buffers, trains of eight, every comparison of the loop body at equality, the float
  clock estimate over a grid of first-pulse values at small and large positions, every code, and the candidate queue of a tile
  exactly full.

Magnitude level (mgpu_demod_mag_buf_ac, one struct mag_buf per call) against the restatement, which tests/test_modeac_reference.py
pins to the reference's objects on built captures; IQ level (every format, whole and buffer by buffer) against the reference's objects
themselves (helpers.reference_run); and the capacity of the candidate lists: exact, or MGPU_E_OVERFLOW, never a short list."""
import numpy as np
import pytest

import helpers
import modeac_util as mu

pytestmark = pytest.mark.gpu

B = mu.B


@pytest.fixture(scope="module")
def one_buffer(built):
    """The context of all magnitude-level cases: chunks of one buffer."""
    import readsb_amd
    d = readsb_amd.Demodulator(mode_ac=1, startup_time_ms=helpers.STARTUP_MS, max_samples=B)
    yield d
    d.close()


@pytest.fixture(scope="module")
def contexts(built):
    import readsb_amd
    cache = {}

    def get(fmt):
        if fmt not in cache:
            cache[fmt] = readsb_amd.Demodulator(fmt=fmt, mode_ac=1, startup_time_ms=helpers.STARTUP_MS, max_samples=4 * B)
        cache[fmt].reset()
        return cache[fmt]

    yield get
    for d in cache.values():
        d.close()


def _check_mag(d, name):
    mu.check_mag_conditions(name)
    _tags, per_buffer, stats, _rel = mu.mag_expected(name)
    want = np.concatenate(per_buffer)
    got, cnt = mu.mag_run(d, mu.MAG_SETS[name]())              # (an overflow of a tile's candidate queue or of a list is an MgpuError here)
    helpers.assert_same_messages(got, want)
    helpers.assert_same_counters(cnt, stats)
    assert int(cnt["demod_modeac"]) == int(stats["demod_modeac"]) == int((want["msgtype"] == 77).sum())


def test_tile_edges(one_buffer):
    """F1 at 2048 k - j for j = -2 .. 70 and all 25 phases: the look-ahead behind a tile, sample by sample."""
    _check_mag(one_buffer, "tile")


def test_buffer_edges(one_buffer):
    """F1 at 0 (never found), 1, 2, 3, at length - 70 .. length - 60, length - 2, length - 1 and at length (the next buffer's), for
    buffers of 131072, 1, 2, 70, 327, 2047 and 2049 samples."""
    _check_mag(one_buffer, "edge")


def test_skip_over_an_accepted_reply(one_buffer):
    """Pairs 60 .. 80 apart in a tile, across a tile edge (two workgroups, two lists, sorted on the host) and across a buffer edge (two
    calls: nothing is hidden there); trains of eight 69, 70 and 71 apart."""
    _check_mag(one_buffer, "skip")


def test_comparisons_at_equality(one_buffer):
    """Each comparison of the loop body with its sample at T - 1, T and T + 1: the edge tests of F1 and F2, the two 6 dB tests, an on
    slot at signal_threshold, an off slot's pair at noise_threshold, a quiet third sample at signal_threshold."""
    _check_mag(one_buffer, "tie")


@pytest.mark.parametrize("f1", mu.GRID_F1)
def test_float_clock_estimate(one_buffer, f1):
    """25 * (f1 + fraction^2) + 0.5 in float over a 64 x 64 grid of the first pulse's two samples, at f1 = 5 and where a float's steps
    are 2^-7 (f1 >= 65536) and the product's 1/8 (f1 = 70001) and 1/4 (f1 = 130900)."""
    _check_mag(one_buffer, f"grid{f1}")


def test_all_codes(one_buffer):
    """All 4096 codes, SPI off and on, through the bit-to-code mapping."""
    _check_mag(one_buffer, "codes")


def test_candidate_queue_exactly_full(one_buffer):
    """1024 of every tile's 2048 positions pass the cheap F1 tests (the most there can be): the queue is full and not over; a genuine
    reply inside such a tile and one across the edge of two are found."""
    _check_mag(one_buffer, "queue")


def _demod(d, iq, fmt, chunk_samples):
    d.reset()
    return d.demodulate_capture(iq, chunk_samples=chunk_samples)


@pytest.mark.parametrize("fmt", (0, 1, 2))
@pytest.mark.parametrize("variant", mu.IQ_VARIANTS)
def test_built_capture(contexts, variant, fmt):
    """Three buffers and a short tail on the IQ entry: replies at delayed positions B - 2 .. B + 2 and 3 B - 2 .. 3 B + 2 (one per
    variant), a pair across 2 B, the tile-edge sweep at five phases, 512 codes; whole (one chunk of four buffers: a list serves three
    tiles) and one buffer per feed."""
    iq, built_replies = mu.iq_capture(variant, fmt)
    want, wst = helpers.reference_run(iq, fmt, 1, 1, 58, mode_ac=1)
    mu.check_iq_conditions(variant, want, built_replies)
    for chunk_samples in (4 * B, B):
        got, cnt = _demod(contexts(fmt), iq, fmt, chunk_samples)
        helpers.assert_same_messages(got, want)
        helpers.assert_same_counters(cnt, wst)
        assert int(cnt["demod_modeac"]) == int(wst["demod_modeac"])


def test_list_capacity(built, one_buffer):
    """Replies 70 samples apart over 64 buffers.  As one chunk: exact, or MGPU_E_OVERFLOW (a list has room for 1536 candidates and
    serves 64 tiles of some 29) -- and the context, reset, is exact again on a small capture.  Buffer by buffer in a context of one
    buffer: exact (a list serves one tile)."""
    import readsb_amd
    iq = mu.capacity_capture()
    want, wst = helpers.reference_run(iq, 0, 1, 1, 58, mode_ac=1)
    mu.check_capacity_conditions(want)
    small, _ = mu.iq_capture(0, 0)
    small_want, small_wst = helpers.reference_run(small, 0, 1, 1, 58, mode_ac=1)
    d = readsb_amd.Demodulator(mode_ac=1, startup_time_ms=helpers.STARTUP_MS, max_samples=64 * B, chunk_buffers=64)
    try:
        try:
            got, cnt = d.demodulate_capture(iq)
        except readsb_amd.MgpuError as e:
            print(f"one chunk of 64 buffers, {int(wst['demod_modeac'])} replies in the reference: {e}")
            assert "overflow" in str(e).lower() and "Mode A/C" in str(e), e
        else:
            print(f"one chunk of 64 buffers, {int(wst['demod_modeac'])} replies in the reference: {len(got)} messages, no overflow")
            helpers.assert_same_messages(got, want)
            helpers.assert_same_counters(cnt, wst)
        d.reset()
        got, cnt = d.demodulate_capture(small)
        helpers.assert_same_messages(got, small_want)
        helpers.assert_same_counters(cnt, small_wst)
    finally:
        d.close()
    got, cnt = _demod(one_buffer, iq, 0, B)
    helpers.assert_same_messages(got, want)
    helpers.assert_same_counters(cnt, wst)
    assert int(cnt["demod_modeac"]) == int(wst["demod_modeac"])
