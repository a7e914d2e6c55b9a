"""-m gpu: the CRC stage of k_slice (classify_frame / lane_diagnose, kernels/slicer.inc) on a capture that is exhaustive where the input
space is small enough to be, against the reference's own objects (helpers.reference_run), exact: every message (msg, raw,
correctedbits, addr, score, timestamp, signal level) and every counter.

The capture (tests/frames_util.py: repair_matrix) is built from the reference's table dump (tests/golden/tables.npz), not drawn: isolated,
noise-free frames 360 samples apart, each at a chosen one of the five sub-sample alignments, in this order —
  primers      one clean DF17 and one clean DF11 (IID 0) per true address, so that every corrected address is in the ICAO filter;
  long table   for EVERY entry of the 112-bit table (107 one-bit; at nfix 2 3831 in all) one DF17 — every 8th DF18 — with exactly those
               bits flipped, at each of the five alignments, address and ME content rotating (AA repairs meet 0 and 1 bits); and a
               sample of the entries on an address the filter does not hold (inside AA: refused; outside: accepted as unknown);
  short table  every one-bit entry in a DF11 at each alignment, with IID 0, 1, 64 and 127; DF11 with two flipped bits (dropped);
  outside      300 DF17 with three flipped bits; one flip inside the DF field, bits 0..4 (fixDF17msgtype's case, run with fix_df 1 and 0),
               known and unknown address, alone and with a second flip; Address/Parity frames with one flip (another address);
               at nfix 1 a sample of --aggressive's two-bit entries, which must miss;
  grid         clean, known and unknown address, every alignment: every DF value 0..31 sealed as Address/Parity at its own length, as
               if short, as if long, and with parity = CRC; DF11 IID 0 / 5; DF17; DF18; a DF11 whose only error lies inside the IID
               bits; the all-zero 56- and 112-bit frames.
About 22 000 frames, 3.3 s of stream at nfix 2; 3 500 frames at nfix 1 (nfix 0, which has no table, takes nfix 1's capture).

What keeps this from passing vacuously is the coverage condition (frames_util.check_coverage), computed from the REFERENCE's list
only and asserted on the CPU as well (tests/test_oracle_repair_matrix.py, which also pins the restatement to the reference on these
captures): the repairs msg ^ raw of the accepted DF17/18 are exactly the long table's entries, all of them; those of the accepted
DF11 exactly the short table's reachable one-bit entries; every try-phase holds at least 10 % of the accepted."""
import time

import numpy as np
import pytest

import frames_util as fx
import helpers

pytestmark = pytest.mark.gpu

B = 131072
MAX_SAMPLES = 64 * B


@pytest.fixture(scope="module")
def contexts(built):
    import readsb_amd
    cache = {}

    def get(fmt, nfix, fixdf=1, mode_ac=0):
        key = (fmt, nfix, fixdf, mode_ac)
        if key not in cache:
            cache[key] = readsb_amd.Demodulator(fmt=fmt, nfix_crc=nfix, fix_df=fixdf, preamble_threshold=58, mode_ac=mode_ac,
                                                startup_time_ms=helpers.STARTUP_MS, max_samples=MAX_SAMPLES)
        cache[key].reset()
        return cache[key]

    yield get
    for d in cache.values():
        d.close()


def _check(contexts, nfix, fixdf=1, fmt=0, mode_ac=0, chunk_samples=MAX_SAMPLES):
    m = fx.repair_matrix(nfix)
    assert m.nsamples <= MAX_SAMPLES
    want, wst = fx.reference(nfix, fixdf, fmt, mode_ac)
    d = contexts(fmt, nfix, fixdf, mode_ac)
    iq, bps, fused = m.iq(fmt), helpers.FMT_BYTES[fmt], 0.0
    t0 = time.perf_counter()
    for off in range(0, m.nsamples, chunk_samples):
        d.feed_iq(iq[off * bps: min(off + chunk_samples, m.nsamples) * bps])
        fused += d.timing()["sweep_fused_chunks"]
    d.finish()
    got, cnt = d.collect()
    print(f"repair matrix nfix {nfix} fix_df {fixdf} {helpers.FMT_NAMES[fmt]} mode_ac {mode_ac} chunk {chunk_samples}: {len(m.frames)} frames, "
          f"{m.nsamples} samples, reference accepted {len(want)} {np.asarray(wst['demod_accepted']).tolist()} bestPhase "
          f"{np.asarray(wst['demod_bestPhase']).tolist()}, device {len(got)} in {time.perf_counter() - t0:.3f} s")
    helpers.assert_same_messages(got, want)
    helpers.assert_same_counters(cnt, wst, float_tol=0.0)
    if mode_ac:
        assert fused == 0, "Mode A/C takes the converter and k_sweep, not the fused kernel"
        assert int(cnt["demod_modeac"]) == int(wst["demod_modeac"])
    else:
        assert fused >= 1, "the capture did not go through the fused sweep kernel"
    return want, wst


def test_reference_objects_are_here():
    assert helpers.have_ref(), "oracle/_ref missing: the checker of this module is the reference's own objects"


@pytest.mark.parametrize("nfix", [1, 2])
def test_reference_covers_every_table_entry(built, nfix):
    """The coverage condition, on the reference's list (the device is not asked)."""
    msgs, st = fx.reference(nfix)
    assert fx.check_coverage(nfix, msgs, st) == ((107, 44) if nfix == 1 else (3831, 44))


@pytest.mark.parametrize("chunk_buffers", [64, 1], ids=["one_feed", "buffer_feeds"])
@pytest.mark.parametrize("nfix,fixdf", [(0, 1), (1, 1), (2, 1), (2, 0)])
def test_uc8(contexts, nfix, fixdf, chunk_buffers):
    """Every table entry through the device's two-level lookup, in one feed and in feeds of one buffer (the ICAO filter state and the
    326-sample tail then cross 60 feeds).  nfix 0: no table at all (n_long = n_short = 0), every damaged frame dropped."""
    want, wst = _check(contexts, nfix, fixdf, chunk_samples=chunk_buffers * B)
    acc = np.asarray(wst["demod_accepted"]).tolist()
    assert (acc[1] == 0 and acc[2] == 0) if nfix == 0 else (acc[1] > 500 and (acc[2] > 18000) == (nfix == 2))


@pytest.mark.parametrize("fmt", [1, 2])
def test_sc16_formats(contexts, fmt):
    """The same capture as SC16 and SC16Q11 at nfix 2: the fused converter-and-sweep kernels of those formats in front of k_slice."""
    want, _ = _check(contexts, 2, fmt=fmt)
    assert len(want) > 19000


def test_mode_ac_unfused_path(contexts):
    """Mode A/C on: k_convert_* + k_sweep instead of the fused kernel, the Mode A/C scan over the same magnitudes."""
    want, _ = _check(contexts, 2, mode_ac=1)
    assert len(want) > 19000
