"""-m gpu: candidate densities four to ten times what the rest of the suite shows the kernels, and the record pool's overflow contract.

Gaussian noise of 12 / 25 LSB at the reference's lowest threshold (40) gives 48-62 preambles per 1000 samples in the reference (the
suite's densest capture before: 13) — k_slice's pooled chunk allocation and chain linking, the pre-screen's segment chains, the count /
write passes and the host walk's batch restarts at a load nothing else reaches.  The checker is the reference's own objects
(helpers.reference_run); tests/test_oracle.py pins the same five captures on the CPU.

The device record pool: mgpu_config.record_pool_records (0 = chunk samples / 16 + 65536) PLUS a reserve of 1024 records per unit of
8192 positions for at most 4096 units (alloc_all, api.cpp) — every k_slice wave's first slice of 256 records lies in that reserve.
A pool that is too small is a clean error (MGPU_E_OVERFLOW, "recreate the context with a larger record_pool_records"), never a
wrong list."""
import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu

B = 131072
DENSE = [   # helpers.synth arguments, fmt; all at nfix 2, threshold 40
    (dict(seed=71, rate=2000.0, dense=4, noise=12.0), 0),
    (dict(seed=72, rate=20000.0, dense=6, noise=12.0), 0),
    (dict(seed=73, rate=20000.0, dense=7, noise=12.0), 0),
    (dict(seed=74, rate=8000.0, dense=7, noise=25.0), 2),
    (dict(seed=75, rate=8000.0, dense=7, noise=12.0), 1),
]


def _is_pool_overflow(exc):
    return "record pool overflow" in str(exc)


def _run(iq, fmt, pool, nfix=2, thr=40, **kw):
    """One context, the capture in one feed -> (messages, counters, timing of the feed)."""
    import readsb_amd
    n = len(iq) // helpers.FMT_BYTES[fmt]
    kw.setdefault("max_samples", max(n, B))
    d = readsb_amd.Demodulator(fmt=fmt, nfix_crc=nfix, preamble_threshold=thr, startup_time_ms=helpers.STARTUP_MS,
                               record_pool_records=pool, **kw)
    try:
        d.feed_iq(iq)
        tm = d.timing()
        d.finish()
        msgs, cnt = d.collect()
        return msgs, cnt, tm
    finally:
        d.close()


@pytest.mark.parametrize("skw,fmt", DENSE, ids=[f"seed{k['seed']}-fmt{f}" for k, f in DENSE])
def test_exact_at_density(built, skw, fmt):
    """2 s each, pool of nsamples / 2 records (the test is about the kernels, not the default pool).  Measured on an MI355X, per 1000
    samples (reference preambles / device records before the pre-screen / live records after it):
      seed 71 UC8      62.49 / 36.43 / 0.46        seed 74 SC16Q11  60.69 / 32.44 / 0.06
      seed 72 UC8      56.98 / 35.13 / 0.17        seed 75 SC16     59.74 / 38.54 / 0.76
      seed 73 UC8      48.40 / 28.13 / 0.11
    (a measurement, printed by the test; nothing is asserted about it beyond the reference's >= 45 preambles per 1000.)"""
    iq = helpers.synth(seconds=2.0, fmt=fmt, **skw)
    n = len(iq) // helpers.FMT_BYTES[fmt]
    want, wst = helpers.reference_run(iq, fmt, 2, 1, 40)
    assert int(wst["demod_preambles"]) / n * 1000 >= 45, "not a dense capture"
    got, cnt, tm = _run(iq, fmt, n // 2)
    print(f"density seed {skw['seed']} fmt {fmt}: reference preambles/1000 {int(wst['demod_preambles']) / n * 1000:.2f}, "
          f"records/1000 {tm['n_records'] / n * 1000:.2f}, live/1000 {tm['n_live_records'] / n * 1000:.2f}, messages {len(want)}")
    helpers.assert_same_messages(got, want)
    helpers.assert_same_counters(cnt, wst, float_tol=0.0)


def test_default_pool_at_density(built):
    """The seed-71 capture with the default pool: exact, or the overflow error — a list that differs fails.  (Measured on an MI355X: exact — 36.4 records per
    1000 samples against the default's 62.5 plus the reserve's 125.)"""
    skw, fmt = DENSE[0]
    import readsb_amd
    iq = helpers.synth(seconds=2.0, fmt=fmt, **skw)
    want, wst = helpers.reference_run(iq, fmt, 2, 1, 40)
    try:
        got, cnt, tm = _run(iq, fmt, 0)
    except readsb_amd.MgpuError as e:
        assert _is_pool_overflow(e), e
        print(f"default pool at density: {e}")
        return
    print(f"default pool at density: exact, records/1000 {tm['n_records'] / (len(iq) // 2) * 1000:.2f}")
    helpers.assert_same_messages(got, want)
    helpers.assert_same_counters(cnt, wst, float_tol=0.0)


def test_smallest_pool_on_ordinary_traffic(built):
    """record_pool_records = 1, the smallest value mgpu_create takes as a size, far below the 1766 messages the reference finds in 2 s
    of the seed-101 capture.  This does NOT have to overflow: the pool also holds the reserve (1024 records per 8192 positions here,
    125 per 1000 samples), which ordinary traffic (6 preambles per 1000) does not fill.  So: exact, or the overflow error, never
    another list; and the default pool is exact."""
    import readsb_amd
    iq = helpers.synth(seconds=2.0, seed=101)
    want, wst = helpers.reference_run(iq, 0, 1, 1, 58)
    assert len(want) > 1000
    try:
        got, cnt, _ = _run(iq, 0, 1, nfix=1, thr=58)
    except readsb_amd.MgpuError as e:
        assert _is_pool_overflow(e), e
    else:
        helpers.assert_same_messages(got, want)
        helpers.assert_same_counters(cnt, wst, float_tol=0.0)
    got, cnt, _ = _run(iq, 0, 0, nfix=1, thr=58)
    helpers.assert_same_messages(got, want)
    helpers.assert_same_counters(cnt, wst, float_tol=0.0)


def test_overflow_is_an_error_and_never_a_list(built):
    """An overflow that follows from counting.  With record_pool_records = 1 a chunk's pool is 1 + 1024 * min(units, 4096) records, at
    most 4194305 however long the chunk — so the chunk has to be long: 100 s of the seed-71 settings as ONE pipeline chunk
    (chunk_buffers 2048).  Every candidate the reference rejects as 'unknown ICAO' or accepts has a try-phase whose score is not -2,
    and the device scores every candidate position the reference does (and those the reference skips behind an accepted frame), so
    it needs at least one record for each: 18 per 1000 samples, 4.4 million — counted from the reference's statistics below, and
    more than the pool holds.  feed / finish / collect must raise MGPU_E_OVERFLOW; a list must not come back.  Then the same
    capture with room for its records (two chunks of 1024 buffers, an expiry of the ICAO filter at 60 s) is exact.

    Why every access after the overflow is in bounds: k_slice writes a segment (header + records) only under
    `base + kPoolChunkRecords <= pool_cap` and links it (unit_first / the previous header's addr) in the same branch, so a chain
    only ever names segments that were written whole; a refused segment moves chunk_base past prev_end, so nothing is appended to
    the segment before it either.  k_count and the write pass follow those links alone (record loads clamped to pool_cap - 1,
    masked by the header's count), the live list is as large as the pool, and fetch_slot returns the error before it reads the
    live count."""
    import readsb_amd
    skw, fmt = DENSE[0]
    nbuf = 1832                                                   # 100.05 s
    iq = helpers.synth(nsamples=nbuf * B, fmt=fmt, threads=16, **skw)
    n = nbuf * B
    want, wst = helpers.reference_run(iq, fmt, 2, 1, 40)
    need = int(wst["demod_rejected_unknown_icao"]) + int(np.sum(wst["demod_accepted"]))
    pool_cap = 1 + 1024 * min((n + 8191) // 8192, 4096)
    assert need > pool_cap, (need, pool_cap)
    with pytest.raises(readsb_amd.MgpuError) as ei:
        _run(iq, fmt, 1, max_samples=n, chunk_buffers=2048)
    assert _is_pool_overflow(ei.value), ei.value
    assert int(wst["nflips"]) >= 2
    got, cnt, tm = _run(iq, fmt, 1024 * B // 8, max_samples=n)     # 125 records per 1000 samples of a chunk (measured need: 36)
    helpers.assert_same_messages(got, want)
    helpers.assert_same_counters(cnt, wst, float_tol=0.0)
