"""-m gpu: the ICAO filter driven from outside (mgpu_config.filter_clock, mgpu_filter_expire, mgpu_filter_add: the deployment of
INTEGRATION.md §2, where a host that keeps its own filter forwards what it does to it).  The filter scripts of tests/filter_util.py
— expiries and adds between feeds, adds of addresses the demodulator never heard, generations, table growth and shrinking, a seeded
mix — through the library, exact: every feed's messages and the counters after it equal the checker's (helpers.reference_run with
the same script; tests/test_oracle_filter_script.py shows on the CPU that each script separates what it claims).  The checker is the
reference's own objects where oracle/_ref was built from a harness that takes scripts, the restatement pinned to them otherwise;
the per-feed counts recorded from the reference (filter_util.RECORDED) are asserted either way.  Each test is one context over at
most 8 buffers."""
import numpy as np
import pytest

import filter_util as fu
import helpers

pytestmark = pytest.mark.gpu

B = helpers.BUF_SAMPLES
TR = helpers.TRAILING


def _demodulator(s, fmt=0, nfix=1, mode_ac=0, clock=None, chunk_buffers=None):
    import readsb_amd
    return readsb_amd.Demodulator(fmt=fmt, nfix_crc=nfix, mode_ac=mode_ac, startup_time_ms=helpers.STARTUP_MS, max_samples=8 * B,
                                  filter_clock=s.clock if clock is None else clock, chunk_buffers=chunk_buffers)


def _check_feed(k, got, cnt, want):
    wm, ws = want[k]
    try:
        helpers.assert_same_messages(got, wm)
        helpers.assert_same_counters(cnt, ws)
        assert int(cnt["demod_modeac"]) == int(ws["demod_modeac"])
    except AssertionError as e:
        raise AssertionError(f"feed {k}: {e}") from None


def _run(d, ops, want, refused_expire=False):
    """The script through feed_iq / collect, feed by feed.  refused_expire: the context runs its own filter clock, so every
    filter_expire() of the script must be refused (and change nothing: `want` is the script without them)."""
    import readsb_amd
    k = 0
    for op in ops:
        if op[0] == "feed":
            d.feed_iq(op[1])
            got, cnt = d.collect()
            _check_feed(k, got, cnt, want)
            k += 1
        elif op[0] == "add":
            d.filter_add(op[1])
        elif refused_expire:
            with pytest.raises(readsb_amd.MgpuError, match="invalid|filter clock"):
                d.filter_expire()
        else:
            d.filter_expire()
    assert k == len(want)


@pytest.mark.parametrize("name", fu.ALL)
def test_filter_script(built, name):
    s = fu.scenario(name)
    want = fu.reference(name)
    if name in fu.RECORDED:                                 # what oracle/_ref gave when the scenario was written, whatever checks today
        assert fu.counts(want) == fu.RECORDED[name][0]
    d = _demodulator(s)
    _run(d, s.ops, want)
    d.close()


@pytest.mark.parametrize("name", ["foreign_add", "grow"])
@pytest.mark.parametrize("fmt,nfix,mode_ac", [(1, 1, 0), (2, 1, 0), (0, 2, 0), (0, 1, 1)], ids=["sc16", "sc16q11", "nfix2", "modeac"])
def test_filter_script_other_configurations(built, name, fmt, nfix, mode_ac):
    s = fu.scenario(name)
    d = _demodulator(s, fmt=fmt, nfix=nfix, mode_ac=mode_ac)
    _run(d, fu.in_format(s.ops, fmt), fu.reference(name, fmt, nfix, mode_ac))
    d.close()


@pytest.mark.parametrize("name,chunk_buffers", [(n, 1) for n in fu.ALL] + [(f"fuzz{k}", 2) for k in fu.FUZZ_SEEDS])
def test_filter_script_small_chunks(built, name, chunk_buffers):
    """chunk_buffers 1 is the smallest mgpu_create takes (0 = the default): a fuzz script's 2- and 3-buffer feeds are several
    pipeline chunks; with 2, a 3-buffer feed is a chunk of two buffers (two ranges of the parallel walk) and one of one."""
    s = fu.scenario(name)
    d = _demodulator(s, chunk_buffers=chunk_buffers)
    _run(d, s.ops, fu.reference(name))
    d.close()


@pytest.mark.parametrize("device_messages", [0, 1], ids=["host_list", "device_list"])
@pytest.mark.parametrize("name", ["foreign_add", "grow", "shrink"] + [f"fuzz{k}" for k in fu.FUZZ_SEEDS])
def test_filter_script_deferred(built, name, device_messages):
    """Deferred feeds: the script's operations arrive while the feed before them is still in flight (nothing of it collected yet).
    mgpu_filter_expire / mgpu_filter_add drain first, so every feed's messages are the synchronous run's — the checker's — and so
    are the counters once everything has landed.  (Counters between feeds would take a drain of their own, which is what this test
    leaves to the filter calls.)  device_list: the messages are built on the GPU (k_build_messages) and copied out of HBM."""
    import readsb_amd
    s = fu.scenario(name)
    want = fu.reference(name)
    d = _demodulator(s, chunk_buffers=2)
    d.set_deferred(True)
    if device_messages:
        d.set_device_messages(1)
    buf = np.empty(8192, dtype=readsb_amd.MSG_DTYPE)
    got, fed = [], 0
    for op in s.ops:
        if op[0] == "feed":
            if fed - len(got) == 2:                       # two feeds in flight at the most: take the older one
                got.append(d.collect_feed(buf)[0].copy())
            d.feed_iq(op[1])
            fed += 1
        elif op[0] == "add":
            d.filter_add(op[1])
        else:
            d.filter_expire()
    cnt = None
    while len(got) < fed:
        m, cnt = d.collect_feed(buf, want_counters=len(got) == fed - 1)
        got.append(m.copy())
    for k, m in enumerate(got):
        try:
            helpers.assert_same_messages(m, want[k][0])
        except AssertionError as e:
            raise AssertionError(f"feed {k}: {e}") from None
    helpers.assert_same_counters(cnt, want[-1][1])
    d.set_deferred(False)
    d.close()


def test_reset_forgets_the_foreign_add(built):
    """mode 2: after foreign_add, a reset and a replay WITHOUT the add give the without-add result (the device's pre-screen bitmap has
    forgotten FOREIGN as the filter has), and one more reset and a replay with the add give the with-add result again."""
    s = fu.scenario("foreign_add")
    with_add, without = fu.reference("foreign_add"), fu.reference("foreign_add", which="no_add")
    assert fu.counts(with_add) == fu.RECORDED["foreign_add"][0] and fu.counts(without) == fu.RECORDED["foreign_add"][1]["no_add"]
    d = _demodulator(s)
    _run(d, s.ops, with_add)
    d.reset()
    _run(d, s.without["no_add"], without)
    d.reset()
    _run(d, s.ops, with_add)
    d.close()


def test_adder_bitmap_holds_the_hosts_adds(built):
    """The pre-screen's bitmap (what the shard protocol hands from rank to rank as "may be known") is a superset of the filter: a
    host's add sets the address's bit and nothing else, an address >= 2^24 has no bit, reset clears."""
    s = fu.scenario("foreign_add")
    d = _demodulator(s)
    assert not d.adder_bitmap().any()
    for addr in (fu.SHOW_ONLY, fu.BIG, fu.FOREIGN, fu.FOREIGN, 0, 0xFFFFFF):
        d.filter_add(addr)
    words = d.adder_bitmap()
    want = np.zeros_like(words)
    for addr in (fu.FOREIGN, 0, 0xFFFFFF):
        want[addr >> 5] |= np.uint32(1 << (addr & 31))
    assert (words == want).all()
    d.reset()
    assert not d.adder_bitmap().any()
    d.close()


def _mag_bufs(iq, fmt, state):
    """ifileRun's grid over one feed (sdr_ifile.c:194-241), as the drop-in adapter hands it over: -> (data = 326 carried-over
    magnitudes + the buffer's own, length, sampleTimestamp, sysTimestamp, mean_level, mean_power) per buffer."""
    n = np.ascontiguousarray(iq).view(np.uint8).size // helpers.FMT_BYTES[fmt]
    bps = helpers.FMT_BYTES[fmt]
    for off in range(0, n, B):
        slen = min(B, n - off)
        mag, ml, mp = helpers.oracle_convert(iq[off * bps:(off + slen) * bps], fmt)
        data = np.zeros(TR + slen, dtype=np.uint16)
        last = state.get("last")
        if last is not None and len(last) - TR >= TR:
            data[:TR] = last[-TR:]
        data[TR:] = mag
        st = state.get("samples", 0) * 5
        yield data, slen, st, st // 12000 + helpers.STARTUP_MS, ml, mp
        state["last"], state["samples"] = data, state.get("samples", 0) + slen


@pytest.mark.parametrize("name", ["foreign_add", "grow"])
@pytest.mark.parametrize("mode_ac", [0, 1], ids=["demod_mag_buf", "demod_mag_buf_ac"])
def test_filter_script_through_the_mag_buf_entries(built, name, mode_ac):
    """What the drop-in adapter calls (demodulate2400 / demodulate2400AC redirected, one struct mag_buf at a time, with the host's
    expiries and adds forwarded in between), without the reference program: magnitudes from the checker's converter."""
    s = fu.scenario(name)
    want = fu.reference(name, mode_ac=mode_ac)
    d = _demodulator(s, mode_ac=mode_ac)
    state, k = {}, 0
    for op in s.ops:
        if op[0] == "feed":
            for data, slen, st, sys, ml, mp in _mag_bufs(op[1], 0, state):
                if mode_ac:
                    d.demod_mag_buf_ac(data, slen, st, sys, ml, mp)
                else:
                    d.demod_mag_buf(data, slen, st, sys, mp)
            got, cnt = d.collect()
            _check_feed(k, got, cnt, want)
            k += 1
        elif op[0] == "add":
            d.filter_add(op[1])
        else:
            d.filter_expire()
    assert k == len(want)
    d.close()


@pytest.mark.parametrize("clock", [0, 1])
@pytest.mark.parametrize("name", ["foreign_add", "grow"])
def test_own_clock_refuses_expire_and_takes_adds(built, name, clock):
    """filter_clock 0 / 1: mgpu_filter_expire is refused (MGPU_E_INVAL) and changes nothing — the rest of the script still matches
    the checker, which runs the script without its expires under the same clock — while mgpu_filter_add is taken in every mode:
    the host's add of FOREIGN separates there too."""
    s = fu.scenario(name)
    kept = [op for op in s.ops if op[0] != "expire"]
    want = helpers.reference_run(None, ops=kept, filter_clock=clock)
    if name == "foreign_add":
        no_add = [op for op in s.without["no_add"] if op[0] != "expire"]
        assert fu.counts(helpers.reference_run(None, ops=no_add, filter_clock=clock)) != fu.counts(want)
    d = _demodulator(s, clock=clock)
    _run(d, s.ops, want, refused_expire=True)
    d.close()
