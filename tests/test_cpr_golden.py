"""tests/golden/cpr_cases.npz — cases for cpr.c's three decoders and what the reference's own object file returns for them
(tests/golden/make_cpr_golden.py) — against the float64 numpy restatement in tests/cpr_util.py, which the GPU tests of the pairing
(tests/test_gpu_cpr.py) build their expectations from.  No tolerance: result codes equal, latitudes and longitudes as bit patterns."""
import numpy as np
import pytest

import cpr_util as cu


def test_golden_covers_what_it_claims():
    cases, want = cu.load_golden()
    assert 0 < len(cases) <= 20000
    assert np.array_equal(cases, cu.golden_cases()), "the committed cases are not what tests/cpr_util.py generates"
    for fn, codes in ((0, (-1, -2)), (1, (-1,)), (2, (-1,))):      # (why surface has no -2: tests/golden/make_cpr_golden.py)
        rc = want["rc"][cases["fn"] == fn]
        assert (rc == 0).mean() >= 0.5
        for code in codes:
            assert (rc == code).mean() >= 0.02, f"function {fn}: result {code}"
    # every NL threshold has latitudes decoded on either side of it
    lat = np.abs(want["lat"][(want["rc"] == 0)])
    for t in cu.NL_THRESHOLDS:
        assert ((lat > t - 2e-3) & (lat < t)).any() and ((lat >= t) & (lat < t + 2e-3)).any(), f"threshold {t}"


def test_numpy_restatement_equals_the_reference():
    cases, want = cu.load_golden()
    cu.assert_same_results(cu.decode_cases(cases), want, "numpy restatement against the golden")


def test_encoder_round_trip():
    """The encoder of tests/cpr_util.py against the decoders: a pair encoded from one position decodes to it within a cell's
    resolution (airborne 360 / 59 / 2^17 degrees in latitude; longitude cells are 360 / NL wide)."""
    rng = np.random.default_rng(3)
    n = 2000
    lat, lon = rng.uniform(-86, 86, size=n), rng.uniform(-180, 180, size=n)
    c = np.zeros(n, dtype=cu.CPR_CASE_DTYPE)
    c["even_lat"], c["even_lon"] = cu.encode(lat, lon, 0, 0)
    c["odd_lat"], c["odd_lon"] = cu.encode(lat, lon, 1, 0)
    c["fflag"] = rng.integers(0, 2, size=n)
    r = cu.decode_cases(c)
    ok = r["rc"] == 0
    assert ok.mean() > 0.98                                       # (a position within a rounding step of a zone boundary may straddle it)
    assert np.abs(r["lat"][ok] - lat[ok]).max() <= 360 / 59 / 131072
    dlon = np.abs((r["lon"][ok] - lon[ok] + 180) % 360 - 180)
    assert (dlon <= 360 / np.maximum(cu.nl(lat[ok]) - 1, 1) / 131072).all()


@pytest.mark.skipif(not cu.ref_available(), reason="needs oracle/_ref/full/cpr.o (make -C oracle full, dev container) and gcc")
def test_golden_is_what_the_reference_object_returns(tmp_path):
    """The harness relinked with the reference's object and rerun: the committed arrays, byte for byte."""
    cases, want = cu.load_golden()
    got = cu.run_ref_harness(cases, str(tmp_path))
    assert got.tobytes() == want.tobytes()
    z = np.load(cu.GOLDEN)
    assert z["cases"].tobytes() == cu.golden_cases().tobytes()
    assert z["lat_bits"].tobytes() == got["lat"].tobytes() and z["lon_bits"].tobytes() == got["lon"].tobytes()
    assert z["rc"].tobytes() == got["rc"].astype(np.int8).tobytes()
