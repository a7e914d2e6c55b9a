"""CPU pin of the repair matrix (tests/frames_util.py; the -m gpu side is tests/test_gpu_repair_matrix.py): the restatement
(oracle/modes_oracle.c) on the same captures must equal the reference's own objects (oracle/_ref) exactly, for nfix 0, 1 and 2 —
and the coverage condition is asserted here, on the reference's list, so that a capture which no longer reaches every table entry
fails on the CPU before anything runs on a GPU.

The last two tests show that the comparison and the coverage condition notice what they are for: a one-bit table where the two-bit
table was meant, and one entry missing from 3831."""
import numpy as np
import pytest

import frames_util as fx
import helpers

needs_ref = pytest.mark.skipif(not helpers.have_ref(), reason="oracle/_ref not built")


def _same(a, sa, b, sb):
    assert len(a) == len(b) and a.tobytes() == b.tobytes()
    for f in helpers.COUNTER_FIELDS:
        assert np.array_equal(np.asarray(sa[f]), np.asarray(sb[f])), f
    for f in ("signal_power_sum", "peak_signal_power", "noise_power_sum"):
        assert float(sa[f]) == float(sb[f]), f


def test_modulator_envelope():
    """One DF17 frame at each alignment, by hand: pulses of 6 ticks at 0, 12, 42, 54 and from 96 on (first half of the bit for a 1),
    box-averaged over 5 ticks, on I over the floor; SC16 / SC16Q11 are the same samples scaled exactly."""
    fr = bytes([0x8D, 0x4B, 0x17, 0x2A] + [0] * 10)
    for align in range(5):
        uc8 = fx.modulate([(fr, 112, 5 * 10 + align, 100)], nsamples=400)
        i, q = uc8[0::2].astype(int), uc8[1::2].astype(int)
        env = np.zeros(400 * 5)
        bits = np.unpackbits(np.frombuffer(fr, dtype=np.uint8))
        for p in [0, 12, 42, 54] + [96 + 12 * k + (0 if bits[k] else 6) for k in range(112)]:
            env[50 + align + p: 50 + align + p + 6] = 100
        assert np.array_equal(i, np.floor(127.5 + fx.FLOOR + env.reshape(-1, 5).mean(axis=1) + 0.5).astype(int))
        assert (q == 128).all() and i[:10].tolist() == [130] * 10 and i.max() == 230
        assert np.array_equal(fx.to_sc16(uc8).view("<i2").astype(float), (uc8.astype(float) - 127.5) * 256)
        assert np.array_equal(fx.to_sc16(uc8, q11=True).view("<i2").astype(float), (uc8.astype(float) - 127.5) * 16)
    noisy = fx.modulate([(fr, 112, 50, 100)], nsamples=400, noise_lsb=3.0, seed=5)
    assert np.array_equal(noisy, fx.modulate([(fr, 112, 50, 100)], nsamples=400, noise_lsb=3.0, seed=5))
    assert 0 < np.abs(noisy.astype(int) - fx.modulate([(fr, 112, 50, 100)], nsamples=400).astype(int)).max() <= 4
    with pytest.raises(AssertionError, match="overlap"):
        fx.modulate([(fr, 112, 0, 100), (fr, 112, 1000, 100)])


def test_matrix_holds_what_it_says():
    """The capture's frame list against the tables: every long entry five times with exactly its bits flipped, every 8th DF18, all
    true addresses primed, AA repairs over 0 and 1 bits; both one-bit tables are the one-bit parts of --aggressive's."""
    assert fx.table_entries("nfix1_112") == {e for e in fx.table_entries("nfix2_112") if len(e) == 1}
    assert fx.table_entries("nfix1_56") == {e for e in fx.table_entries("nfix2_56") if len(e) == 1}
    for nfix in (1, 2):
        m = fx.repair_matrix(nfix)
        t = fx.TABLES[f"nfix{nfix}_112"]
        sel = np.nonzero(m.kind == fx.KINDS.index("long"))[0]
        assert len(sel) == 5 * len(t) and m.nsamples <= 64 * 131072
        syn = fx.fu.crc24_vec(m.frames[sel], 14)
        assert np.array_equal(syn, t[m.entry[sel], 0].astype(np.uint32))                   # the syndrome on the air IS the entry's
        assert {(int(e), int(a)) for e, a in zip(m.entry[sel], m.align[sel])} == {(e, a) for e in range(len(t)) for a in range(5)}
        df = m.frames[sel, 0] >> 3
        assert np.array_equal(df == 18, m.entry[sel] % 8 == 7) and ((df == 17) | (df == 18)).all()
        short = np.nonzero((m.kind == fx.KINDS.index("short")))[0]
        assert len(short) == 51 * 5 * 4 and (m.frames[short, 0] >> 3 == 11).all()
        # a repaired AA bit is a 0 in some frames and a 1 in others
        aa_bits = np.unpackbits(m.frames[sel, 1:4], axis=1)
        for b in range(8, 32):
            hit = (t[m.entry[sel], 2] == b) | (t[m.entry[sel], 3] == b)
            assert set(aa_bits[hit, b - 8].tolist()) == {0, 1}, b


@needs_ref
@pytest.mark.parametrize("nfix,fixdf", [(0, 1), (1, 1), (2, 1), (2, 0)])
def test_restatement_equals_reference_on_the_matrix(built, nfix, fixdf):
    m = fx.repair_matrix(nfix)
    want, wst = fx.reference(nfix, fixdf)
    got, gst = helpers.oracle_run(m.uc8, 0, nfix, fixdf, 58)
    _same(got, gst, want, wst)
    assert len(want) > (300 if nfix == 0 else 1000 if nfix == 1 else 19000)


@needs_ref
@pytest.mark.parametrize("fmt,mode_ac", [(1, 0), (2, 0), (0, 1)])
def test_restatement_equals_reference_on_the_other_formats_and_mode_ac(built, fmt, mode_ac):
    m = fx.repair_matrix(2)
    want, wst = fx.reference(2, 1, fmt, mode_ac)
    got, gst = helpers.oracle_run(m.iq(fmt), fmt, 2, 1, 58, mode_ac=mode_ac)
    _same(got, gst, want, wst)
    assert len(want) > 19000


@needs_ref
@pytest.mark.parametrize("nfix", [1, 2])
def test_reference_covers_every_table_entry(built, nfix):
    """Section "coverage" of the matrix: asserted on the reference's list alone."""
    msgs, st = fx.reference(nfix)
    nlong, nshort = fx.check_coverage(nfix, msgs, st)
    assert (nlong, nshort) == ((107, 44) if nfix == 1 else (3831, 44))


@needs_ref
def test_reference_rejects_or_misrepairs_what_is_outside_the_tables(built):
    """What the capture holds beyond the tables does what it was put there for (on the reference's list): no DF11 with two flipped
    bits is accepted as repaired, DF-field repairs happen with fix_df and not without, an Address/Parity frame with its last bit flipped
    passes as the neighbouring address, the all-zero frames and the formats that are none come to nothing."""
    m = fx.repair_matrix(2)
    for fixdf in (1, 0):
        msgs, st = fx.reference(2, fixdf)
        idx = fx.frame_of(m, msgs)
        kind = m.kind[idx]
        K = fx.KINDS.index
        assert (msgs["correctedbits"][kind == K("short2")] == 0).all()          # (accepted only where both bits lie inside the IID)
        dffix = msgs[(kind == K("dfbit"))]
        assert (len(dffix) == 50 and (dffix["correctedbits"] == 1).all() and (dffix["msgtype"] == 17).all()) if fixdf else len(dffix) == 0
        assert set(dffix["score"].tolist()) == ({900, 700} if fixdf else set())
        ap = msgs[kind == K("ap_flip")]
        assert len(ap) == 12 and set(ap["addr"].tolist()) == {int(fx.KNOWN[0]), fx.NEIGHBOUR}
        unk, sent = msgs[kind == K("long_unknown")], m.kind == K("long_unknown")
        t = fx.TABLES["nfix2_112"][m.entry[sent]]
        outside_aa = ~(((t[:, 2] >= 8) & (t[:, 2] <= 31)) | ((t[:, 3] >= 8) & (t[:, 3] <= 31)))
        assert 50 < len(unk) == outside_aa.sum() < sent.sum() - 100                      # accepted exactly where the repair left AA alone
        assert (unk["addr"] == fx.UNKNOWN_REPAIR).all() and set(unk["score"].tolist()) == {700, 466}
        grid = msgs[kind == K("grid")]
        assert set(grid["msgtype"].tolist()) == {0, 4, 5, 11, 16, 17, 18, 20, 21}
        assert (m.frames[idx].any(axis=1)).all()
        assert int(st["demod_rejected_unknown_icao"]) > 1000 and int(st["demod_rejected_bad"]) > 1000


@needs_ref
def test_comparison_notices_a_one_bit_table(built):
    """Sensitivity: the restatement given nfix 1 on the capture built for nfix 2 differs loudly from the reference at nfix 2."""
    m = fx.repair_matrix(2)
    want, wst = fx.reference(2)
    got, gst = helpers.oracle_run(m.uc8, 0, 1, 1, 58)
    assert len(want) - len(got) > 15000
    with pytest.raises(AssertionError):
        _same(got, gst, want, wst)


@needs_ref
def test_coverage_notices_one_missing_entry(built):
    """Sensitivity: with one entry of 3831 taken out — of the expected set, or of the capture — the coverage condition fails."""
    msgs, st = fx.reference(2)
    full = fx.table_entries("nfix2_112")
    row = 1917
    gone = tuple(int(b) for b in fx.TABLES["nfix2_112"][row, 2:4])
    assert gone in full
    with pytest.raises(AssertionError, match="1 repairs outside the table"):
        fx.check_coverage(2, msgs, st, long_entries=full - {gone})
    short = fx.repair_matrix(2, drop_long_entry=row)
    msgs2, st2 = helpers.reference_run(short.uc8, 0, 2, 1, 58)
    found_long, _ = fx.coverage(msgs2)
    assert full - found_long == {gone}


def test_device_lookup_on_all_syndromes(built, tmp_path):
    """The slicer kernels' two-level lookup (kernels/crc_lookup.inc), compiled unchanged for the host: all 2^24 syndromes in both
    tables for nfix 0, 1 and 2 against mgpu_crc_diagnose (tests/host_stub/key_tables_check.cpp) — false hits on noise syndromes
    and every bucket edge, which no stream of frames can show."""
    import os
    import re
    import subprocess
    csrc = os.path.join(helpers.ROOT, "readsb_amd", "csrc")
    kblock = re.search(r"constexpr int kBlock = (\d+);", open(os.path.join(csrc, "kernels.h")).read()).group(1)
    exe = str(tmp_path / "key_tables_check")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wno-unknown-pragmas", f"-DK_BLOCK={kblock}", "-o", exe,
                    os.path.join(helpers.ROOT, "tests", "host_stub", "key_tables_check.cpp"), "-L" + csrc, "-lmodes_gpu", "-Wl,-rpath," + csrc],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 3 and all(ln.endswith(" 0 differences") for ln in lines), r.stdout
    assert "long 3831 entries 3831 hits, short 1326 entries 1326 hits" in lines[2] and "long 107 entries 107 hits, short 51 entries 51 hits" in lines[1]
