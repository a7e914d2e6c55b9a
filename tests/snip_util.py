"""Checker of the snip tests: `readsb --snip <level>` (snipMode, readsb.c:1187-1206) as a numpy model of its closed form, the
reference program itself (oracle/_ref/full/readsb_full --snip), and the builders of the crafted inputs."""
import os
import subprocess

import numpy as np

import helpers

FULL = os.path.join(helpers.ORACLE_DIR, "_ref", "full", "readsb_full")
RUN = 32                                   # MODES_PREAMBLE_SIZE (readsb.h:118-120)
TILE = 8192                                # kSnipTileSamples (readsb_amd/csrc/kernels.h): samples a workgroup holds at a time
GROUP = 4 * TILE                           # kSnipGroupSamples: samples per workgroup
LEVELS = [-5, 0, 1, 2, 64, 128, 129]
RUN_LENGTHS = [0, 1, 31, 32, 33, 34, 63, 64, 65, 95, 96, 97, 1000]
MGPU_OK, MGPU_E_INVAL, MGPU_E_OVERFLOW = 0, -1, -5


def quiet_flags(iq, level):
    """quiet(k) = abs(i - 127) < level && abs(q - 127) < level in int arithmetic."""
    s = np.frombuffer(bytes(iq), dtype=np.uint8)
    s = s[: s.size // 2 * 2].reshape(-1, 2).astype(np.int64)
    return (np.abs(s[:, 0] - 127) < level) & (np.abs(s[:, 1] - 127) < level)


def model(iq, level, c_in=0):
    """-> (kept bytes, c_out): one call of n samples with carry c_in, by the closed form — p(k) the last loud sample before k in this
    call, run(k) = k - p(k) or c_in + k + 1 without one, keep(k) = !quiet(k) || run(k) <= 32; c_out the trailing quiet samples, or
    c_in + n (uint64) for a call without a loud sample."""
    quiet = quiet_flags(iq, level)
    n = quiet.size
    k = np.arange(n, dtype=np.int64)
    last_loud = np.maximum.accumulate(np.where(quiet, -1, k)) if n else k
    p = np.concatenate(([-1], last_loud[:-1])) if n else k
    run = np.where(p >= 0, k - p, min(int(c_in), 2 * RUN) + k + 1)           # (beyond 32 only "more than 32" matters)
    keep = ~quiet | (run <= RUN)
    s = np.frombuffer(bytes(iq), dtype=np.uint8)[: 2 * n].reshape(-1, 2)
    c_out = n - 1 - int(last_loud[-1]) if n and last_loud[-1] >= 0 else (int(c_in) + n) % (1 << 64)
    return s[keep].tobytes(), c_out


def sequential(iq, level, c=0):
    """The reference's loop itself, for small inputs: the model's own check."""
    out = bytearray()
    b = bytes(iq)
    for k in range(len(b) // 2):
        i, q = b[2 * k], b[2 * k + 1]
        if abs(i - 127) < level and abs(q - 127) < level:
            c = (c + 1) % (1 << 64)
            if c > RUN:
                continue
        else:
            c = 0
        out += bytes((i, q))
    return bytes(out), c


def have_reference():
    return os.path.exists(FULL)


def reference_snip(iq_bytes, level):
    """stdout of `readsb_full --snip=<level>` fed iq_bytes on stdin (exit status 0 asserted)."""
    r = subprocess.run([FULL, f"--snip={int(level)}"], input=bytes(iq_bytes), capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr[-500:]
    return r.stdout


def edge_bytes(level):
    """-> (quiet bytes, loud bytes) at the decision edges 127 +- level, 127 +- (level - 1), and 0, 255, 127; either may be empty."""
    cand = sorted({min(255, max(0, b)) for b in (127 - level, 127 + level, 127 - (level - 1), 127 + (level - 1), 0, 255, 127)})
    return [b for b in cand if abs(b - 127) < level], [b for b in cand if abs(b - 127) >= level]


def crafted(level, nsamples=200003):
    """Alternating [loud x a][quiet x L], L cycling through RUN_LENGTHS and a through 1..67 (13 and 67 are coprime: run starts and the
    32/33 boundary land on every residue mod 64 and across every tile edge), bytes at the decision edges of `level`.  Where the level
    has no quiet (or no loud) byte the stream is all loud (all quiet) by construction."""
    qb, lb = edge_bytes(level)
    want_quiet = np.zeros(nsamples, dtype=bool)
    at = seg = 0
    while at < nsamples:
        at += 1 + seg % 67
        run = RUN_LENGTHS[seg % len(RUN_LENGTHS)]
        want_quiet[at: at + run] = True
        at += run
        seg += 1
    k = np.arange(nsamples)
    q_pool, l_pool = np.array(qb or lb, dtype=np.uint8), np.array(lb or qb, dtype=np.uint8)
    iq = np.empty((nsamples, 2), dtype=np.uint8)
    # quiet samples: both bytes quiet; loud samples: (loud, quiet), (quiet, loud), (loud, loud) in turn
    iq[:, 0] = np.where(want_quiet | (k % 3 == 1), q_pool[k % q_pool.size], l_pool[k % l_pool.size])
    iq[:, 1] = np.where(want_quiet | (k % 3 == 0), q_pool[(k // 2) % q_pool.size], l_pool[(k // 3) % l_pool.size])
    return iq.tobytes()


def random_stream(nsamples, loud_density, seed, level=4):
    """Samples that are loud with the given probability: quiet bytes within 127 +- (level - 1), loud ones with a byte at 127 +- level or beyond."""
    rng = np.random.default_rng(seed)
    loud = rng.random(nsamples) < loud_density if 0 < loud_density < 1 else np.full(nsamples, loud_density >= 1)
    iq = rng.integers(127 - (level - 1), 127 + level, size=(nsamples, 2)).astype(np.uint8)
    which = rng.integers(0, 2, size=nsamples)
    far = np.where(rng.integers(0, 2, size=nsamples) == 0, 127 - level - rng.integers(0, 3, size=nsamples), 127 + level + rng.integers(0, 3, size=nsamples))
    iq[loud, which[loud]] = far[loud].astype(np.uint8)
    return iq.tobytes()


def cut_points(nsamples, ncuts, seed):
    """Seeded random cut points of a stream into calls, with 0-sample and 1-sample calls among them. -> sorted boundaries 0 .. nsamples"""
    rng = np.random.default_rng(seed)
    cuts = sorted(int(x) for x in rng.integers(0, nsamples + 1, size=ncuts))
    cuts += [cuts[0], cuts[len(cuts) // 2], min(cuts[1] + 1, nsamples), min(cuts[-1] + 1, nsamples)]     # empty and one-sample calls
    return [0] + sorted(cuts) + [nsamples]
