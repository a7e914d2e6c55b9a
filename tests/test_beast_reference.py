"""CPU tests: tests/beast_util.py's numpy encoder — the checker of tests/test_gpu_beast_records.py — is pinned against the restated C
encoder (modes_oracle_beast_frame, itself pinned against the whole reference program's streams in tests/test_oracle.py) on the
generated record lists, and against those streams (tests/golden/beast_*.bin) directly, ungated and gated."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import beast_util as bu
import gate_util as gu
import helpers
from helpers import GOLDEN_BEAST

LEVEL_C = """
#include "modes_gpu.h"
void levels(const struct mgpu_msg *m, uint64_t n, double *out) { for (uint64_t i = 0; i < n; ++i) out[i] = mgpu_msg_signal_level(&m[i]); }
"""


@pytest.fixture(scope="module")
def level_lib(tmp_path_factory):
    """mgpu_msg_signal_level (include/modes_gpu.h) as the host's C compiler builds it."""
    d = tmp_path_factory.mktemp("level")
    src, so = os.path.join(d, "level.c"), os.path.join(d, "liblevel.so")
    open(src, "w").write(LEVEL_C)
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(helpers.ROOT, "include"), "-o", so, src], check=True)
    lib = C.CDLL(so)
    lib.levels.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
    return lib


def _restated_frames(msgs, level_lib):
    """modes_oracle_beast_frame per record, fed signalLevel = mgpu_msg_signal_level(record)."""
    msgs = np.ascontiguousarray(msgs)
    n = len(msgs)
    o = np.zeros(n, dtype=helpers.ORACLE_MSG)
    lv = np.empty(n, dtype=np.float64)
    level_lib.levels(msgs.ctypes.data, n, lv.ctypes.data)
    o["timestamp"], o["msgbits"], o["msg"], o["signalLevel"] = msgs["timestamp"], msgs["msgbits"], msgs["msg"], lv
    lib = helpers.oracle_lib()
    lib.modes_oracle_beast_frame.restype = C.c_size_t
    lib.modes_oracle_beast_frame.argtypes = [C.c_void_p, C.c_void_p]
    buf = (C.c_uint8 * 64)()
    return [bytes(buf[:lib.modes_oracle_beast_frame(o[k:k + 1].ctypes.data, buf)]) for k in range(n)]


def _split(stream, length):
    ends = np.cumsum(length)
    return [stream[int(e - l):int(e)] for e, l in zip(ends, length)]


@pytest.mark.parametrize("gen", ["hostile", "signal", "ladder"])
def test_reference_equals_the_restated_encoder(built, level_lib, gen):
    msgs = {"hostile": lambda: bu.hostile_records(40000, 11), "signal": lambda: bu.signal_records(12), "ladder": bu.ladder}[gen]()
    stream, length, deferred = bu.beast_reference(msgs)
    want = _restated_frames(msgs, level_lib)
    got = _split(stream, length)
    bad = [k for k in range(len(msgs)) if got[k] != want[k]]
    assert not bad, (len(bad), bad[:5], got[bad[0]].hex(), want[bad[0]].hex())
    assert len(stream) == sum(len(f) for f in want) and len(deferred) == 0
    if gen != "signal":
        assert set(range(11, 45)) <= set(length.tolist())
    if gen == "hostile":
        bu.check_lengths(msgs)
        bu.check_gated(msgs, bu.random_verdicts(len(msgs), 13), net_rule=True)
        # gated: exactly the frames of the kept messages, deferred entries where the frame would start
        for net_rule in (False, True):
            v = bu.random_verdicts(len(msgs), 14)
            gs, gl, gd = bu.beast_reference(msgs, v, net_rule)
            ok = np.ones(len(msgs), dtype=bool) if not net_rule else msgs["correctedbits"] < 2
            keep = ((v & 3) == 1) & ok
            assert gs == b"".join(want[k] for k in np.nonzero(keep)[0])
            dk = np.nonzero(((v & 3) == 2) & ok & (length > 0))[0]
            assert np.array_equal(gd["index"], dk)
            kept_len = np.where(keep, [len(f) for f in want], 0)
            assert np.array_equal(gl, kept_len) and np.array_equal(gd["offset"], (np.cumsum(kept_len) - kept_len)[dk])


def test_signal_generator_covers_every_byte_and_exact_ties():
    """On the reference's output: all 256 signal bytes occur, the escaped value 0x1a for each sig_len, both sides of every rounding
    boundary, and doubles that lie exactly on a boundary below an even byte (where round-half-even and round-half-up differ)."""
    sums, lens = bu.signal_boundaries()
    sig, x = bu.signal_byte(sums, lens)
    assert set(sig.tolist()) == set(range(256))
    for ln in bu.SIG_LENS:
        s = sig[lens == ln]
        assert 0x1A in s and set(s.tolist()) == set(range(256))
    tie = (x == np.floor(x) + 0.5) & (x < 255) & (np.floor(x) % 2 == 0) & (x > 1)
    assert tie.sum() >= 20
    assert (sig[tie] == np.floor(x[tie])).all()
    assert sig[sums == 1].tolist() == [1] * len(bu.SIG_LENS) and (sig[sums == (1 << 64) - 1] == 255).all()


def _oracle_as_records(o):
    """The restatement's message list as mgpu_msg records: the integer sum behind signalLevel recovered (and checked to give it back)."""
    m = np.zeros(len(o), dtype=bu.MSG)
    for f in ("timestamp", "correctedbits", "msgtype", "msgbits", "addr", "msg", "raw"):
        m[f] = o[f]
    m["sig_len"] = np.where(o["msgbits"] == 112, 268, np.where(o["msgbits"] == 56, 134, 1))
    m["sig_sumsq"] = np.rint(o["signalLevel"] * m["sig_len"] * 65535.0 * 65535.0).astype(np.uint64)
    assert np.array_equal(m["sig_sumsq"].astype(np.float64) / 65535.0 / 65535.0 / m["sig_len"].astype(np.float64), o["signalLevel"])
    return m


@pytest.mark.parametrize("name,synth_kw,opt", GOLDEN_BEAST)
def test_reference_reproduces_the_reference_programs_streams(built, name, synth_kw, opt):
    """Same matching as test_oracle.py::test_beast_frames_equal_the_reference_programs, with the numpy encoder's frames."""
    gold = open(os.path.join(helpers.GOLDEN_DIR, f"beast_{name}.bin"), "rb").read()
    frames = helpers.beast_frames(gold)
    iq = helpers.synth(**synth_kw)
    o, _ = helpers.oracle_run(iq, 0, opt["nfix"], 1, 58, mode_ac=opt["mode_ac"])
    msgs = _oracle_as_records(o)
    stream, length, _ = bu.beast_reference(msgs)
    by_ts = {}
    for k, f in enumerate(_split(stream, length)):
        by_ts.setdefault(int(msgs["timestamp"][k]) & ((1 << 48) - 1), []).append(f)
    assert len(frames) > 0.5 * len(msgs) > 500
    for raw, typ, ts, sig, body in frames:
        assert ts in by_ts and raw in by_ts[ts], (ts, raw.hex())


@pytest.mark.parametrize("name", [g[0] for g in GOLDEN_BEAST])
def test_gated_reference_reproduces_the_forwarded_set(built, name):
    """The gated rule on the restated gate's verdicts: a frame only for messages the whole reference program forwarded, none dropped
    that it forwarded, and with the deferred ones it forwarded spliced in at their offsets, its --dump-beast file byte for byte."""
    gold = open(os.path.join(helpers.GOLDEN_DIR, f"beast_{name}.bin"), "rb").read()
    fwd = gu.golden_forwarded(name)
    _, o, fields = gu.oracle_messages(name)
    v = gu.oracle_gate(o, fields)
    msgs = _oracle_as_records(o)
    assert len(msgs) == len(fwd)
    full = _split(*bu.beast_reference(msgs)[:2])
    stream, length, deferred = bu.beast_reference(msgs, v)
    is_def = np.zeros(len(msgs), dtype=bool)
    is_def[deferred["index"].astype(np.int64)] = True
    assert fwd[length > 0].all() and not fwd[(length == 0) & ~is_def].any()
    out, at = bytearray(), 0
    for e in deferred:
        out += stream[at:int(e["offset"])]
        at = int(e["offset"])
        if fwd[int(e["index"])]:
            out += full[int(e["index"])]
    out += stream[at:]
    assert bytes(out) == gold
