"""Writes tests/golden/dump_cases.npz: the case sets of tests/dump_util.py and, per set and mode, the bytes the REFERENCE's
displayModesMessage printed for them (tests/host_stub/dump_ref_harness.c, linked against oracle/_ref/full) with the length per case.
Needs the reference tree and the full build (`__graft_entry__.build()`).  Asserts on the reference's output that every line of the
dump appears in at least five cases, that no case of groups (a)-(d) is near an RSSI rounding boundary (so "0 deferred" there is the
reference's alone), that exactly the near cases of group (e) are, and that the plain-Python model of tests/dump_util.py prints the
harness's bytes.
    python tests/golden/make_dump_golden.py"""
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import dump_util as du  # noqa: E402

# one marker per printf of displayModesMessage / sprintACASInfoShort a demodulated message can reach
MARKERS = [b"hex:  ", b"hex: ~", b" ? CRC", b"RSSI: ", b"reduce_forward: 0\n", b"reduce_forward: 1\n", b"Score: ", b"receiverId: ", b"synthetic MLAT", b"synthetic UAT",
           b"no_forward message", b"receiverTime: ", b"utcTime: ", b"DF:  0 addr:", b"DF:  4 addr:", b"DF:  5 addr:", b"DF: 11 AA:", b"DF: 16 addr:", b"DF: 17 AA:",
           b"DF: 18 AA:", b"DF: 20 addr:", b"DF: 21 addr:", b"DF: 24 addr:", b" modeac\n", b" out of range\n", b" reserved\n", b"/1)\n", b" (11)\n",
           b"Comm-B format: ", b"Other Address: ", b"ICAO Address:  ", b"Air/Ground:    ", b"Baro altitude:  ", b"Geom altitude:  ", b"Geom - baro:   ",
           b"  Ground track ", b"  Mag heading ", b"  True heading ", b"  Heading    ", b"  Track/Heading ", b"  unknown heading type ", b"Track rate:    ", b" deg/sec left",
           b" deg/sec right", b"Roll:          ", b" degrees left", b" degrees right", b" degrees \n", b"Groundspeed:   ", b" (v0: ", b" (v2: ", b"IAS:           ",
           b"TAS:           ", b"Mach number:   ", b"Baro rate:     ", b"Geom rate:     ", b"Squawk:        ", b"Ident:         ", b"Category:      ",
           b"CPR type:      Surface", b"CPR type:      Airborne", b"CPR type:      TIS-B", b"CPR odd flag:  odd", b"CPR odd flag:  even", b"CPR decoding:  none",
           b"CPR decoding:  global", b"CPR decoding:  local", b"  NIC:           ", b"  Rc:            ", b"NIC-A:", b"NIC-B:", b"NIC-C:", b"NIC-baro:", b"NACp:", b"NACv:",
           b"GVA:", b"SIL:           ", b"p <= 0.1%", b"p <= 0.001%", b"p <= 0.00001%", b"p > 0.1%", b"SDA:", b"Aircraft Operational Status:", b"ACAS ", b"CDTI ", b"1090IN ",
           b"ARV ", b"TS ", b"TC=", b"UATIN ", b"POA ", b"B2-LOW ", b"L/W=", b"GPS-OFFSET=", b"ACASRA ", b"IDENT ", b"ATC ", b"SAF ", b"Track/heading:      ",
           b"Heading ref dir:    ", b"Selected heading: ", b"FMS selected altitude:", b"MCP selected altitude:  ", b"QNH:  ", b"source:  aircraft altitude",
           b"source:  MCP", b"source:  FMS", b"source:  unknown", b"Nav modes:  ", b"Emergency/priority:", b",DF:,16,bytes:,", b"Clear of Conflict", b"RA:", b"RA multithreat:",
           b"; TIDh: ", b"not below", b"not right", b" Level Off", b" Maintain vertical Speed", b" Monitor vertical Speed", b" NOW", b"; Crossing"]


def main():
    assert du.have_ref_full(), "needs /root/reference and oracle/_ref/full (run __graft_entry__.build())"
    groups, near = du.build_groups()
    out = {"e_near": near}
    with tempfile.TemporaryDirectory() as tmp:
        exe = du.build_ref_harness(tmp)
        hits = np.zeros(len(MARKERS), dtype=np.int64)
        for g, c in groups.items():
            for k, v in c.items():
                out[f"{g}_{k}"] = v
            deferred = np.nonzero(du.classes(c, 0) == du.DEFER)[0]
            assert deferred.tolist() == (near.tolist() if g == "e" else []), (g, deferred)
            for mode, flags in du.MODES.items():
                stream, lens = du.run_ref_harness(exe, c, flags, tmp)
                assert int(lens.sum()) == len(stream) and lens.max() <= du.DUMP_MAX, (g, mode)
                assert ((lens != 0) == (du.classes(c, flags) != du.SKIP)).all(), (g, mode)
                assert du.model_chunks(c, flags) == du.chunks(stream, lens), (g, mode)       # the model equals the harness byte for byte
                out[f"ref_{g}_{mode}"], out[f"len_{g}_{mode}"] = np.frombuffer(stream, dtype=np.uint8), lens.astype(np.int16)
                if mode == "full":
                    for text in du.chunks(stream, lens):
                        hits += [m in text for m in MARKERS]
                print(g, mode, len(c["msgs"]), "cases", len(stream), "bytes, longest", int(lens.max()))
        rare = [(m, int(h)) for m, h in zip(MARKERS, hits) if h < 5]
        assert not rare, rare
    np.savez_compressed(du.GOLDEN, **out)
    size = os.path.getsize(du.GOLDEN)
    print(du.GOLDEN, size, "bytes")
    assert size < 1000000


if __name__ == "__main__":
    main()
