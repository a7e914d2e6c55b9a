"""Golden vectors for the beast encoder's --net-verbatim path, by the WHOLE reference program like make_beast_golden.py (whose
functions this imports): the same two seeded captures with `--net-verbatim --net-receiver-id` added to `--dump-beast`.  The flag
sends mm->verbatim (the frame as sliced) instead of mm->msg and lifts both forwarding tests (net_io.c:1662, 5846, 5869), so the
stream holds a frame for every accepted message.  --net-receiver-id adds nothing to it: an SDR message's receiverId is 0, and so is
a fresh writer's lastReceiverId (net_io.c:343, 1669) — which is what the goldens pin about the prefix rule.
Only runs in the development container (needs the reference's sources).

    python tests/golden/make_beast_verbatim_golden.py        -> tests/golden/beast_verbatim_<name>.bin"""
import os
import subprocess

import make_beast_golden as g

OPTS = ["--net-verbatim", "--net-receiver-id"]


def main():
    """Eight runs per capture, the shortest of the distinct streams kept (the start-up race: make_beast_golden.main)."""
    if not os.path.exists(g.FULL):
        subprocess.run(["make", "-s", "-C", os.path.join(g.ROOT, "oracle"), "full"], check=True)
    for name, kw, opts in g.CASES:
        iq = g.helpers.synth(**kw)
        runs = [g.reference_frames(iq, opts + OPTS) for _ in range(8)]
        variants = sorted(set(runs), key=len)
        open(os.path.join(g.HERE, f"beast_verbatim_{name}.bin"), "wb").write(variants[0])
        print(name, kw, opts + OPTS, len(variants[0]), "bytes;", len(variants), "distinct stream(s) in 8 runs", [len(v) for v in variants])


if __name__ == "__main__":
    main()
