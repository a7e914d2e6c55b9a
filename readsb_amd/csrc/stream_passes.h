// stream_passes.h — private to the library and its check programs: how a host form cuts a stream into passes.  No HIP and nothing of a
// format in this file: tests/host_stub/stream_passes_check.cpp drives it with a format made up on the spot.
#pragma once
#include <cstdint>

namespace mgpu {

// The stream [0, nbytes) in stretches of `pass` bytes (0: the whole stream in one).  A stretch is consumed up to the last unit — a
// line, a frame, a record — that ends inside it; the next stretch starts there, so the remainder is carried, and the sum is exactly
// the result of one call over the whole stream.  A stretch that consumes nothing, stops nothing and does not end the stream holds a
// unit longer than itself: it is undone and repeated twice as long.
//   run(at, nb, final, all, n) -> 0 or an error, which ends the passes: the stretch [at, at + nb) — final: it reaches the end of the
//     stream — continuing what `all` has counted so far; its results stored behind all's in the caller's arrays as far as they reach,
//     its counts in n (a fresh Counts; n.consumed relative to at).
//   undo(): the state run() moved on (a filter) as before the last run.
//   Counts: consumed; stopped(): the stretch met something that ends the call where it stands; add(n): n's counts into the sum
//     (consumed is the driver's, and counts n already).
//   tail_pass: a stretch that reaches the end of the stream and leaves a tail is followed by one more over that tail alone (the line
//     formats, whose unterminated last line is looked at once more); otherwise the stretch that ends the stream ends the passes.
template <class Counts, class Run, class Undo>
int stream_passes(uint64_t nbytes, uint64_t pass, bool tail_pass, Counts &all, Run run, Undo undo) {
    if (pass == 0 || pass > nbytes) pass = nbytes;
    for (uint64_t at = 0; at < nbytes;) {
        const uint64_t nb = pass < nbytes - at ? pass : nbytes - at;
        const bool final = at + nb >= nbytes;
        Counts n;
        if (int rc = run(at, nb, final, all, n)) return rc;
        if (n.consumed == 0 && !n.stopped() && !final) {
            undo();
            pass = pass > nbytes / 2 ? nbytes : 2 * pass;
            continue;
        }
        at += n.consumed;
        all.consumed = at;
        all.add(n);
        if (n.stopped() || n.consumed == 0 || (final && !tail_pass)) break;
    }
    return 0;
}

}  // namespace mgpu
