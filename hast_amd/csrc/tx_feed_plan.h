// tx_feed_plan.h -- the reading rule of fake_10x's loop, stated once, for whoever cannot look at the bytes: the paired feed of the
// device route (tx_feed.cpp: the bytes lie in HBM) and its sequential model (tests/native/test_tx_feed_plan.cpp).  Host only.
//
// fake_10x_main.cpp decides per step and side from the bytes it holds (have[]): does the side read a block, and which mode has the
// step.  Both follow from three numbers a step of mode 0 leaves behind -- the newlines of what it was given (hast_tx_result.lines),
// the pairs it converted and the bytes it consumed:
//   * what a side carries into the next step holds a whole record (four newlines) iff lines - 4 * pairs >= 4;
//   * a side holds a whole record iff lines >= 4, so hast_tx_step_mode's answer over what a step was GIVEN is known once the step's
//     lines are.  A step of mode 0 over inputs whose mode is 1 or 2 converts nothing (one side has no whole record, so there is no
//     whole pair): it may be run before its mode is known, and whoever then reads mode 1 or 2 takes the bytes to the host untouched.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace hast {
namespace txfeed {

// bytes a side may hold in one step: what fake_10x gives hast_tx_create (a step holds what the step before left and a block: two
// blocks in all but odd cases; at least 1 MB, so that records far larger than a small block still fit; at most what 32-bit offsets
// allow)
inline size_t room_of(size_t block) {
    const size_t two = 2 * block + 4096, least = (size_t)1 << 20, most = (size_t)128 << 20;
    return two < least ? least : two > most ? most : two;
}

// what a side carries out of a step that was given `lines` newlines and converted `pairs` pairs: a whole record?
inline bool carries_record(uint32_t lines, uint64_t pairs) { return (uint64_t)lines - 4 * pairs >= 4; }

// the reading rule: a side that has been read to its end, or that holds more than a block with a whole record in it, reads nothing
// (the other side has to catch up)
inline bool wants(bool eof, size_t held, bool holds_record, size_t block) { return !eof && !(held > block && holds_record); }

// a side that wants to read needs held + block bytes of room; false: a record longer than the buffers
inline bool fits(size_t held, size_t block, size_t room) { return held <= room && block <= room - held; }

// hast_tx_step_mode over inputs of lines1 / lines2 newlines: 0 the whole pairs, 2 read 2 has ended, 1 the inputs end here
inline int mode_of(bool eof1, bool eof2, uint32_t lines1, uint32_t lines2) {
    const bool rec1 = lines1 >= 4, rec2 = lines2 >= 4;
    if (eof1 && !rec1 && (eof2 || rec2)) return 1;
    if (eof2 && !rec2) return 2;
    return 0;
}

// One side of the feed between two steps, and the whole rule over it.
struct Side {
    size_t carry = 0;              // bytes the step before left
    size_t fresh = 0;              // bytes read for the next step, behind them
    bool record = false;           // the carried bytes hold a whole record
    bool eof = false;              // read to its end: a read came back short of a block
    bool read = false;             // has read for the next step
    bool wants(size_t block) const { return !read && txfeed::wants(eof, carry, record, block); }
    void submitted(size_t n, size_t block) {
        fresh = n;
        read = true;
        if (n < block) eof = true;
    }
    size_t held() const { return carry + fresh; }
    void stepped(uint32_t lines, uint64_t pairs, uint64_t consumed) {
        carry = held() - (size_t)consumed;
        fresh = 0;
        read = false;
        record = carries_record(lines, pairs);
    }
};

}  // namespace txfeed
}  // namespace hast
