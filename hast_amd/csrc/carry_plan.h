// carry_plan.h -- the accounting of a carried-block feed: carry_feed.h and its sequential model (tests/native/test_carry_plan.cpp).
// Host only.  Two views of room_of(block) bytes.  Block n lies in view n & 1 as [carried bytes | new bytes]: the new bytes always at
// offset `block`, what block n-1 left unframed right in front of them -- so block n+1 is written before anybody knows how much block
// n leaves.  A step frames [block - tail, block + n_new) of its view; what it leaves goes to offset block - left of the OTHER view.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace hast {
namespace carry {

// bytes of a view: carried bytes, a block, a pad for whoever reads a few bytes behind it
inline size_t room_of(size_t block) { return 2 * block + 64; }

struct View {
    int slot;
    size_t off, bytes;             // [off, off + bytes) of view `slot`
};

struct Plan {
    size_t block = 0;
    uint64_t n_submitted = 0, n_done = 0;
    size_t tail = 0;               // bytes carried in front of block n_done's new bytes
    int handed = 0;                // what the caller holds: 0 nothing, 1 a host block, 2 a device block
    size_t n_new[2] = {0, 0};
    bool on_device[2] = {false, false};        // no upload to wait for

    int submit_slot() const { return (int)(n_submitted & 1); }
    int step_slot() const { return (int)(n_done & 1); }
    bool may_hand() const { return n_submitted - n_done < 2; }       // false: two blocks are waiting for their steps
    bool waiting() const { return n_submitted != n_done; }
    bool at_rest() const { return !waiting() && !handed && !tail; }  // no input is on its way through
    size_t new_off() const { return block; }                         // where a block's new bytes go, in view submit_slot()
    bool hand(int what) { return may_hand() && (handed = what); }
    // allow_empty: 0 bytes are a block too (nothing to upload: it counts as on the device)
    bool may_submit(size_t n, bool allow_empty) const { return may_hand() && handed && n <= block && (n > 0 || allow_empty); }
    bool submitted(size_t n) {     // true: the bytes lie in the staging block and have to be uploaded
        const int slot = submit_slot();
        on_device[slot] = handed == 2 || n == 0;
        n_new[slot] = n;
        handed = 0;
        ++n_submitted;
        return !on_device[slot];
    }
    View view() const { return View{step_slot(), block - tail, tail + n_new[step_slot()]}; }       // what the next step frames
    View tail_view() const { return View{step_slot(), block - tail, tail}; }                       // the carried bytes alone
    bool fits(size_t left) const { return left <= block; }           // of what a step leaves
    size_t left_off(size_t left) const { return block - left; }      // where it goes, in the view that is not the step's
    void done() { ++n_done; }      // the step's block is not looked at again
    void drop_tail() { tail = 0; }
};

}  // namespace carry
}  // namespace hast
