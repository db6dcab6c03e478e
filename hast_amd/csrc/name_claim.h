// name_claim.h -- the claim protocol of the device-side barcode DICTIONARY, once: the per-lane state machine k_fq_name_claim
// (fq_kernels.hip) steps in its wave-uniform loop, and that tests/native/test_name_claim.cpp steps under a scheduler which
// enumerates every interleaving of the lanes' memory operations.  Every access to memory that lanes share goes through a policy
// type `Mem`; the kernel's policy is the device atomics, the test's yields to its scheduler at each of them.
//
// The table: open addressing over NameEntry, state 0 empty -> 1 being written -> 2 ready (final), or 1 -> 0 when the writer found
// every id gone.  Ids come from ONE counter, `limit` of them; a text the dictionary cannot number is left to the host ("unknown").
//
// What must hold, whatever the interleaving: ONE ANSWER PER TEXT -- every lane that asks for a text gets the same id, or every one
// is told "unknown".  The host numbers what is unknown in a range of its own, and the output has one row per id: a text with an id
// from both sides would be printed twice with its counts split.
//
// The order that breaks it (shipped up to round 10): look at the slot, see it empty, THEN look at the counter, see it at the
// limit, give up.  Between the two looks another lane with the same text may claim that very slot, take the last id and publish.
// The order here: a lane that sees the counter at the limit looks at the slot AGAIN and gives up only if it is still empty.
//   Why that suffices.  Let A hold an id below the limit for text T, and B, same text, have seen the counter at or above the limit.
//   (1) All `limit` additions that returned an id precede B's look in the counter's modification order, A's among them.
//   (2) A claimed its slot s' (compare-and-swap 0 -> 1) BEFORE its addition, and keeps it: only a lane that got no id gives a slot
//       back.  Both walk the same probe sequence and pass only READY entries of other texts, which never change again.
//   (3) The addition is a RELEASE, B's look at the counter an ACQUIRE (both at agent scope: every context of one GPU that shares the
//       table is covered).  So what A did and saw before its addition -- its claim of s', and the ready entries it passed -- happens
//       before whatever B reads after its look at the counter.
//   (4) B's second look at its slot s therefore sees: s' == s: A's claim or A's entry (state 1 or 2, never 0 again) -> B waits or
//       takes A's id.  s' behind s: A passed s as a ready entry of another text -> B sees it ready and walks on.  s' in front of s: B
//       passed s' as a ready entry of another text, which it stays for good, so A could never have claimed it.
//   The checker explores the protocol under sequential consistency; (3) is what makes the device behave like that where it matters.
#pragma once
#include <stdint.h>

#ifndef HAST_HD
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HAST_HD __host__ __device__ __forceinline__
#else
#define HAST_HD inline
#endif
#endif

namespace hast {

// Device-side table barcode text -> dense id: 32-byte entries, open addressing.  key = the 16-byte text record the framer makes
// (length byte + up to 15 bytes).
struct NameEntry {
    uint32_t key[4];
    uint32_t id;
    uint32_t state;            // 0 empty, 1 being written, 2 ready
    uint32_t pad[2];
};
constexpr uint32_t kNameUnknown = 0xFFFFFFFFu;

HAST_HD uint32_t name_hash(const uint32_t k[4]) {
    uint32_t h = k[0] * 0x9E3779B1u;
    h = (h ^ (h >> 15) ^ k[1]) * 0x85EBCA6Bu;
    h = (h ^ (h >> 13) ^ k[2]) * 0xC2B2AE35u;
    h = (h ^ (h >> 16) ^ k[3]) * 0x27D4EB2Fu;
    return h ^ (h >> 15);
}

struct NameClaimLane {         // what a lane keeps between two steps
    uint32_t k[4];             // its text record
    uint32_t at, probes;       // the slot it looks at, slots passed
    uint32_t id;               // the answer once !busy
    bool busy;
};
HAST_HD void name_claim_begin(NameClaimLane &l, const uint32_t k[4], uint32_t home) {
    l.k[0] = k[0]; l.k[1] = k[1]; l.k[2] = k[2]; l.k[3] = k[3];
    l.at = home;
    l.probes = 0;
    l.id = kNameUnknown;
    l.busy = true;
}

// What `Mem` provides (e = slot index):
//   uint32_t load_state(e)                  acquire
//   uint32_t load_counter()                 acquire
//   uint32_t cas_state_0_1(e)               the state found (0: claimed)
//   uint32_t add_counter()                  fetch-add 1, release; the value before
//   void     store_state(e, v)              release (2: publish, 0: give the slot back)
//   void     write_entry(e, k, id)          plain: the slot is this lane's while its state is 1
//   void     write_text(id, k)              plain: text_of_id[id], nobody else's
//   bool     key_equals(e, k), uint32_t load_id(e)      plain, of an entry seen ready
// One step = one turn of the kernel's loop for a busy lane.  A lane that finds its slot being written changes nothing and looks
// again at its next step.
template <class Mem>
HAST_HD void name_claim_step(Mem &m, NameClaimLane &l, uint32_t mask, uint32_t limit) {
    const uint32_t e = l.at;
    uint32_t st = m.load_state(e);
    if (st == 0) {
        if (m.load_counter() >= limit) {
            // every id is out -- but one of them may have gone to this text, into this slot, since the look above
            st = m.load_state(e);
            if (st == 0) { l.busy = false; return; }
        } else {
            st = m.cas_state_0_1(e);
            if (st == 0) {                                        // claimed
                const uint32_t got = m.add_counter();
                if (got >= limit) m.store_state(e, 0u);           // (the last ids went while this lane claimed: give the slot back)
                else {
                    m.write_entry(e, l.k, got);
                    m.write_text(got, l.k);
                    m.store_state(e, 2u);
                    l.id = got;
                }
                l.busy = false;
                return;
            }
        }
    }
    if (st == 2) {                                                // a ready entry: this text, or another one's -> next slot
        if (m.key_equals(e, l.k)) { l.id = m.load_id(e); l.busy = false; }
        else {
            l.at = (l.at + 1) & mask;
            if (++l.probes > mask) l.busy = false;
        }
    }
    // st == 1: being written by another lane (of this wave, or of another stream's kernel) -- look again at the next step
}

}  // namespace hast
