// The claim protocol of the device-side barcode dictionary (hast_amd/csrc/name_claim.h: the code k_fq_name_claim steps), model-checked:
// the SAME step function, instantiated with a memory policy that hands control back to a scheduler at every operation on shared
// memory, and every interleaving of the lanes' operations enumerated (sequential consistency; the argument that the device's
// acquire/release orderings give the protocol what it needs of that is in the header).
//
// How a lane is suspended in the middle of straight-line code: by replay.  A lane's state is what it held at the start of its current
// step plus the values its operations have returned since; to advance it by ONE operation the step is run again from its start, the
// logged operations answered from the log, the next one performed for real, and whatever comes after it answered with dummies and
// thrown away (every access goes through the policy, so such a run touches nothing).
//
// States are hashed: the number of complete schedules is the number of paths through a DAG, summed by memo.  The only cycles a lane
// can make are turns that change nothing -- it found its slot in state 1 and will look again: those transitions are CUT, and the
// driver checks that each cut is exactly that (one operation, load_state, answer 1, nothing changed), that no other cycle exists, and
// that every state with a busy lane has a way on that is not a cut (nobody waits for ever).
//
// At the end of every complete schedule: one answer per text; the ids handed out are 0 .. min(limit, distinct texts) - 1, each to one
// text; every ready slot's key, id and text_of_id agree; no slot is left in state 1.
//
// `r6`: the order shipped up to round 10 (counter looked at after the state, no second look), kept HERE ONLY so that the checker
// proves itself: it must find violations in r6 and none in the header.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../hast_amd/csrc/name_claim.h"

using hast::kNameUnknown;
using hast::NameClaimLane;

namespace {

constexpr int kMaxSlots = 4, kMaxIds = 4, kMaxLanes = 5, kMaxLog = 10;

struct World {
    uint32_t state[kMaxSlots], key[kMaxSlots], id[kMaxSlots];
    uint32_t counter;
    uint32_t text_of_id[kMaxIds];
};
enum Op : uint8_t { kNone, kLoadState, kLoadCounter, kCas, kAdd, kStoreState, kWriteEntry, kWriteText, kKeyEquals, kLoadId };

struct SchedMem {
    World *w;
    const uint32_t *log;
    int n_log, pos = 0;
    int n_slots = 0, n_ids = 0;
    bool did = false, beyond = false;      // the one real operation of this run has been done; an operation after it was asked for
    Op op = kNone;
    uint32_t result = 0;
    template <class F> uint32_t run(Op kind, F f) {
        if (pos < n_log) return log[pos++];
        if (!did) { did = true; pos++; op = kind; result = f(); return result; }
        beyond = true;
        return 0;
    }
    void slot(uint32_t e) const { if (e >= (uint32_t)n_slots) { fprintf(stderr, "slot %u out of range\n", e); abort(); } }
    uint32_t load_state(uint32_t e) { return run(kLoadState, [&] { slot(e); return w->state[e]; }); }
    uint32_t load_counter() { return run(kLoadCounter, [&] { return w->counter; }); }
    uint32_t cas_state_0_1(uint32_t e) { return run(kCas, [&] { slot(e); const uint32_t old = w->state[e]; if (old == 0) w->state[e] = 1; return old; }); }
    uint32_t add_counter() { return run(kAdd, [&] { return w->counter++; }); }
    void store_state(uint32_t e, uint32_t v) {
        run(kStoreState, [&] {
            slot(e);
            if (w->state[e] != 1) { fprintf(stderr, "store to a slot that is not this lane's\n"); abort(); }
            w->state[e] = v;
            return 0u;
        });
    }
    void write_entry(uint32_t e, const uint32_t k[4], uint32_t id) {
        run(kWriteEntry, [&] {
            slot(e);
            if (w->state[e] != 1) { fprintf(stderr, "entry written outside state 1\n"); abort(); }
            w->key[e] = k[0]; w->id[e] = id;
            return 0u;
        });
    }
    void write_text(uint32_t id, const uint32_t k[4]) {
        run(kWriteText, [&] {
            if (id >= (uint32_t)n_ids || w->text_of_id[id]) { fprintf(stderr, "text_of_id[%u]: out of range or written twice\n", id); abort(); }
            w->text_of_id[id] = k[0];
            return 0u;
        });
    }
    bool key_equals(uint32_t e, const uint32_t k[4]) {
        return run(kKeyEquals, [&] { slot(e); if (w->state[e] != 2) { fprintf(stderr, "key read of a slot that is not ready\n"); abort(); } return (uint32_t)(w->key[e] == k[0]); }) != 0;
    }
    uint32_t load_id(uint32_t e) { return run(kLoadId, [&] { slot(e); return w->id[e]; }); }
};

// the order of rounds 6 to 10: the counter is looked at once, after the state, and a lane that finds it at the limit gives up at once
template <class Mem> void name_claim_step_r6(Mem &m, NameClaimLane &l, uint32_t mask, uint32_t limit) {
    const uint32_t e = l.at;
    uint32_t st = m.load_state(e);
    if (st == 0) {
        if (m.load_counter() >= limit) { l.busy = false; return; }
        st = m.cas_state_0_1(e);
        if (st == 0) {
            const uint32_t got = m.add_counter();
            if (got >= limit) m.store_state(e, 0u);
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
    if (st == 2) {
        if (m.key_equals(e, l.k)) { l.id = m.load_id(e); l.busy = false; }
        else {
            l.at = (l.at + 1) & mask;
            if (++l.probes > mask) l.busy = false;
        }
    }
}

struct LaneSpec { uint32_t text, home, after; };      // text code (> 0), home slot, lanes (bit mask) that must have finished first: an earlier kernel of its stream
struct Config {
    const char *name;
    int n_slots, limit;
    std::vector<LaneSpec> lanes;
};
struct LaneState {
    uint32_t at, probes, id;
    uint32_t busy, n_log;
    uint32_t log[kMaxLog];
};
struct State {
    World w;
    LaneState lane[kMaxLanes];
};
struct Count { unsigned __int128 all = 0, bad = 0; };
struct Stats { uint64_t states = 0, cuts = 0, terminals = 0, bad_terminals = 0; };

std::string dec(unsigned __int128 v) {
    std::string s;
    do { s.insert(s.begin(), (char)('0' + (int)(v % 10))); v /= 10; } while (v);
    return s;
}

template <bool kShipped> struct Checker {
    const Config &cfg;
    std::unordered_map<std::string, std::pair<Count, bool>> memo;      // (result, done): !done = on the path being walked
    Stats st;
    std::string first_bad;
    explicit Checker(const Config &c) : cfg(c) {}

    static std::string key_of(const State &s) { return std::string(reinterpret_cast<const char *>(&s), sizeof(State)); }

    // lane i by one operation; false: the operation was a cut (nothing changed)
    bool advance(const State &from, int i, State &to) {
        to = from;
        LaneState &ls = to.lane[i];
        NameClaimLane l;
        const uint32_t k[4] = {cfg.lanes[(size_t)i].text, 0, 0, 0};
        hast::name_claim_begin(l, k, 0);
        l.at = ls.at; l.probes = ls.probes; l.id = ls.id; l.busy = true;
        SchedMem m{&to.w, ls.log, (int)ls.n_log};
        m.n_slots = cfg.n_slots;
        m.n_ids = cfg.limit;
        if (kShipped) hast::name_claim_step(m, l, (uint32_t)cfg.n_slots - 1, (uint32_t)cfg.limit);
        else name_claim_step_r6(m, l, (uint32_t)cfg.n_slots - 1, (uint32_t)cfg.limit);
        if (!m.did) { fprintf(stderr, "%s: a step without an operation\n", cfg.name); abort(); }
        if (m.beyond) {                                 // the step goes on: keep what it held at its start, and the longer log
            if (ls.n_log >= kMaxLog) { fprintf(stderr, "log overflow\n"); abort(); }
            ls.log[ls.n_log++] = m.result;
        } else {                                        // the step is through
            ls.at = l.at; ls.probes = l.probes; ls.id = l.id; ls.busy = l.busy;
            ls.n_log = 0;
            memset(ls.log, 0, sizeof(ls.log));
        }
        if (memcmp(&from, &to, sizeof(State)) == 0) {
            // nothing moved: the only thing this may be is a lane that found its slot being written
            if (!(m.op == kLoadState && m.result == 1 && from.lane[i].n_log == 0)) {
                fprintf(stderr, "%s: a cut that is not a spin on a state-1 slot (op %d -> %u)\n", cfg.name, (int)m.op, m.result);
                abort();
            }
            st.cuts++;
            return false;
        }
        return true;
    }

    bool terminal_ok(const State &s, std::string &why) {
        const int n = (int)cfg.lanes.size();
        uint32_t id_of_text[16];
        bool seen[16] = {false};
        int distinct = 0;
        for (int i = 0; i < n; i++) {
            const uint32_t t = cfg.lanes[(size_t)i].text;
            if (!seen[t]) { seen[t] = true; id_of_text[t] = s.lane[i].id; distinct++; }
            else if (id_of_text[t] != s.lane[i].id) { why = "two answers for one text"; return false; }
        }
        const int want = distinct < cfg.limit ? distinct : cfg.limit;
        uint32_t text_of[kMaxIds] = {0};
        int handed = 0;
        for (uint32_t t = 1; t < 16; t++) {
            if (!seen[t] || id_of_text[t] == kNameUnknown) continue;
            if (id_of_text[t] >= (uint32_t)want || text_of[id_of_text[t]]) { why = "ids not 0 .. min(limit, texts) - 1, one text each"; return false; }
            text_of[id_of_text[t]] = t;
            handed++;
        }
        if (handed != want) { why = "fewer ids handed out than there are"; return false; }
        int ready = 0;
        for (int e = 0; e < cfg.n_slots; e++) {
            if (s.w.state[e] == 1) { why = "a slot left in state 1"; return false; }
            if (s.w.state[e] != 2) continue;
            ready++;
            const uint32_t id = s.w.id[e];
            if (id >= (uint32_t)want || text_of[id] != s.w.key[e] || s.w.text_of_id[id] != s.w.key[e]) { why = "slot, id and text_of_id disagree"; return false; }
        }
        if (ready != want) { why = "ready slots != ids handed out"; return false; }
        if (s.w.counter < (uint32_t)want) { why = "counter below the ids handed out"; return false; }
        return true;
    }

    Count walk(const State &s) {
        const std::string key = key_of(s);
        auto it = memo.find(key);
        if (it != memo.end()) {
            if (!it->second.second) { fprintf(stderr, "%s: a cycle that is not a spin\n", cfg.name); abort(); }
            return it->second.first;
        }
        memo.emplace(key, std::make_pair(Count(), false));
        st.states++;
        const int n = (int)cfg.lanes.size();
        uint32_t finished = 0;
        for (int i = 0; i < n; i++)
            if (!s.lane[i].busy) finished |= 1u << i;
        Count c;
        if (finished == (1u << n) - 1) {
            std::string why;
            c.all = 1;
            st.terminals++;
            if (!terminal_ok(s, why)) {
                c.bad = 1;
                st.bad_terminals++;
                if (first_bad.empty()) first_bad = why;
            }
        } else {
            int ways = 0;
            for (int i = 0; i < n; i++) {
                if (!s.lane[i].busy || (cfg.lanes[(size_t)i].after & ~finished)) continue;
                State to;
                if (!advance(s, i, to)) continue;
                ways++;
                const Count sub = walk(to);
                c.all += sub.all;
                c.bad += sub.bad;
            }
            if (!ways) { fprintf(stderr, "%s: a state in which every lane only waits\n", cfg.name); abort(); }
        }
        memo[key] = std::make_pair(c, true);
        return c;
    }

    Count run() {
        State s;
        memset(&s, 0, sizeof(s));
        for (size_t i = 0; i < cfg.lanes.size(); i++) {
            s.lane[i].at = cfg.lanes[i].home;
            s.lane[i].id = kNameUnknown;
            s.lane[i].busy = 1;
        }
        return walk(s);
    }
};

}  // namespace

int main() {
    const uint32_t T = 1, U = 2, V = 3;
    const std::vector<Config> configs = {
        {"TT_limit1", 2, 1, {{T, 0, 0}, {T, 0, 0}}},
        {"TTU_limit1_same_home", 4, 1, {{T, 0, 0}, {T, 0, 0}, {U, 0, 0}}},
        {"TTU_limit1_other_home", 4, 1, {{T, 0, 0}, {T, 0, 0}, {U, 2, 0}}},
        {"TTU_limit2", 4, 2, {{T, 0, 0}, {T, 0, 0}, {U, 1, 0}}},
        {"TTU_limit2_same_home", 4, 2, {{T, 0, 0}, {T, 0, 0}, {U, 0, 0}}},
        {"TUV_limit2", 4, 2, {{T, 0, 0}, {U, 0, 0}, {V, 1, 0}}},
        {"TTUU_limit1", 4, 1, {{T, 0, 0}, {T, 0, 0}, {U, 1, 0}, {U, 1, 0}}},
        {"TTUU_limit1_same_home", 4, 1, {{T, 0, 0}, {T, 0, 0}, {U, 0, 0}, {U, 0, 0}}},
        {"TTUU_limit2", 4, 2, {{T, 0, 0}, {T, 0, 0}, {U, 1, 0}, {U, 1, 0}}},
        {"TTUU_limit2_same_home", 4, 2, {{T, 0, 0}, {T, 0, 0}, {U, 0, 0}, {U, 0, 0}}},
        // probing wraps: everybody is homed on the last slot
        {"wrap_TTU_2slots_limit1", 2, 1, {{T, 1, 0}, {T, 1, 0}, {U, 1, 0}}},
        {"wrap_TUV_4slots_limit2", 4, 2, {{T, 3, 0}, {U, 3, 0}, {V, 3, 0}}},
        {"wrap_TTUU_4slots_limit2", 4, 2, {{T, 3, 0}, {T, 3, 0}, {U, 3, 0}, {U, 3, 0}}},
        // two kernels of one stream (lanes 2, 3 start when 0 and 1 are through) and one of another stream, on one table
        {"two_kernels_limit1", 4, 1, {{T, 0, 0}, {U, 1, 0}, {T, 0, 3}, {U, 1, 3}, {T, 0, 0}}},
        {"two_kernels_limit2", 4, 2, {{T, 0, 0}, {U, 0, 0}, {V, 1, 3}, {T, 0, 3}, {V, 1, 0}}},
    };
    unsigned __int128 shipped_all = 0, r6_all = 0, r6_bad = 0;
    int r6_configs_bad = 0;
    for (const Config &c : configs) {
        Checker<true> a(c);
        const Count ca = a.run();
        Checker<false> b(c);
        const Count cb = b.run();
        printf("%-28s shipped: %s schedules, %s bad, %llu states, %llu cuts | r6: %s schedules, %s bad%s%s\n", c.name, dec(ca.all).c_str(), dec(ca.bad).c_str(),
               (unsigned long long)a.st.states, (unsigned long long)a.st.cuts, dec(cb.all).c_str(), dec(cb.bad).c_str(), cb.bad ? ": " : "", b.first_bad.c_str());
        if (ca.bad) {
            fprintf(stderr, "FAIL %s: the shipped protocol breaks an invariant in %s of %s schedules: %s\n", c.name, dec(ca.bad).c_str(), dec(ca.all).c_str(), a.first_bad.c_str());
            return 1;
        }
        if (!a.st.cuts) { fprintf(stderr, "FAIL %s: no lane ever met a slot being written -- the configuration explores nothing\n", c.name); return 1; }
        shipped_all += ca.all;
        r6_all += cb.all;
        r6_bad += cb.bad;
        r6_configs_bad += cb.bad != 0;
    }
    // the checker proves itself: the old order must be caught, in the smallest configuration and in most of the others
    {
        Checker<false> b(configs[0]);
        const Count cb = b.run();
        if (!cb.bad || b.first_bad != "two answers for one text") { fprintf(stderr, "FAIL: the checker finds nothing in the round-6 order at (T, T), limit 1\n"); return 1; }
    }
    if (r6_configs_bad < (int)configs.size() / 2) { fprintf(stderr, "FAIL: the round-6 order is caught in only %d configurations\n", r6_configs_bad); return 1; }
    printf("ok shipped %s schedules 0 bad; r6 %s schedules %s bad in %d of %zu configurations\n", dec(shipped_all).c_str(), dec(r6_all).c_str(), dec(r6_bad).c_str(),
           r6_configs_bad, configs.size());
    return 0;
}
