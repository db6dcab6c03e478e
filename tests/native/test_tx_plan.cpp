// test_tx_plan.cpp -- the device step of the stLFR -> 10x conversion as a sequential model: the steps of tx_kernels.hip as plain
// loops over the shared functions of hast_amd/csrc/tx_plan.h (newline index, pairs and consumed bytes, keys and table, the scan of
// the kept pairs, the plans and sizes, the verdict, the emit through rec1_byte / rec2_byte).  Nothing of tx::pair_host is used by
// the model; pair_host is what it is compared with.
//   test_tx_plan -b BLOCK READ1 READ2 MAP OUT1 OUT2     feeds the model the way the fake_10x program feeds the device: every step of
//       mode 0 over a device_ok map goes through the model AND through pair_host(final = 0), and every result field, the state and
//       every byte must be equal; the steps of mode 1 and 2 (and every step of a map that is not device_ok) are pair_host's.
//       A step whose outputs are larger than the program's room (2 x the bytes given + 4 KB) must be refused whole, and is
//       compared with room that fits exactly.  stdout is the script's; stderr gets one line about the map and the steps per route.
//   test_tx_plan --table MAP...     every key of every map is found in its table with its value, slots that hold nothing are empty
//   test_tx_plan --rules            key_record on the rows of the key-rule table; absent keys, header keys of 15 and 16 bytes at load 0.5
// Exit 0: all equal; 1: a difference (said on stderr); 2: usage or a file that cannot be read.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../hast_amd/csrc/tx_host.h"

using namespace hast;

static bool slurp(const char *path, std::vector<uint8_t> &out) {
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    uint8_t buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + n);
    fclose(f);
    return true;
}

struct StepResult {            // hast_tx_result, and whether the step was refused for its room
    uint64_t consumed[2] = {0, 0}, pairs = 0, used = 0, out_bytes[2] = {0, 0};
    uint32_t lines[2] = {0, 0};
    bool refused = false;
};

// One step of the device, kernel by kernel, over exact-size buffers.  `used` = N so far; out[] get the bytes unless refused.
static StepResult device_model(const std::vector<tx::TableSlot> &table, const std::vector<uint8_t> in[2], uint64_t used, uint64_t cap0, uint64_t cap1,
                               std::string out[2]) {
    StepResult r;
    // k_nl_count / k_tx_scan / k_nl_index: the newline index of both sides
    std::vector<uint32_t> nl[2];
    for (int s = 0; s < 2; ++s) {
        for (size_t i = 0; i < in[s].size(); ++i)
            if (in[s][i] == '\n') nl[s].push_back((uint32_t)i);
        r.lines[s] = (uint32_t)nl[s].size();
        nl[s].shrink_to_fit();                                   // (exact size: an index past the last newline is the sanitizer's to see)
    }
    const uint32_t m = tx::pairs_of(r.lines[0], r.lines[1]);
    r.pairs = m;
    for (int s = 0; s < 2; ++s) r.consumed[s] = tx::consumed_of(nl[s].data(), m);
    // k_tx_keys
    std::vector<uint32_t> slot(m);
    for (uint32_t i = 0; i < m; ++i) {
        uint64_t lo, hi;
        uint32_t key[4];
        tx::header_of(nl[0].data(), i, &lo, &hi);
        slot[i] = tx::key_record(in[0].data(), lo, hi, key) ? tx::table_find(table.data(), (uint32_t)table.size(), key) : tx::kNoSlot;
    }
    // k_tx_scan_kept / k_tx_sizes / k_tx_scan_out: rank, N, plan, where every record goes
    std::vector<uint32_t> rank(m), dst[2];
    dst[0].resize(m);
    dst[1].resize(m);
    uint32_t kept_so_far = 0, at[2] = {0, 0};
    for (uint32_t i = 0; i < m; ++i) {
        rank[i] = kept_so_far;
        const bool kept = slot[i] != tx::kNoSlot;
        dst[0][i] = at[0];
        dst[1][i] = at[1];
        if (kept) {
            const tx::Plan p = tx::plan_pair(nl[0].data(), nl[1].data(), i, true, used + 1 + rank[i], table[slot[i]].v);
            at[0] += p.rec1_len;
            at[1] += p.rec2_len;
            ++kept_so_far;
        }
    }
    r.used = kept_so_far;
    r.out_bytes[0] = at[0];
    r.out_bytes[1] = at[1];
    r.refused = at[0] > cap0 || at[1] > cap1;
    if (r.refused) return r;
    // k_tx_copy
    out[0].assign(at[0], '\0');
    out[1].assign(at[1], '\0');
    for (uint32_t i = 0; i < m; ++i) {
        if (slot[i] == tx::kNoSlot) continue;
        const tx::TableSlot &t = table[slot[i]];
        const uint64_t n = used + 1 + rank[i];
        const tx::Plan p = tx::plan_pair(nl[0].data(), nl[1].data(), i, true, n, t.v);
        for (uint32_t b = 0; b < p.rec1_len; ++b) out[0][dst[0][i] + b] = (char)tx::rec1_byte(p, in[0].data(), n, t.value, t.v, b);
        for (uint32_t b = 0; b < p.rec2_len; ++b) out[1][dst[1][i] + b] = (char)tx::rec2_byte(p, in[1].data(), n, b);
    }
    return r;
}

static int differ(const char *what, unsigned long long step, unsigned long long got, unsigned long long want) {
    fprintf(stderr, "step %llu: %s: the model has %llu, pair_host %llu\n", step, what, got, want);
    return 1;
}

static int run_blocks(size_t block, char **argv) {
    std::vector<uint8_t> in[2], map_text;
    if (!slurp(argv[0], in[0]) || !slurp(argv[1], in[1]) || !slurp(argv[2], map_text)) return 2;
    tx::Map map;
    tx::map_parse(map_text.data(), map_text.size(), map);
    std::vector<tx::TableSlot> table;
    if (map.device_ok) tx::table_build(map, table);
    fprintf(stderr, "map: n_keys=%zu device_ok=%d reason=%s\n", map.kv.size(), map.device_ok ? 1 : 0, map.reason.c_str());
    printf("Merge stLFR reads into 10X format !\n read1 :  %s \n. read2 : %s \n map file : %s\n", argv[0], argv[1], argv[2]);
    FILE *out[2] = {fopen(argv[3], "wb"), fopen(argv[4], "wb")};
    if (!out[0] || !out[1]) return 2;
    tx::State st;
    std::vector<uint8_t> have[2];
    size_t at[2] = {0, 0};
    uint64_t steps = 0, on_model = 0, refused = 0, room = 0;
    for (bool final = false; !final;) {
        for (int s = 0; s < 2; ++s) {
            const size_t take = std::min(block, in[s].size() - at[s]);
            have[s].insert(have[s].end(), in[s].begin() + at[s], in[s].begin() + at[s] + take);
            at[s] += take;
        }
        std::vector<uint8_t> ex[2] = {have[0], have[1]};                   // exact-size copies: no slack behind the last byte
        ex[0].shrink_to_fit();
        ex[1].shrink_to_fit();
        const int mode = tx::step_mode(at[0] == in[0].size(), at[1] == in[1].size(), ex[0].data(), ex[0].size(), ex[1].data(), ex[1].size());
        final = mode == tx::kFinal;
        std::string o[2], log;
        size_t c[2];
        const tx::State before = st;
        tx::pair_host(map, ex[0].data(), ex[0].size(), ex[1].data(), ex[1].size(), mode, st, o[0], o[1], &c[0], &c[1]);
        if (mode == tx::kNotFinal && map.device_ok) {
            // the program's room: twice the bytes given and 4 KB; and one byte short of what is needed, which must be refused whole
            std::string d[2];
            StepResult r = device_model(table, ex, before.used, 2 * ex[0].size() + 4096, 2 * ex[1].size() + 4096, d);
            ++on_model;
            if (r.refused) {                                               // short records can grow past that room: the program then takes the host's
                if (o[0].size() <= 2 * ex[0].size() + 4096 && o[1].size() <= 2 * ex[1].size() + 4096) return differ("refused with the program's room", steps, 1, 0);
                if (d[0].size() || d[1].size()) return differ("bytes written by a refused step", steps, d[0].size() + d[1].size(), 0);
                ++room;
                r = device_model(table, ex, before.used, o[0].size(), o[1].size(), d);        // room that fits exactly
                if (r.refused) return differ("refused with room that fits exactly", steps, 1, 0);
            }
            if (r.consumed[0] != c[0]) return differ("consumed1", steps, r.consumed[0], c[0]);
            if (r.consumed[1] != c[1]) return differ("consumed2", steps, r.consumed[1], c[1]);
            if (r.pairs != st.headers - before.headers) return differ("pairs", steps, r.pairs, st.headers - before.headers);
            if (r.used != st.used - before.used) return differ("used", steps, r.used, st.used - before.used);
            for (int s = 0; s < 2; ++s) {
                if (r.out_bytes[s] != o[s].size()) return differ(s ? "out_bytes[1]" : "out_bytes[0]", steps, r.out_bytes[s], o[s].size());
                if (r.lines[s] != (uint64_t)std::count(ex[s].begin(), ex[s].end(), (uint8_t)'\n')) return differ("lines", steps, r.lines[s], 0);
                if (d[s] != o[s]) {
                    size_t k = 0;
                    while (k < d[s].size() && d[s][k] == o[s][k]) ++k;
                    return differ(s ? "byte of out2" : "byte of out1", steps, k, k);
                }
                if (o[s].size()) {
                    std::string none[2];
                    const StepResult shortr = device_model(table, ex, before.used, s == 0 ? o[0].size() - 1 : o[0].size(), s == 1 ? o[1].size() - 1 : o[1].size(), none);
                    if (!shortr.refused || shortr.out_bytes[0] != o[0].size() || shortr.out_bytes[1] != o[1].size() || none[0].size() || none[1].size())
                        return differ("a room one byte short", steps, shortr.refused, 1);
                    ++refused;
                }
            }
        }
        tx::progress_lines(before.headers, st.headers, log);
        fputs(log.c_str(), stdout);
        for (int s = 0; s < 2; ++s) {
            if (fwrite(o[s].data(), 1, o[s].size(), out[s]) != o[s].size()) return 3;
            have[s].erase(have[s].begin(), have[s].begin() + c[s]);
        }
        ++steps;
    }
    printf("Total %llu pair reads and used %llu pairs.\n", (unsigned long long)st.headers, (unsigned long long)st.used);
    fprintf(stderr, "steps=%llu on_model=%llu refused_short=%llu over_the_programs_room=%llu\n", (unsigned long long)steps, (unsigned long long)on_model,
            (unsigned long long)refused, (unsigned long long)room);
    return fclose(out[0]) || fclose(out[1]) ? 3 : 0;
}

static bool find_is(const std::vector<tx::TableSlot> &table, const std::string &key, const std::string *value) {
    uint32_t k[4];
    tx::pack_key(reinterpret_cast<const uint8_t *>(key.data()), (uint32_t)key.size(), k);
    const uint32_t at = tx::table_find(table.data(), (uint32_t)table.size(), k);
    if (!value) return at == tx::kNoSlot;
    return at != tx::kNoSlot && table[at].v == value->size() && memcmp(table[at].value, value->data(), value->size()) == 0;
}

static int run_tables(int n, char **paths) {
    for (int f = 0; f < n; ++f) {
        std::vector<uint8_t> text;
        if (!slurp(paths[f], text)) return 2;
        tx::Map map;
        tx::map_parse(text.data(), text.size(), map);
        if (!map.device_ok) {
            fprintf(stderr, "%s: not device_ok (%s)\n", paths[f], map.reason.c_str());
            return 1;
        }
        std::vector<tx::TableSlot> table;
        tx::table_build(map, table);
        size_t full = 0;
        for (const tx::TableSlot &s : table) full += s.key[0] != 0;
        if (full != map.kv.size() || (table.size() & (table.size() - 1)) || 2 * full > table.size()) {
            fprintf(stderr, "%s: %zu keys, %zu full slots of %zu\n", paths[f], map.kv.size(), full, table.size());
            return 1;
        }
        for (const auto &e : map.kv) {
            if (!find_is(table, e.first, &e.second)) { fprintf(stderr, "%s: key %s not found with its value\n", paths[f], e.first.c_str()); return 1; }
            // near misses: the key with its last byte changed, and (while it fits) with one byte more
            std::string miss = e.first;
            miss.back() = (char)(miss.back() ^ 1);
            if (!map.kv.count(miss) && !find_is(table, miss, nullptr)) { fprintf(stderr, "%s: %s found\n", paths[f], miss.c_str()); return 1; }
            miss = e.first + "x";
            if (miss.size() <= tx::kMaxKey && !map.kv.count(miss) && !find_is(table, miss, nullptr)) { fprintf(stderr, "%s: %s found\n", paths[f], miss.c_str()); return 1; }
        }
        fprintf(stderr, "%s: %zu keys in %zu slots\n", paths[f], map.kv.size(), table.size());
    }
    return 0;
}

// the key of `header` through key_record + table_find: the slot's value, "<none>" when key_record says the map cannot hold it,
// "<absent>" when the table does not
static std::string lookup(const std::vector<tx::TableSlot> &table, const std::string &header) {
    std::vector<uint8_t> buf(header.begin(), header.end());
    buf.push_back('\n');
    buf.shrink_to_fit();
    uint32_t k[4];
    if (!tx::key_record(buf.data(), 0, header.size(), k)) return "<none>";
    const uint32_t at = tx::table_find(table.data(), (uint32_t)table.size(), k);
    return at == tx::kNoSlot ? "<absent>" : std::string(reinterpret_cast<const char *>(table[at].value), table[at].v);
}

static int run_rules() {
    // the rows of test_key_rule_table (tests/test_tx_core_cpu.py): header -> key
    const char *rows[][2] = {{"@r#A_1/1\tx", "A_1"}, {"@r#A_1#zz/1", "A_1"}, {"@r/1#A_1", "A_1"}, {"@r\t#A_1/1", ""}, {"@r#A_1\r", "A_1\r"}, {"@r#A_1 /1", "A_1 "},
                             {"@r#/1", ""}, {"@r#", ""}, {"@r", ""}};
    for (const auto &row : rows) {
        const std::string head = row[0], key = row[1];
        for (int probe = 0; probe < 2; ++probe) {                          // a map that holds exactly the key keeps the pair, key + "x" drops it
            tx::Map map;
            const std::string text = (probe ? key + "x" : key) + "\tV\n";
            tx::map_parse(reinterpret_cast<const uint8_t *>(text.data()), text.size(), map);
            const std::string want = key.empty() ? "<none>" : probe ? "<absent>" : "V";
            if (!map.device_ok) {                                          // the empty key: such a map never reaches the device
                if (!key.empty() || probe) { fprintf(stderr, "rules: a map with key %s is not device_ok\n", text.c_str()); return 1; }
                map.kv.clear();
            }
            std::vector<tx::TableSlot> table;
            tx::table_build(map, table);
            const std::string got = lookup(table, head);
            if (got != want) { fprintf(stderr, "rules: header %s with map key %s: %s, not %s\n", head.c_str(), text.c_str(), got.c_str(), want.c_str()); return 1; }
        }
    }
    // a table at load exactly 0.5: 4096 keys in 8192 slots, among them keys of 15 bytes; header keys of 15 bytes are found, of 16
    // bytes cannot be in the map, absent keys end at an empty slot
    tx::Map map;
    char buf[64];
    for (int i = 0; i < 4096; ++i) {
        snprintf(buf, sizeof buf, i % 2 ? "K%014d" : "k%d", i);            // 15 bytes, or 2 .. 5
        map.kv[buf] = std::string((size_t)(i % 17), (char)('A' + i % 4));
    }
    std::vector<tx::TableSlot> table;
    tx::table_build(map, table);
    if (table.size() != 8192) { fprintf(stderr, "rules: 4096 keys in %zu slots\n", table.size()); return 1; }
    for (const auto &e : map.kv) {
        if (lookup(table, "@read#" + e.first + "/1") != e.second) { fprintf(stderr, "rules: %s not found at load 0.5\n", e.first.c_str()); return 1; }
        if (lookup(table, "@read#" + e.first + "_/1") != (e.first.size() == 15 ? "<none>" : "<absent>")) { fprintf(stderr, "rules: %s_ found\n", e.first.c_str()); return 1; }
    }
    for (int i = 4096; i < 12288; ++i) {
        snprintf(buf, sizeof buf, i % 2 ? "K%014d" : "k%d", i);
        if (lookup(table, std::string("@r#") + buf) != "<absent>") { fprintf(stderr, "rules: absent key %s found\n", buf); return 1; }
    }
    if (lookup(table, "@r#K234567890123456/1") != "<none>" || lookup(table, "@r#K00000000000001") != map.kv["K00000000000001"]) {
        fprintf(stderr, "rules: header keys of 16 and 15 bytes\n");
        return 1;
    }
    fprintf(stderr, "rules ok\n");
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 2 && strcmp(argv[1], "--rules") == 0) return run_rules();
    if (argc >= 3 && strcmp(argv[1], "--table") == 0) return run_tables(argc - 2, argv + 2);
    if (argc != 8 || strcmp(argv[1], "-b") != 0 || strtoull(argv[2], nullptr, 10) < 1) {
        fprintf(stderr, "usage: test_tx_plan -b BLOCK READ1 READ2 MAP OUT1 OUT2 | --table MAP... | --rules\n");
        return 2;
    }
    return run_blocks(strtoull(argv[2], nullptr, 10), argv + 3);
}
