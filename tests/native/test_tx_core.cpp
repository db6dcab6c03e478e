// test_tx_core.cpp -- steps the host model of the stLFR -> 10x conversion (hast_amd/csrc/tx_host.h over tx_core.h) the way the
// fake_10x program feeds it: both inputs in blocks of -b bytes, what a step leaves carried in front of the next block, the end of
// the inputs handed to the model's final step.
//   test_tx_core -b BLOCK READ1 READ2 MAP OUT1 OUT2
// READ1 / READ2 are plain FASTQ.  stdout is the script's; stderr gets one line about the map.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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

int main(int argc, char **argv) {
    if (argc != 8 || strcmp(argv[1], "-b") != 0) {
        fprintf(stderr, "usage: test_tx_core -b BLOCK READ1 READ2 MAP OUT1 OUT2\n");
        return 2;
    }
    const size_t block = strtoull(argv[2], nullptr, 10);
    std::vector<uint8_t> in[2], map_text;
    if (block < 1 || !slurp(argv[3], in[0]) || !slurp(argv[4], in[1]) || !slurp(argv[5], map_text)) return 2;
    tx::Map map;
    tx::map_parse(map_text.data(), map_text.size(), map);
    fprintf(stderr, "map: n_keys=%zu device_ok=%d reason=%s\n", map.kv.size(), map.device_ok ? 1 : 0, map.reason.c_str());
    printf("Merge stLFR reads into 10X format !\n read1 :  %s \n. read2 : %s \n map file : %s\n", argv[3], argv[4], argv[5]);
    FILE *out[2] = {fopen(argv[6], "wb"), fopen(argv[7], "wb")};
    if (!out[0] || !out[1]) return 2;
    tx::State st;
    std::vector<uint8_t> have[2];            // carried bytes + the block just read, exactly: a read past the end is the sanitizer's to see
    size_t at[2] = {0, 0};
    uint64_t steps = 0;
    for (bool final = false; !final;) {
        for (int s = 0; s < 2; ++s) {
            const size_t take = std::min(block, in[s].size() - at[s]);
            have[s].insert(have[s].end(), in[s].begin() + at[s], in[s].begin() + at[s] + take);
            at[s] += take;
        }
        std::string o[2], log;
        size_t c[2];
        const uint64_t before = st.headers;
        std::vector<uint8_t> a(have[0]), b(have[1]);                       // (exact-size copies: no slack behind the last byte)
        a.shrink_to_fit();
        b.shrink_to_fit();
        const int mode = tx::step_mode(at[0] == in[0].size(), at[1] == in[1].size(), a.data(), a.size(), b.data(), b.size());
        final = mode == tx::kFinal;
        tx::pair_host(map, a.data(), a.size(), b.data(), b.size(), mode, st, o[0], o[1], &c[0], &c[1]);
        tx::progress_lines(before, st.headers, log);
        fputs(log.c_str(), stdout);
        for (int s = 0; s < 2; ++s) {
            if (fwrite(o[s].data(), 1, o[s].size(), out[s]) != o[s].size()) return 3;
            have[s].erase(have[s].begin(), have[s].begin() + c[s]);
        }
        ++steps;
    }
    printf("Total %llu pair reads and used %llu pairs.\n", (unsigned long long)st.headers, (unsigned long long)st.used);
    fprintf(stderr, "steps=%llu\n", (unsigned long long)steps);
    return fclose(out[0]) || fclose(out[1]) ? 3 : 0;
}
