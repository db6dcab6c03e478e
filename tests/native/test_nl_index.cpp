// Host test of nl_bits4 (hast_amd/csrc/nl_index.h), the word -> 4-bit step of the newline index the framing kernels share: against a
// byte loop, on all 16^4 words over an alphabet that holds every neighbour of '\n' under the carries of the bit trick -- '\n' itself,
// the bytes one bit from it (0B, 1A, 2A, 4A, 8A), its complement and theirs, and what the +0x7F and the high-bit mask could confuse
// (00, 7F, 80, FF).
#include <cstdint>
#include <cstdio>

#include "../../hast_amd/csrc/nl_index.h"

int main() {
    const uint8_t alpha[16] = {0x00, 0x09, 0x0A, 0x0B, 0x0D, 0x1A, 0x2A, 0x4A, 0x7F, 0x80, 0x8A, 0x8B, 0xF5, 0xFF, 0x0A ^ 0xFF, 0x8A ^ 0xFF};
    uint32_t checked = 0, with_nl = 0;
    for (uint32_t i = 0; i < 65536; ++i) {
        uint32_t w = 0, want = 0;
        for (int b = 0; b < 4; ++b) {
            const uint8_t c = alpha[(i >> (4 * b)) & 15];
            w |= (uint32_t)c << (8 * b);
            if (c == '\n') want |= 1u << b;
        }
        const uint32_t got = hast::nl_bits4(w);
        if (got != want) {
            printf("FAIL word %08x: got %x want %x\n", w, got, want);
            return 1;
        }
        ++checked;
        with_nl += want != 0;
    }
    // the sizing helpers: a range of n bytes that starts up to 15 bytes into its first tile; an index of n newlines
    for (size_t n = 0; n < 5 * hast::kNlTile; ++n)
        if (hast::nl_tiles(n) < (n + 15 + hast::kNlTile - 1) / hast::kNlTile || hast::nl_tiles(n) < 1 || hast::nl_index_words(n) < n) {
            printf("FAIL sizes of %zu bytes\n", n);
            return 1;
        }
    printf("ok %u words, %u with a newline\n", checked, with_nl);
    return 0;
}
