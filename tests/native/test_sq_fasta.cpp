// Host model of the stage-00 device ingest of FASTA (test infrastructure): frames views of raw FASTA with the rules of
// hast_amd/csrc/sq_core.h (namespace sqfa), the code the kernels of sq_fasta_kernels.hip step.
//
//   sq_fasta_model_frame()   one view, the contract of hast_sq_frame_fasta_device (tests/test_sq_fasta_gpu.py loads this file as a
//                            shared library, built with -DSQ_FASTA_MODEL_LIB)
//   main()                   test_sq_fasta -b BLOCK [-c] FILE...: every file (with -c: all files as one stream) block by block the way
//                            hast_sq_feed_* feeds it -- a view is [what the view before left | up to BLOCK new bytes], [consumed, n) is
//                            carried, a header seen in an earlier view opens the next one, and what is carried at the end of the input is
//                            the last view -- the stream to FILE.sqfa (-c: the first file's name) and one line per input to stdout:
//                                STATUS records bases bytes views
//                            STATUS: ok | nofit (more than BLOCK bytes to carry: a line longer than a block) | io
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <sys/stat.h>

#include "../../hast_amd/csrc/sq_core.h"

struct SqModelResult {          // = hast_sq_result
    uint64_t consumed, out_bytes, records, bases;
    uint32_t flags, first_bad;
};

extern "C" void sq_fasta_model_frame(const uint8_t *in, size_t n, unsigned in_flags, uint8_t *out, SqModelResult *res) {
    namespace fa = hast::sqfa;
    const bool open_in = (in_flags & SQ_FA_OPEN) != 0, last = (in_flags & SQ_FA_LAST) != 0;
    std::vector<uint32_t> nl;
    for (size_t i = 0; i < n; ++i)
        if (in[i] == '\n') nl.push_back((uint32_t)i);
    const uint32_t n_nl = (uint32_t)nl.size(), n_lines = fa::n_lines(nl.data(), n_nl, n, last);
    uint32_t raw = 0, hdrs = 0;
    for (uint32_t j = 0; j < n_lines; ++j) {
        const uint32_t lo = fa::line_lo(nl.data(), j), hi = fa::line_hi(nl.data(), n_nl, n, j);
        uint32_t len;
        const uint32_t cls = fa::line_class(in, lo, hi, &len), k = fa::emit(cls, len, hdrs, open_in);
        uint8_t *o = out + fa::line_dst(raw, hdrs, open_in);
        if (cls == fa::kHeader && k) *o = '\n';
        if (cls == fa::kSequence) memcpy(o, in + lo, k);
        raw += fa::raw_emit(cls, len);
        hdrs += cls == fa::kHeader;
    }
    const uint32_t lines_bytes = fa::line_dst(raw, hdrs, open_in), closing = fa::closing(hdrs, open_in, last);
    if (closing) out[lines_bytes] = '\n';
    *res = SqModelResult{fa::consumed(nl.data(), n_nl, n, last), (uint64_t)lines_bytes + closing, hdrs, fa::bases(raw, hdrs), 0, hast::sq::kNoBad};
}

#ifndef SQ_FASTA_MODEL_LIB
namespace {
size_t size_of(const char *path) {
    struct stat sb;
    return stat(path, &sb) == 0 ? (size_t)sb.st_size : 0;
}

struct Input {
    std::vector<uint8_t> view, framed;
    std::string stream;
    size_t block, piece, have = 0, bytes = 0, views = 0, records = 0, bases = 0;      // piece: min(block, the input's size), what the buffers are sized by
    bool open = false, nofit = false;
    Input(size_t b, size_t total) : block(b), piece(b < total ? b : total + 1) {
        view.resize(2 * piece);
        framed.resize(2 * piece + 1);
    }
    void frame(bool last) {
        SqModelResult r;
        sq_fasta_model_frame(view.data(), have, (open ? SQ_FA_OPEN : 0u) | (last ? SQ_FA_LAST : 0u), framed.data(), &r);
        if (have - r.consumed > block) {
            nofit = true;
            return;
        }
        ++views;
        stream.append(reinterpret_cast<const char *>(framed.data()), r.out_bytes);
        records += r.records;
        bases += r.bases;
        if (r.records) open = true;
        memmove(view.data(), view.data() + r.consumed, have - r.consumed);
        have -= r.consumed;
    }
    bool file(const char *path) {
        FILE *f = fopen(path, "rb");
        if (!f) return false;
        for (size_t got; !nofit && (got = fread(view.data() + have, 1, piece, f)) > 0;) {
            bytes += got;
            have += got;
            frame(false);
        }
        fclose(f);
        return true;
    }
    void finish(const char *path) {
        if (!nofit) frame(true);
        const std::string op = std::string(path) + ".sqfa";
        if (FILE *o = fopen(op.c_str(), "wb")) {
            if (!nofit) fwrite(stream.data(), 1, stream.size(), o);
            fclose(o);
        }
        printf("%s %zu %zu %zu %zu\n", nofit ? "nofit" : "ok", records, bases, bytes, views);
    }
};
}  // namespace

int main(int argc, char **argv) {
    size_t block = 1 << 16;
    bool concat = false;
    std::vector<const char *> files;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "-b") && i + 1 < argc) block = (size_t)atol(argv[++i]);
        else if (!strcmp(argv[i], "-c")) concat = true;
        else files.push_back(argv[i]);
    }
    if (block < 1 || files.empty()) return 2;
    if (concat) {
        size_t total = 0;
        for (const char *p : files) total += size_of(p);
        Input in(block, total);
        for (const char *p : files)
            if (!in.file(p)) {
                printf("io 0 0 0 0\n");
                return 0;
            }
        in.finish(files[0]);
        return 0;
    }
    for (const char *p : files) {
        Input in(block, size_of(p));
        if (!in.file(p)) printf("io 0 0 0 0\n");
        else in.finish(p);
    }
    return 0;
}
#endif
