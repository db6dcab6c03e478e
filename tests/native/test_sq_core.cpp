// Host model of the stage-00 device ingest (test infrastructure): frames four-line FASTQ with the rules of
// hast_amd/csrc/sq_core.h, the code the kernels of sq_kernels.hip step.
//
//   sq_model_frame()   one block, the contract of hast_sq_frame_device (tests/test_sq_gpu.py loads this file as a shared library,
//                      built with -DSQ_MODEL_LIB)
//   main()             test_sq_core -b BLOCK FILE...: every file block by block the way `unshared_kmers --ingest device` feeds it --
//                      [consumed, n) of a block carried in front of the next bytes, the tail at the end of the file through SeqParser --
//                      the stream to FILE.sq and one line per file to stdout:
//                          STATUS records bases bytes blocks first_bad [: message]
//                      STATUS: ok | flagged (a record breaks a rule) | nofit (a full block without a record) | badfirst (the file does
//                      not start with '@') | tail (SeqParser refuses the tail; its message follows).  Everything but ok is a refusal: the
//                      program then reads the input with the host parser.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../hast_amd/csrc/seqstream.h"
#include "../../hast_amd/csrc/sq_core.h"

struct SqModelResult {          // = hast_sq_result
    uint64_t consumed, out_bytes, records, bases;
    uint32_t flags, first_bad;
};

extern "C" void sq_model_frame(const uint8_t *in, size_t n, uint8_t *out, SqModelResult *res) {
    std::vector<uint32_t> nl;
    for (size_t i = 0; i < n; ++i)
        if (in[i] == '\n') nl.push_back((uint32_t)i);
    *res = SqModelResult{0, 0, 0, 0, 0, hast::sq::kNoBad};
    const uint32_t n_rec = (uint32_t)(nl.size() / 4);
    if (n_rec == 0) {
        res->flags = SQ_NO_RECORD;
        return;
    }
    std::vector<uint32_t> at(n_rec), ls(n_rec);
    for (uint32_t i = 0; i < n_rec; ++i)
        if (!hast::sq::record_at(in, nl.data(), i, &at[i], &ls[i])) {
            res->flags = SQ_NOT_FOUR_LINE;          // refused as a whole: nothing is written
            res->first_bad = i;
            return;
        }
    uint8_t *o = out;
    for (uint32_t i = 0; i < n_rec; ++i) {
        if (ls[i]) memcpy(o, in + at[i], ls[i]);
        o += ls[i];
        *o++ = '\n';
        res->bases += ls[i];
    }
    res->records = n_rec;
    res->out_bytes = (uint64_t)(o - out);
    res->consumed = (uint64_t)nl[4 * (size_t)n_rec - 1] + 1;
}

#ifndef SQ_MODEL_LIB
namespace {
struct Out {
    std::string s;
    size_t bases = 0;
    void append(const char *p, size_t n) { s.append(p, n); bases += n; }
    void separator() { s.push_back('\n'); }
};

void one_file(const char *path, size_t block) {
    FILE *f = fopen(path, "rb");
    if (!f) {
        printf("io 0 0 0 0 0\n");
        return;
    }
    std::vector<uint8_t> in(block), framed(block);
    Out out;
    size_t have = 0, bytes = 0, blocks = 0, records = 0;
    const char *status = "ok";
    std::string msg;
    uint32_t first_bad = hast::sq::kNoBad;
    bool first = true, eof = false;
    while (!eof) {
        const size_t room = block - have, got = fread(in.data() + have, 1, room, f);
        eof = got < room;
        bytes += got;
        have += got;
        if (first && have) {
            first = false;
            if (in[0] != '@') { status = "badfirst"; break; }
        }
        SqModelResult r;
        sq_model_frame(in.data(), have, framed.data(), &r);
        if (r.flags & SQ_NOT_FOUR_LINE) { status = "flagged"; first_bad = r.first_bad; break; }
        if (r.flags & SQ_NO_RECORD) {
            if (!eof) status = "nofit";              // (the buffer is full)
            break;
        }
        ++blocks;
        out.s.append(reinterpret_cast<const char *>(framed.data()), r.out_bytes);
        out.bases += r.bases;
        records += r.records;
        memmove(in.data(), in.data() + r.consumed, have - r.consumed);      // fewer than four newlines
        have -= r.consumed;
    }
    fclose(f);
    if (!strcmp(status, "ok")) {                     // fewer than four newlines are left: the parser's
        hast::SeqParser<Out> parser(out);
        if (!parser.feed(reinterpret_cast<const char *>(in.data()), have) || !parser.finish()) {
            status = "tail";
            msg = parser.error();
        }
        records += parser.records();
    }
    const std::string op = std::string(path) + ".sq";
    if (FILE *o = fopen(op.c_str(), "wb")) {
        if (!strcmp(status, "ok")) fwrite(out.s.data(), 1, out.s.size(), o);
        fclose(o);
    }
    printf("%s %zu %zu %zu %zu %u%s%s\n", status, records, out.bases, bytes, blocks, first_bad, msg.empty() ? "" : " : ", msg.c_str());
}
}  // namespace

int main(int argc, char **argv) {
    size_t block = 1 << 16;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "-b")) block = (size_t)atol(argv[++i]);
        else one_file(argv[i], block);
    }
    return 0;
}
#endif
