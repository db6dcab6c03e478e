// quartering.h -- the routing step right after `classify` in HAST stage 01, shared by the stand-alone program
// (quartering_main.cpp) and by `classify` itself (HAST_PHASE_READS=1: steps 10 and 11 of the wrapper done by the program that has the
// barcodes' classes in memory and the GPU's inflate at hand): every FASTQ record to <prefix>.{paternal,maternal,homozygous,nobarcode}.fastq
// by the barcode lists, which the reference does with single-threaded awk
// (/root/reference/01.classify_stlfr_reads/quartering_fastq.awk, invoked at classify_stlfr_reads.sh:176-185).
//
// Same outputs byte for byte: the four FASTQ files (created only when something is routed to them), the
// "ERROR : unclassify barcode" lines on stderr (those records are dropped, awk :31-34) and the lines appended
// to filter_reads.log (awk :18-20, :51-57).  Semantics restated from the awk program: fields are split at '#'
// or '/' (-F '#|/'); a list line contributes its first field (:12-16); a header line (every 4th line from the
// first, :21) with more than one field and a second field other than "0_0_0" is looked up in the paternal, then
// maternal, then homozygous list (:23-35), otherwise it is a no-barcode read (:36-39); all four lines follow the
// header's class (:41-49).  Host code; the bytes come from a block source (ingest.h BlockSource: plain files, .gz inflated by the
// host decoders, "-"; or anything else with next() / recycle() / error(), e.g. a .gz inflated on the GPU).
#pragma once
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <string_view>
#include <unordered_map>
#include <vector>

#include <zlib.h>

#include "ingest.h"

namespace hast {
namespace quartering {

// --gz-out: what the host routes leaves as gzip members too (<prefix>.<class>.fastq.gz; concatenated members are one gzip file, so the
// members `classify` gets from the GPU's encoder and the ones made here share a file).  n bytes -> one member appended to out; level 1,
// as the files are an intermediate that the next stage reads once.  False: zlib failed (out of memory).
inline bool gz_member(const char *p, size_t n, std::string &out) {
    z_stream z;
    memset(&z, 0, sizeof z);
    if (deflateInit2(&z, 1, Z_DEFLATED, 15 + 16, 8, Z_DEFAULT_STRATEGY) != Z_OK) return false;
    const size_t at = out.size();
    out.resize(at + deflateBound(&z, (uLong)n) + 32);
    size_t done = 0, written = 0;
    int rc = Z_OK;
    do {                                                            // (avail_in is 32 bits wide)
        const size_t take = std::min<size_t>(n - done, 1u << 30);
        z.next_in = reinterpret_cast<Bytef *>(const_cast<char *>(p + done));
        z.avail_in = (uInt)take;
        done += take;
        do {
            if (out.size() - at - written < (1u << 16)) out.resize(out.size() + (1u << 20));
            z.next_out = reinterpret_cast<Bytef *>(&out[at + written]);
            const size_t room = std::min<size_t>(out.size() - at - written, 1u << 30);
            z.avail_out = (uInt)room;
            rc = deflate(&z, done == n ? Z_FINISH : Z_NO_FLUSH);
            written += room - z.avail_out;
        } while (rc == Z_OK && z.avail_out == 0);
    } while (rc == Z_OK && done < n);
    deflateEnd(&z);
    out.resize(at + written);
    return rc == Z_STREAM_END;
}
// --gz-format bgzf: the same bytes as BLOCKED gzip (BGZF: bgzip, htslib, hast_gz_open_blocked), the host twin of the device encoder's
// blocked mode (dz_core.h): raw deflate (level 1) over slices of at most kBgzfSlice bytes -- what a member of the device's holds --
// each wrapped as a member of its own: 18 bytes of header with the BC subfield (BSIZE = the member's bytes - 1), CRC-32 and ISIZE of
// the slice.  n bytes -> ceil(n / kBgzfSlice) members appended to out (n = 0: nothing); host-made members need not equal the
// device's byte for byte.  False: zlib failed.
enum class GzFormat { kNone, kGzip, kBgzf };    // how the four files are written: plain, gzip members, BGZF members
constexpr size_t kBgzfSlice = 3 * 16384;
constexpr size_t kBgzfFrame = 18 + 2 + 8;       // header + the empty final block the device writes + trailer: a member's bytes beside its pieces
// the end-of-file block every BGZF file ends with: an empty member
constexpr unsigned char kBgzfEof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
inline size_t bgzf_member_count(size_t n) { return (n + kBgzfSlice - 1) / kBgzfSlice; }
inline bool bgzf_members(const char *p, size_t n, std::string &out) {
    for (size_t done = 0; done < n;) {
        const size_t take = std::min(n - done, kBgzfSlice);
        z_stream z;
        memset(&z, 0, sizeof z);
        if (deflateInit2(&z, 1, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) return false;
        const size_t at = out.size(), room = deflateBound(&z, (uLong)take);
        out.resize(at + 18 + room + 8);
        z.next_in = reinterpret_cast<Bytef *>(const_cast<char *>(p + done));
        z.avail_in = (uInt)take;
        z.next_out = reinterpret_cast<Bytef *>(&out[at + 18]);
        z.avail_out = (uInt)room;
        const int rc = deflate(&z, Z_FINISH);
        const size_t total = 18 + (room - z.avail_out) + 8;
        deflateEnd(&z);
        if (rc != Z_STREAM_END || total > (1u << 16)) return false;     // (deflateBound of 48 KB is 48 KB + 22 bytes: it fits)
        memcpy(&out[at], kBgzfEof, 16);
        out[at + 16] = (char)((total - 1) & 0xFF);
        out[at + 17] = (char)((total - 1) >> 8);
        const uint32_t crc = (uint32_t)crc32(0, reinterpret_cast<const Bytef *>(p + done), (uInt)take), isize = (uint32_t)take;
        for (int k = 0; k < 4; k++) {
            out[at + total - 8 + k] = (char)(crc >> (8 * k));
            out[at + total - 4 + k] = (char)(isize >> (8 * k));
        }
        out.resize(at + total);
        done += take;
    }
    return true;
}
struct GzOutStats {             // --stats: what went into and came out of the encoder, members written (an end-of-file block is one)
    unsigned long long bytes_in = 0, bytes_out = 0, members = 0;
};

inline std::string_view field(std::string_view line, int idx) {      // idx-th field under -F '#|/' (0-based); npos data() if absent
    size_t start = 0;
    for (int f = 0;; ++f) {
        size_t e = start;
        while (e < line.size() && line[e] != '#' && line[e] != '/') ++e;
        if (f == idx) return line.substr(start, e - start);
        if (e >= line.size()) return std::string_view(nullptr, 0);
        start = e + 1;
    }
}

using ClassMap = std::unordered_map<std::string, uint8_t>;           // first field of a list line -> 1 paternal, 2 maternal, 3 homozygous

inline bool load_list(const std::string &path, uint8_t cls, ClassMap &map) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return false;
    std::string data;
    char buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) data.append(buf, n);
    fclose(f);
    size_t pos = 0;
    while (pos < data.size()) {
        size_t e = data.find('\n', pos);
        if (e == std::string::npos) e = data.size();
        std::string_view line(data.data() + pos, e - pos);
        map.emplace(std::string(field(line, 0)), cls);             // first list wins, as the awk's if/else chain does
        pos = e + 1;
    }
    return true;
}

// Routes the records of one input.  src: next() -> a block with kFrontPad bytes of room in front of its data (empty = end of input),
// recycle(), error().  log_name: what awk's FILENAME would be (the path as given, "-" behind `gzip -dc`).  who: the program's name in
// messages.  Returns 0, or the exit code of a failure (2: I/O, 3: a record larger than 4 GB).
// format other than kNone: the four files are <prefix>.<class>.fastq.gz, every worker's share of a block one gzip member, or (kBgzf)
// BGZF members of at most kBgzfSlice bytes and an end-of-file block where a file ends (gz_stats: totals, may be null)
template <class Source>
int route(const std::string &prefix, const ClassMap &cls_of, Source &src, const std::string &log_name, int t_num, const char *who,
          GzFormat format = GzFormat::kNone, GzOutStats *gz_stats = nullptr) {
    const bool gz_out = format != GzFormat::kNone, bgzf = format == GzFormat::kBgzf;
    hast::WorkerPool pool(t_num);
    const int T = pool.size();
    const char *suffix_plain[4] = {".nobarcode.fastq", ".paternal.fastq", ".maternal.fastq", ".homozygous.fastq"};
    const char *suffix_gz[4] = {".nobarcode.fastq.gz", ".paternal.fastq.gz", ".maternal.fastq.gz", ".homozygous.fastq.gz"};
    const char *const *suffix = gz_out ? suffix_gz : suffix_plain;
    FILE *out[4] = {nullptr, nullptr, nullptr, nullptr};
    long long counts[5] = {0, 0, 0, 0, 0};                         // no, pa, ma, ho, total
    bool any_input = false;
    struct Local {
        std::string buf[4], err, zbuf;
        long long n[4] = {0, 0, 0, 0};
        bool z_failed = false;
        GzOutStats z;
    };
    // a worker's four buffers, each replaced by one gzip member of its bytes (BGZF: by the members of its slices)
    auto compress_local = [&](Local &L) {
        for (int c = 0; c < 4; c++) {
            if (L.buf[c].empty()) continue;
            L.zbuf.clear();
            if (!(bgzf ? bgzf_members(L.buf[c].data(), L.buf[c].size(), L.zbuf) : gz_member(L.buf[c].data(), L.buf[c].size(), L.zbuf))) L.z_failed = true;
            L.z.bytes_in += L.buf[c].size();
            L.z.bytes_out += L.zbuf.size();
            L.z.members += bgzf ? bgzf_member_count(L.buf[c].size()) : 1;
            L.buf[c].swap(L.zbuf);
        }
    };
    std::vector<Local> loc(T);

    // class of a header line: 0 nobarcode, 1..3 lists, -1 unclassified (dropped with an ERROR line)
    auto classify = [&](std::string_view head, std::string &err) -> int {
        std::string_view f2 = field(head, 1);
        if (f2.data() == nullptr || f2 == "0_0_0") return 0;        // NF <= 1, or the no-barcode marker (awk :22,36-39)
        auto it = cls_of.find(std::string(f2));
        if (it != cls_of.end()) return it->second;
        err.append("ERROR : unclassify barcode : ").append(f2).append("\n");
        return -1;
    };
    bool write_failed = false;
    auto emit = [&]() {                                             // worker buffers -> files, in input order
        for (int t = 0; t < T; t++) {
            fputs(loc[t].err.c_str(), stderr);
            if (loc[t].z_failed) {
                fprintf(stderr, "%s: cannot compress the records of %s\n", who, prefix.c_str());
                write_failed = true;
                return;
            }
            if (gz_stats) {
                gz_stats->bytes_in += loc[t].z.bytes_in;
                gz_stats->bytes_out += loc[t].z.bytes_out;
                gz_stats->members += loc[t].z.members;
            }
            loc[t].z = GzOutStats();
            for (int c = 0; c < 4; c++) {
                counts[c] += loc[t].n[c];
                if (loc[t].buf[c].empty()) continue;
                if (!out[c]) out[c] = fopen((prefix + suffix[c]).c_str(), "wb");
                if (!out[c] || fwrite(loc[t].buf[c].data(), 1, loc[t].buf[c].size(), out[c]) != loc[t].buf[c].size()) {
                    fprintf(stderr, "%s: cannot write %s%s\n", who, prefix.c_str(), suffix[c]);
                    write_failed = true;
                    return;
                }
            }
        }
    };
    hast::BlockWork work;                                          // (carry + block, newline index: ingest.h)
    for (;;) {
        if (!work.next(src)) {
            fprintf(stderr, "%s: %s\n", who, src.error().c_str());
            for (FILE *f : out) if (f) fclose(f);
            return 2;
        }
        const char *data = work.data;
        const size_t len = work.len;
        if (len) any_input = true;
        if (len >= (1ull << 32)) { fprintf(stderr, "%s: record larger than 4 GB\n", who); return 3; }
        work.index(pool);
        const std::vector<uint32_t> &allnl = work.nl;
        const size_t n_rec = allnl.size() / 4;
        pool.run([&](int t) {
            Local &L = loc[t];
            for (auto &b : L.buf) b.clear();
            L.err.clear();
            for (auto &x : L.n) x = 0;
            for (size_t i = n_rec * (size_t)t / T; i < n_rec * (size_t)(t + 1) / T; i++) {
                const size_t r0 = i ? (size_t)allnl[4 * i - 1] + 1 : 0, h1 = allnl[4 * i], r1 = (size_t)allnl[4 * i + 3] + 1;
                const int c = classify(std::string_view(data + r0, h1 - r0), L.err);
                if (c >= 0) { L.buf[c].append(data + r0, r1 - r0); L.n[c]++; }
            }
            if (gz_out) compress_local(L);
        });
        counts[4] += (long long)n_rec;
        emit();
        if (write_failed) break;
        const size_t consumed = n_rec ? (size_t)allnl[4 * n_rec - 1] + 1 : 0;
        if (work.last) {
            // trailing partial record: awk still treats every remaining line (terminated or not) as a record (:21,41-49)
            std::string_view rest(data + consumed, len - consumed);
            if (!rest.empty()) {
                Local &L = loc[0];
                for (int t = 0; t < T; t++) { for (auto &b : loc[t].buf) b.clear(); loc[t].err.clear(); for (auto &x : loc[t].n) x = 0; }
                size_t e = rest.find('\n');
                const int c = classify(rest.substr(0, e == std::string_view::npos ? rest.size() : e), L.err);
                counts[4]++;
                if (c >= 0) {
                    L.buf[c].append(rest);
                    if (rest.back() != '\n') L.buf[c].push_back('\n');
                    L.n[c]++;
                }
                if (gz_out) compress_local(L);
                emit();
            }
            break;
        }
        work.keep(src, consumed);
    }
    for (FILE *f : out) {
        if (!f) continue;
        if (bgzf && !write_failed) {                                // every BGZF file that exists ends with one end-of-file block
            if (fwrite(kBgzfEof, 1, sizeof kBgzfEof, f) != sizeof kBgzfEof) write_failed = true;
            if (gz_stats) gz_stats->bytes_out += sizeof kBgzfEof, gz_stats->members++;
        }
        if (fclose(f) != 0) write_failed = true;
    }
    if (write_failed) return 2;
    FILE *lg = fopen("filter_reads.log", "ab");
    if (lg) {
        if (any_input) fprintf(lg, "%s\n", log_name.c_str());           // awk :18-20 (FNR==1 of the reads file)
        fprintf(lg, "#Total reads                : %lld \n", counts[4]);
        fprintf(lg, "#Reads without barcode      : %lld \n", counts[0]);
        fprintf(lg, "#Paternal reads             : %lld \n", counts[1]);
        fprintf(lg, "#Maternal reads             : %lld \n", counts[2]);
        fprintf(lg, "#Homozygous reads           : %lld \n", counts[3]);
        fclose(lg);
    }
    return 0;
}

}  // namespace quartering
}  // namespace hast
