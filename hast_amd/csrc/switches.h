// switches.h -- every environment variable the library and the programs read: one table, one reader per kind.  Host only, nothing but
// the standard library.  This file holds the only getenv( of hast_amd/csrc; tools/switch_table.py prints INTEGRATION.md's table from
// the rows below, and tests/test_switches_cpu.py holds source, table and document to each other.
//
// A reader takes an id of the table (a name that has no row does not compile) and reads the environment when it is called: nothing
// is cached here, a site that reads once keeps its own `static`.  A value that is not what the row takes counts as unset, and one
// line on stderr says so, once per variable and process.  Bounds that depend on something else (HAST_MINIMIZER <= K) and rounding
// stay with the caller.
#pragma once
#include <atomic>
#include <cctype>
#include <cerrno>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace hast {

// a count or a size, on the command line and in the environment: decimal digits and at most one of K, M, G behind them (powers of
// 1024, either case); anything else -- no digits, a sign, a fraction, another suffix, trailing bytes, more than 64 bits hold -- is
// not a number
inline bool parse_count(const char *text, uint64_t *out) {
    if (!text || *text < '0' || *text > '9') return false;
    errno = 0;
    char *end = nullptr;
    const unsigned long long v = strtoull(text, &end, 10);
    if (errno || end == text) return false;
    int shift = 0;
    switch (*end) {
    case 'K': case 'k': shift = 10; end++; break;
    case 'M': case 'm': shift = 20; end++; break;
    case 'G': case 'g': shift = 30; end++; break;
    default: break;
    }
    if (*end || (shift && v > (~0ull >> shift))) return false;
    *out = (uint64_t)v << shift;
    return true;
}

namespace sw {

enum Kind { Flag, FlagDefaultOn, Int, Size, Real, Word };
enum Policy { Clamp, Ignore };                 // a number outside [lo, hi]: taken as the nearer bound, or not taken
constexpr double NOLIM = 1.8446744073709552e19;  // hi of a row without an upper bound (2^64)

// X(name, kind, lo, hi, policy, words, default, read by and when, meaning) -- one row on one line; lo, hi and policy count for
// Int, Size and Real, words ("a|b") for Word.  The last three columns are the document's.
#define HAST_SWITCHES(X) \
    X(HAST_CLASSIFY, Word, 0, 0, Ignore, "exact|filter", "filter", "hast_ctx_create", "`exact` probes the exact table directly (the round-1 kernel) instead of the filter") \
    X(HAST_FILTER_EXACT, Word, 0, 0, Ignore, "0|1|once", "1", "hast_ctx_create", "`0` keeps 16-bit prints in the filter where exact entries would fit; `once` files exact entries once per strand under the sampled m-mer where they would be filed under every m-mer (DESIGN section 2, dense filing)") \
    X(HAST_FILTER_M, Int, 0, 32, Ignore, "", "by K and key count", "hast_ctx_create", "the filter's m-mer length (0 = default)") \
    X(HAST_FILTER_T, Int, 0, 32, Ignore, "", "by K and key count", "hast_ctx_create", "the filter's t-mer length (0 = default)") \
    X(HAST_FILTER_KP, Int, 0, 32, Ignore, "", "by K and key count", "hast_ctx_create", "the filter's print length (0 = default)") \
    X(HAST_F_GEO, FlagDefaultOn, 0, 0, Ignore, "", "on", "hast_ctx_create", "`0` runs the generic probe kernel where one with the filter geometry compiled in exists") \
    X(HAST_F_RL, FlagDefaultOn, 0, 0, Ignore, "", "on", "hast_ctx_create", "`0` runs the probe kernel without the read length compiled in") \
    X(HAST_TILE_LDS, Size, 4096, 163840, Ignore, "", "by the device", "hast_ctx_create", "bytes of LDS a classify tile may take") \
    X(HAST_COUNT_LOOKUPS, Flag, 0, 0, Ignore, "", "off", "hast_ctx_create", "the probe kernel counts its table look-ups (slower; hast_ctx_lookups)") \
    X(HAST_TEST_FILTER_OOM, Flag, 0, 0, Ignore, "", "off", "hast_ctx_create", "the filter's allocation fails: the fallback's messages") \
    X(HAST_COMMIT, Word, 0, 0, Ignore, "atomic|partition", "by batch size", "hast_ctx_create", "forces one of the two per-barcode bookkeeping paths (default: batches of >= 2M device-resident reads over >= 128 bins of barcodes are partitioned and summed in LDS, everything else takes one atomic per read)") \
    X(HAST_PART_SPAN, Int, 8, 13, Ignore, "", "by barcode count", "hast_ctx_create", "barcodes per bin of the partitioned bookkeeping, as bits") \
    X(HAST_MINIMIZER, Int, 1, 32, Ignore, "", "K <= 16: K, else max(16, K - 8)", "hast_ctx_create, hast_kc_create", "minimizer length of the bucket placement; at most K") \
    X(HAST_TRACE_INIT, Flag, 0, 0, Ignore, "", "off", "hast_ctx_create", "the time of every HIP call of a context's creation, on stderr") \
    X(HAST_FORCE_RCCL, Flag, 0, 0, Ignore, "", "off", "hast_counts_allreduce", "one GPU runs the RCCL path too (a 1-rank communicator): library loading, symbols, enum values") \
    X(HAST_PARK_GB, Real, 0, 1048576, Clamp, "", "32", "library, at the first park; classify: alias of --park-gb", "GB of closed streams' buffers that may wait before they are freed for real (0 = free at once: every free waits for all streams of the device)") \
    X(HAST_PARK_SITES, Int, -1, 2147483647, Ignore, "", "-1 (all)", "library, at the first park", "bit mask of the sites whose buffers are parked (bisecting)") \
    X(HAST_FQ_HOST_RECORDS, Size, 1, NOLIM, Clamp, "", "by the block size", "hast_fq_create", "records whose framing a block hands to the host in one piece (tests: force the copy path)") \
    X(HAST_GZ_TRACE, Flag, 0, 0, Ignore, "", "off", "hast_gz open, read, close; host inflate (par_inflate.h)", "per-batch timings of the inflate on stderr") \
    X(HAST_GZ_TRACE_JOBS, Flag, 0, 0, Ignore, "", "off", "hast_gz, every decode pass", "every pass's first jobs and all its candidates, on stderr") \
    X(HAST_GZ_SPLIT, Word, 0, 0, Ignore, "contexts", "a unit per GPU", "hast_gz open", "`contexts` gives every context of `--devices` a decode unit of its own even where contexts share a GPU (the several-GPU code on one GPU)") \
    X(HAST_GZ_CHUNK_BYTES, Size, 0, NOLIM, Clamp, "", "16K", "hast_gz open, where the caller passes no geometry", "compressed bytes per chunk of the device inflate (tests: many passes over a small file)") \
    X(HAST_GZ_PASS_CHUNKS, Size, 0, NOLIM, Clamp, "", "6144", "hast_gz open, where the caller passes no geometry", "chunks per decode pass") \
    X(HAST_GZ_AHEAD, Int, 0, 2, Clamp, "", "1", "hast_gz open", "further decode passes of a `.gz` file that run beside the one in front, each with a symbol arena of its own (0 = one at a time; 1: 7-14 % of the read phase for 2.8 GB more per open file; 2: another ~4 % for another 2.8 GB)") \
    X(HAST_GZ_ROOM, Real, 0, NOLIM, Ignore, "", "20", "hast_gz open, where the caller passes no room", "symbols of room per compressed byte of a chunk") \
    X(HAST_GZ_SLOT_FRACTION, Real, 0.01, 1, Clamp, "", "0.7, then what the passes find", "hast_gz open", "share of a pass's chunks that get a symbol slot (set: fixed)") \
    X(HAST_GZ_PIECE_BYTES, Size, 4096, 16777216, Clamp, "", "16M", "hast_gz open", "upload granule of a `.gz` file, rounded down to 4096 (tests use KB)") \
    X(HAST_GZ_RING_BYTES, Size, 0, NOLIM, Clamp, "", "2G", "hast_gz open; classify: alias of --gz-ring-bytes", "the ring a `.gz` file larger than it goes round on the device") \
    X(HAST_GZ_FREE_CUS, Int, 0, 65536, Clamp, "", "32", "hast_gz open", "CUs the device inflate's decode passes leave to the kernels behind them (0: none)") \
    X(HAST_BZ_BATCH_IN_BYTES, Size, 0, NOLIM, Clamp, "", "32M", "hast_gz_open_blocked, where the caller passes no geometry", "compressed bytes per batch of the blocked-gzip device inflate (`--bgzf device`)") \
    X(HAST_BZ_BATCH_OUT_BYTES, Size, 0, NOLIM, Clamp, "", "192M", "hast_gz_open_blocked, where the caller passes no geometry", "output bytes per batch of the blocked-gzip device inflate") \
    X(HAST_KC_COUNT, Word, 0, 0, Ignore, "atomic|partition", "by table size", "hast_kc_create", "stage 00: forces the direct or the partitioned counting path") \
    X(HAST_KC_FLUSH, Word, 0, 0, Ignore, "sweep|atomic", "by the number of records", "hast_kc_create", "stage 00: how a flush of records is applied") \
    X(HAST_KC_L1_SPLIT, Int, 1, 32, Clamp, "", "8", "hast_kc_create", "stage 00: regions per level-1 bin") \
    X(HAST_KC_RECORD_MB, Int, 0, 1048576, Ignore, "", "what is free next to the table", "hast_kc_create", "stage 00: caps the record buffer, in MB") \
    X(HAST_KC_FRESH, FlagDefaultOn, 0, 0, Ignore, "", "on", "hast_kc_create and every table reset", "stage 00: `0` clears a table before it is counted into (default: its first flush writes every slice)") \
    X(HAST_KC_TILE, Int, 256, 16384, Ignore, "", "by K and minimizer", "hast_kc_create", "stage 00: window starts per tile, rounded down to 32") \
    X(HAST_KC_EMIT, Word, 0, 0, Ignore, "lanes", "four lanes a window where they apply", "hast_kc count, every launch", "stage 00: `lanes` keeps the lane-per-window emit kernel for K = 17 ... 21 too") \
    X(HAST_KC_INGEST, Word, 0, 0, Ignore, "host|device", "host", "unshared_kmers: alias of --ingest", "stage 00: who inflates and frames the parents' reads") \
    X(HAST_KC_DEVICE_FASTA, Flag, 0, 0, Ignore, "", "off", "unshared_kmers: alias of --device-fasta", "stage 00: FASTA parents are framed on the GPU too") \
    X(HAST_KC_INGEST_BLOCK, Size, 64, NOLIM, Ignore, "", "16M", "unshared_kmers --ingest device", "stage 00: bytes per block of the device ingest (tests: blocks of a few hundred bytes)") \
    X(HAST_INFLATE, Word, 0, 0, Ignore, "device|host|zlib", "device", "every program, at each input it opens; alias of --inflate", "`host` keeps `.gz` inputs off the GPU, `zlib` inflates them with zlib on one thread") \
    X(HAST_BGZF_THREADS, Int, 1, 1024, Clamp, "", "an eighth of the hardware threads, 2 to 16", "host inflate, at each BGZF input", "threads that inflate one blocked-gzip input on the host") \
    X(HAST_GZ_THREADS, Int, 1, 1024, Clamp, "", "an eighth of the hardware threads, 2 to 8", "host inflate, at each `.gz` input", "threads that inflate one ordinary `.gz` input on the host (1 = the serial decoder)") \
    X(HAST_GZ_BUDGET, Int, 1, 1024, Clamp, "", "the CPU quota, else 16", "host inflate, at each `.gz` input", "inflate threads over all ordinary `.gz` inputs open at once") \
    X(HAST_TRACE_BLOCKS, Flag, 0, 0, Ignore, "", "off", "classify, barcode_freq: at the first block", "a line on stderr per block filled and submitted") \
    X(HAST_BGZF, Word, 0, 0, Ignore, "host|device", "host", "classify: alias of --bgzf", "who inflates blocked-gzip inputs; another word is a usage error, as for the flag") \
    X(HAST_ROWS, Word, 0, 0, Ignore, "host|device", "host", "classify: alias of --rows", "who sorts and formats the output table; another word is a usage error, as for the flag") \
    X(HAST_PHASE_READS, Flag, 0, 0, Ignore, "", "off", "classify: alias of --phase-reads", "the reads are routed to per-haplotype files") \
    X(HAST_PHASE_GZ, Flag, 0, 0, Ignore, "", "off", "classify: alias of --gz-out", "the routed files are written as gzip") \
    X(HAST_PHASE_GZ_FORMAT, Word, 0, 0, Ignore, "gzip|bgzf", "gzip", "classify: alias of --gz-format", "`bgzf` writes the routed files as blocked gzip; another word is a usage error, as for the flag") \
    X(HAST_DEAL, Word, 0, 0, Ignore, "blocks|files", "blocks", "classify: alias of --deal", "`files` makes `--devices` deal whole files instead of blocks") \
    X(HAST_NAME_CACHE, Size, 0, NOLIM, Clamp, "", "16M", "classify: alias of --name-cache", "ids the device-side barcode dictionary can hand out (0: the host names every barcode)") \
    X(HAST_NAME_DICT, Word, 0, 0, Ignore, "0|1|context", "1", "classify, before the streams are created", "`0` keeps the host's dictionary as the one that numbers the barcodes; `context` gives every context a dictionary even where contexts share a GPU") \
    X(HAST_TEARDOWN, Flag, 0, 0, Ignore, "", "off", "classify, at the end", "the process frees everything in order instead of leaving with _exit") \
    X(HAST_RS_BLOCK, Size, 64, NOLIM, Clamp, "", "--block-mb", "classify_read", "bytes per block of the read feed (tests: blocks of a few hundred bytes)") \
    X(HAST_READ_BLOCK_BYTES, Size, 1, NOLIM, Clamp, "", "256M", "classify_read, host route", "bytes per block the host parser reads") \
    X(HAST_TX_BLOCK, Size, 64, NOLIM, Ignore, "", "--block", "fake_10x, unless --block is given", "bytes per input block (tests: blocks of a few KB)") \
    X(HAST_BF_BLOCK, Size, 1, NOLIM, Ignore, "", "--block", "barcode_freq, unless --block is given", "bytes per input block (tests: blocks of a few hundred bytes)")

#define HAST_SW_ID(id, kind, lo, hi, policy, words, dflt, reader, desc) id,
enum Id { HAST_SWITCHES(HAST_SW_ID) kCount };
#undef HAST_SW_ID

struct Row {
    const char *name;
    Kind kind;
    double lo, hi;
    Policy policy;
    const char *words, *dflt, *reader, *desc;
};
#define HAST_SW_ROW(id, kind, lo, hi, policy, words, dflt, reader, desc) {#id, kind, (double)(lo), (double)(hi), policy, words, dflt, reader, desc},
constexpr Row kRows[kCount] = {HAST_SWITCHES(HAST_SW_ROW)};
#undef HAST_SW_ROW

// the variable's text as it stands, or null: for the programs' aliases that hold the value to the rule of their flag (a wrong word
// is the usage text), and for printing what was set
inline const char *text(Id id) { return getenv(kRows[id].name); }

inline void ignored(Id id, const char *value) {
    static std::atomic<bool> said[kCount];
    if (said[id].exchange(true)) return;
    const Row &r = kRows[id];
    const char *kind = r.kind == Size ? "a count (digits, then at most one of K, M, G)" : r.kind == Int ? "an integer" : "a number";
    char what[160];
    if (r.kind == Word) snprintf(what, sizeof(what), "one of %s", r.words);
    else if (r.hi >= NOLIM) snprintf(what, sizeof(what), "%s of %.10g or more", kind, r.lo);
    else snprintf(what, sizeof(what), "%s in [%.10g, %.10g]", kind, r.lo, r.hi);
    fprintf(stderr, "hast: %s=%s is not %s; ignored\n", r.name, value, what);
}

// Flag: on iff the value is non-empty and not exactly 0.  FlagDefaultOn: off iff the value is exactly 0.
inline bool flag(Id id) {
    const char *e = text(id);
    if (kRows[id].kind == FlagDefaultOn) return !(e && !strcmp(e, "0"));
    return e && *e && strcmp(e, "0") != 0;
}

// The numbers: true = the variable is set to what the row takes, and *out is it (clamped where the row says so); else *out is
// untouched.  take: v as parsed from the text e, or not parsed, against the row's range.
template <class V, class T>
inline bool take(Id id, const char *e, bool parsed, V v, T *out) {
    const Row &r = kRows[id];
    const bool below = (double)v < r.lo, above = r.hi < NOLIM && (double)v > r.hi;
    if (!parsed || ((below || above) && r.policy == Ignore)) return ignored(id, e), false;
    *out = (T)(below ? (V)r.lo : above ? (V)r.hi : v);
    return true;
}
template <class T>
inline bool integer(Id id, T *out) {
    const char *e = text(id);
    if (!e) return false;
    errno = 0;
    char *end = nullptr;
    const long long v = strtoll(e, &end, 10);
    return take(id, e, !errno && end != e && !*end && !isspace((unsigned char)*e), v, out);
}
template <class T>
inline bool size(Id id, T *out) {
    const char *e = text(id);
    if (!e) return false;
    uint64_t v = 0;
    const bool parsed = parse_count(e, &v);                    // (before v is handed on)
    return take(id, e, parsed, v, out);
}
inline bool real(Id id, double *out) {
    const char *e = text(id);
    if (!e) return false;
    errno = 0;
    char *end = nullptr;
    const double v = strtod(e, &end);
    return take(id, e, !errno && end != e && !*end && !isspace((unsigned char)*e) && std::isfinite(v), v, out);
}

// the index of the value among the row's words, -1: unset or none of them
inline int word(Id id) {
    const char *e = text(id);
    if (!e) return -1;
    const size_t n = strlen(e);
    int i = 0;
    for (const char *w = kRows[id].words; n && *w; ++i) {
        const char *bar = strchr(w, '|');
        const size_t len = bar ? (size_t)(bar - w) : strlen(w);
        if (len == n && !memcmp(w, e, n)) return i;
        w += len + (bar ? 1 : 0);
    }
    return ignored(id, e), -1;
}
inline bool word_is(Id id, const char *w) {                   // the value is this word of the row
    return word(id) >= 0 && !strcmp(text(id), w);
}

// a profiler is listening (rocprofv3 preloads its tool library and writes its files when the process ends in an orderly way)
inline bool profiler_listening() {
    const char *preload = getenv("LD_PRELOAD");
    return getenv("ROCP_TOOL_LIBRARIES") || (preload && strstr(preload, "rocprofiler"));
}

}  // namespace sw
}  // namespace hast
