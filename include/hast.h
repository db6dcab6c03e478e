/*
 * hast.h -- C ABI of libhast.so, the MI355X-native (gfx950) implementation of HAST's stage-01
 * read-classification hot path.
 *
 * What it replaces.  The reference has no FFI for this path: it is a process
 * (`01.classify_stlfr_reads/classify`, argv in / TSV on stdout, classify.cpp:373-450).  The
 * drop-in boundary is therefore the `classify` executable built from hast_amd/csrc/classify_main.cpp,
 * and THIS header is the seam between that host program (and bench.py / pytest via ctypes) and
 * the HIP device code.  Each entry point cites the reference code whose work it takes over
 * (paths relative to /root/reference/01.classify_stlfr_reads/).
 *
 * Conventions
 *   - plain C types only; every call returns a hast_status and never throws across the ABI;
 *     hast_last_error() gives a thread-local message for the last failing call.
 *   - the caller owns host buffers; pointers named d_* are DEVICE pointers (from hast_dev_alloc
 *     or from any other allocator on the same device, e.g. a torch tensor's data_ptr()).
 *   - one context per device; calls on one context are serialised by the caller.
 *   - hast_stream is a hipStream_t passed as void* (NULL = the context's own stream).  A context has ONE set of launch
 *     scratch (tile queue, segment table, vote scratch): at most one classification of a context may be in flight, i.e. all
 *     classify calls of a context must go to the same stream (any stream, but one).
 *   - there is NO CPU fallback: with no usable GPU hast_ctx_create fails with HAST_ERR_NO_DEVICE.
 */
#ifndef HAST_H
#define HAST_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    HAST_OK = 0,
    HAST_ERR_INVALID = 1,    /* bad argument / K out of [1,32] / wrong call order            */
    HAST_ERR_NO_DEVICE = 2,  /* no HIP device, or the device is not usable                  */
    HAST_ERR_HIP = 3,        /* a HIP runtime call failed (message in hast_last_error)      */
    HAST_ERR_OOM = 4,        /* host or device allocation failed                            */
    HAST_ERR_TABLE_FULL = 5, /* more distinct keys than hast_table_reserve planned for      */
    HAST_ERR_FORMAT = 6,     /* k-mer text is not fixed-width K-byte lines (kmer.h:154)     */
    HAST_ERR_RCCL = 7,       /* the RCCL all-reduce failed                                  */
    HAST_ERR_IO = 8,         /* file could not be opened / read / is damaged                */
    HAST_ERR_UNSUPPORTED = 9 /* this entry cannot take this input; another one can (e.g. hast_gz_open: inflate on the host) */
} hast_status;

typedef struct hast_ctx hast_ctx;
typedef void *hast_stream;

const char *hast_version(void);
const char *hast_last_error(void);

/* ---- context ------------------------------------------------------------------------------
 * Holds what the reference keeps in process globals: g_K (classify.cpp:29), g_kmers[2]
 * (classify.cpp:27) as ONE merged open-addressed table in HBM, and the per-barcode counters
 * (BarcodeCache, classify.cpp:50-64).  k in [1,32] (the reference's correct range; at k = 32 a key
 * fills the 64-bit slot, so the table is two tag-less per-haplotype tables and every window is probed twice). */
hast_status hast_ctx_create(int device_ordinal, int k, hast_ctx **out);
void        hast_ctx_destroy(hast_ctx *);
/* Streams that are closed (hast_fq_destroy, hast_gz_close) PARK their device and pinned buffers instead of freeing them: a free waits
 * for every stream of the device, i.e. stalls the streams that are still at work.  The parked memory is freed for real here, by
 * hast_ctx_destroy, when more than HAST_PARK_GB (environment, default 32; 0 = free at once) are waiting, or when a stream's allocation fails.  No reference
 * counterpart (the reference's streams are host objects). */
void        hast_release_parked(void);
int         hast_ctx_k(const hast_ctx *);
/* Tuning: length m of the minimizer that places a key's bucket (see hast_common.h).  Defaults to
 * K for K<=16, else max(16, K-8).  May only be changed before hast_table_reserve. */
int         hast_ctx_minimizer(const hast_ctx *);
hast_status hast_ctx_set_minimizer(hast_ctx *, int m);
int         hast_ctx_device(const hast_ctx *);
/* Measurement switches.  The environment is read ONCE, when a context is created (HAST_CLASSIFY, HAST_FILTER_*, HAST_COMMIT,
 * HAST_PART_SPAN, HAST_F_GEO, HAST_F_RL, HAST_TILE_LDS, HAST_MINIMIZER, HAST_COUNT_LOOKUPS); results never depend on them.  hast_ctx_set_option changes one on a live
 * context: "commit" 0 = by batch size / 1 = one atomic per read / 2 = partitioned; "part_span" 8 .. 13 = barcodes per bin of the
 * partitioned commit as a power of two (0 = by barcode count); "kernel_geo", "kernel_rl" 0 = the generic
 * k_classify_f instantiations instead of the ones with the BASELINE geometry / row length compiled in; "tile_lds" bytes (0 =
 * default); "filter_exact_once" 1 = exact filter entries filed once per strand (see hast_ctx_set_filter).  hast_ctx_options writes the switches that differ from their defaults as "name=value ..." ("" = none). */
hast_status hast_ctx_set_option(hast_ctx *, const char *name, long value);
hast_status hast_ctx_options(const hast_ctx *, char *out, size_t cap);
hast_stream hast_ctx_stream(const hast_ctx *);
hast_status hast_stream_sync(hast_ctx *, hast_stream);

/* ---- raw device memory (for callers without another allocator, e.g. ctypes tests) ---------- */
hast_status hast_dev_alloc(hast_ctx *, size_t bytes, void **d_out);
hast_status hast_dev_free(hast_ctx *, void *d_ptr);
/* free and total memory of the context's device, and the bytes closed streams have parked (hast_release_parked): what `classify --stats`
 * samples for its HBM head-room line.  Any of the three may be NULL. */
hast_status hast_dev_mem_info(hast_ctx *, size_t *free_bytes, size_t *total_bytes, size_t *parked_bytes);
hast_status hast_memcpy_h2d(hast_ctx *, void *d_dst, const void *src, size_t bytes);
hast_status hast_memcpy_d2h(hast_ctx *, void *dst, const void *d_src, size_t bytes);
hast_status hast_memset_d(hast_ctx *, void *d_dst, int byte, size_t bytes, hast_stream);

/* ---- the k-mer table: g_kmers[0], g_kmers[1] (classify.cpp:27) -----------------------------
 * One table, slot = (canonical_key << 2) | tags, tag bit h set <=> key in haplotype h's set.
 * Buckets of 8 slots = 64 B; home bucket from the hash of the key's minimizer (consecutive windows of
 * a read then mostly share a bucket line); a key whose home bucket is full goes to a bucket chosen by the key's own
 * hash and walks on from there (hast_common.h: overflow_bucket / next_bucket). */

/* Size the table for up to `max_keys` distinct keys (both haplotypes together) at the given
 * load factor (0 => 0.2: 288 GB of HBM make a sparse table free, and full buckets rare).  Discards
 * any previous table. */
hast_status hast_table_reserve(hast_ctx *, uint64_t max_keys, double load_factor);

/* load_kmers (classify.cpp:30-46) on an in-memory image of the file: '\n'-separated K-byte lines,
 * parsed, canonicalised (Kmer::str2Kmer, kmer.h:153-166) and inserted ON THE DEVICE.  A final piece
 * without '\n' is dropped (classify.cpp:41).  *lines_out = number of lines used ("Recorded N").
 * HAST_ERR_FORMAT if any line is not exactly K bytes (the reference asserts, kmer.h:154). */
hast_status hast_table_insert_text(hast_ctx *, int hap, const char *text, size_t nbytes,
                                   uint64_t *lines_out);
/* The same straight from a regular FILE, streamed (several threads pread the next piece into pinned memory while the
 * previous one is inserted): 2 x 4.4 GB of 21-mer text load in well under a second instead of at one thread's read rate.
 * HAST_ERR_IO if the path cannot be opened or is not a regular file (a pipe: read it and use hast_table_insert_text). */
hast_status hast_table_insert_text_file(hast_ctx *, int hap, const char *path, uint64_t *lines_out);
/* acgt_only != 0: both calls above also fail with HAST_ERR_FORMAT when a line holds a byte other than upper-case A/C/G/T
 * (checked on the device).  Stage 01 accepts any byte (kmer.h:11 codes them all); the stage-03 classifier compares k-mers
 * as case-sensitive strings (S03/src_main/classify.cpp:59-65), which integer keys reproduce only for such lines. */
hast_status hast_ctx_set_text_check(hast_ctx *, int acgt_only);
/* Same, keys already canonical 2K-bit values (host / device resident). */
hast_status hast_table_insert_keys(hast_ctx *, int hap, const uint64_t *canon_keys, size_t n);
hast_status hast_table_insert_keys_device(hast_ctx *, int hap, const uint64_t *d_canon_keys, size_t n,
                                          hast_stream);

/* InitAdaptor (classify.cpp:314-339): remove each key from BOTH sets.  out_hit[i] (optional) gets
 * bit h set when key i was present in haplotype h's set (the reference logs one INFO line each). */
hast_status hast_table_erase(hast_ctx *, const uint64_t *canon_keys, size_t n, uint8_t *out_hit);

/* g_kmers[h].size() as used by getHap (classify.cpp:70-71): distinct canonical keys per haplotype
 * after any erase. */
hast_status hast_table_sizes(hast_ctx *, uint64_t *n_hap0, uint64_t *n_hap1);

/* Membership of host keys (test/diagnostic entry): out_tags[i] = tag bits of key i (0 = absent). */
hast_status hast_table_lookup(hast_ctx *, const uint64_t *canon_keys, size_t n, uint8_t *out_tags);

/* Binary key-set cache (so the multi-GB k-mer text files are parsed once): hast_table_save writes the live keys
 * with their tag bits (8 B per distinct key, sorted; both sets, after any erase) to `path`; hast_table_load sizes a
 * new table for them (load factor as in hast_table_reserve) and re-inserts them.  K must match the context. */
hast_status hast_table_save(hast_ctx *, const char *path);
hast_status hast_table_load(hast_ctx *, const char *path, double load_factor);
hast_status hast_table_file_info(const char *path, int *k_out, uint64_t *n_keys_out);   /* no GPU needed */

/* Replicate src's finished table (and its filter) onto dst's device with one peer copy (xGMI), instead of building it
 * once per GPU: what the multi-GPU classify CLI does after building the table on its first device.  Same K required;
 * dst's previous table is discarded. */
hast_status hast_table_clone(hast_ctx *dst, hast_ctx *src);

/* geometry, for roofline accounting */
hast_status hast_table_info(const hast_ctx *, uint64_t *n_buckets, uint64_t *bytes);

/* ---- the fingerprint filter in front of the table ----------------------------------------------
 * What hast_classify_* actually probes (hast_amd/csrc/hast_common.h): 16-bit prints of every key,
 * in 128-B blocks named by a forward mod-minimizer of the key's string and of its reverse complement, so that the
 * consecutive windows of a read ask for few blocks.  A window the filter cannot rule out is looked up in the table
 * above, which alone decides hits, so results never depend on the filter.  It is (re)built from the table's live keys
 * by the first classification after keys were added, or explicitly by hast_filter_build (e.g. outside a timed region).
 * The geometry follows the key count: 4^m blocks with m up to 15 (137 GB, chosen above 537M keys; 4^14 = 34 GB below that and
 * when HBM has no room), a print filed in the less loaded of two sub-buckets where blocks are crowded, in one where they hold
 * <= 2.2 strings on average (the probe then loads and compares one sub-bucket per window).
 * Where a filed string fits a 16-bit entry EXACTLY (its block is a bijection of the sampled m-mer, the entry holds the rest:
 * 2(K-m) + log2(W) <= 17 bits, e.g. K = 21 with m = 14) the entries are exact codes + the key's tag bits instead of prints,
 * and a match in the filter IS the hit: only windows that land in a full sub-bucket still ask the table.  Same results.
 * hast_ctx_set_filter: enable = 0 probes the table directly (the round-1 kernel; also HAST_CLASSIFY=exact in the
 * environment), 1 = filter, exact entries where they fit, 2 = filter with prints always (also HAST_FILTER_EXACT=0); m (sampled
 * m-mer, 4^m blocks), t (ordering t-mer), kp (bases of a window the sampling looks at) = 0 picks the geometry from K and
 * the key count.  hast_filter_info: *enabled = 0 off, 1 prints, 2 exact entries (known once the filter is built).
 * Exact entries are filed DENSELY -- under every one of a string's W = K-m+1 m-mers instead of under one sampled m-mer -- where W
 * is a power of two <= 8 and the sub-buckets then hold <= 3.2 entries on average (K = 21 up to ~430M keys): the probe takes the
 * m-mer on a fixed grid of the row, ceil(windows / W) blocks per read, no sampling arithmetic.  A dense entry sits in the sub-bucket
 * of its m-mer's position, and a sub-bucket that turned entries away says which (a signature in its mark), so nearly no window
 * without a match has to ask the table.  HAST_FILTER_EXACT=once in the
 * environment (hast_ctx_set_option "filter_exact_once") keeps exact entries filed once per strand under the sampled m-mer.
 * hast_filter_dense: *dense = 1 when the filter built for the current table is a dense one.  Same results either way. */
hast_status hast_ctx_set_filter(hast_ctx *, int enable, int m, int t, int kp);
hast_status hast_filter_build(hast_ctx *);
hast_status hast_filter_info(const hast_ctx *, int *enabled, int *m, int *t, int *kp, uint64_t *bytes);
hast_status hast_filter_dense(const hast_ctx *, int *dense);
/* Measurement entry (bench.py's roofline): requests per second at which this GPU serves uniformly random 128-B blocks of the
 * context's own filter, read in the probe kernel's access shape with no arithmetic -- the request-rate ceiling of this box
 * over this footprint, against which k_classify_f's own request rate is priced in the same run. */
hast_status hast_filter_request_ceiling(hast_ctx *, double *requests_per_s);
/* Measurement entry: the windows k_classify_f has sent to the exact table on this context since it was created, for filters
 * with exact entries (windows without a match in a sub-bucket whose mark says a key like theirs was turned away; filters with
 * prints send every hit there and are not counted).  Counted only when
 * HAST_COUNT_LOOKUPS=1 was in the environment at hast_ctx_create (one atomic per 64 look-ups); an error otherwise. */
hast_status hast_filter_lookups(hast_ctx *, uint64_t *n);

/* ---- per-barcode counters: BarcodeCache (classify.cpp:50-64) -------------------------------
 * Device layout: uint64 counts[n_barcodes][4] = { c0, c1, neg, reserved } (32-byte records: a record is one sector for the commit
 * kernels' updates; what leaves the GPU -- the all-reduce, the copy to the host -- is the three live words, see hast_counts_pack):
 *   c0/c1 = sum of per-read votes for key 0/1 (classify.cpp:203-206), neg = key -1 (:191,:207-208).
 * A barcode was "seen" (gets an output row, classify.cpp:94) iff c0|c1|neg != 0.
 * 64-bit accumulation on the device, narrowed by whoever prints ("Hot barcode"): the reference counts in `int`
 * (classify.cpp:51), which the no-barcode bucket "0_0_0" -- 10-20 % of real stLFR reads -- overflows on large runs (undefined
 * there).  Here no counter wraps and none carries into its neighbour, whichever commit path a batch takes: one atomic per
 * counter and read (k_commit_votes), or, for large device-resident batches over many barcodes, pairs grouped by barcode range and
 * summed in LDS, then plain adds by the one workgroup that owns the range (hast_ctx_set_option "commit" / HAST_COMMIT=
 * atomic|partition at context creation force either; same sums).  The classify program prints the exact count and warns when it
 * is above INT_MAX.
 * Exclusivity: while a classification of a context is in flight nothing else may update the counters it is bound to -- the
 * partitioned path adds with plain read-modify-writes.  Two contexts (or two streams) may share a caller-owned buffer only if
 * their classify calls do not overlap in time. */
hast_status hast_counts_resize(hast_ctx *, size_t n_barcodes);                 /* library-owned, zeroed */
hast_status hast_counts_bind(hast_ctx *, uint64_t *d_counts, size_t n_barcodes); /* caller-owned buffer, 32-byte aligned */
hast_status hast_counts_zero(hast_ctx *, hast_stream);
hast_status hast_counts_read(hast_ctx *, uint64_t *c0, uint64_t *c1, uint64_t *neg, size_t n_barcodes);
/* the same for records [first, first + n): a job whose ids come from two numberings (a device dictionary from 0, the host's above
 * hast_names_limit) reads the two ranges that exist */
hast_status hast_counts_read_range(hast_ctx *, size_t first, size_t n, uint64_t *c0, uint64_t *c1, uint64_t *neg);
/* The three live words of the first n_barcodes records as three arrays, d_packed = c0[n] | c1[n] | neg[n] (3 x n_barcodes u64, device),
 * and back (the records' three words are overwritten, the reserved one is left alone): what a caller that runs its own collective --
 * bench.py: one torch.distributed all_reduce over RCCL -- moves is 24 bytes per barcode, not the 32 of the padded records;
 * hast_counts_read and hast_counts_allreduce do the same inside.  Asynchronous on `stream`. */
hast_status hast_counts_pack(hast_ctx *, uint64_t *d_packed, size_t n_barcodes, hast_stream);
hast_status hast_counts_unpack(hast_ctx *, const uint64_t *d_packed, size_t n_barcodes, hast_stream);
/* The bookkeeping alone (classify.cpp:203-208) for per-read votes the caller holds: d_votes[n_reads][2] = (vote0, vote1), 8-byte
 * aligned; d_barcode_ids[n_reads] < n_barcodes; max_votes = an upper bound on any single vote (reads of up to 255 windows may take
 * the partitioned path).  Asynchronous on `stream`. */
hast_status hast_counts_add_votes(hast_ctx *, const uint32_t *d_votes, const uint32_t *d_barcode_ids, size_t n_reads,
                                  uint32_t max_votes, hast_stream);
/* Thread-merge of the reference (collectBarcodes/BarcodeCache::Add, classify.cpp:57-63,226-229)
 * across the GPUs of ONE process: a single in-place RCCL all-reduce(sum,u64) over the counters of
 * n_ctx contexts (same n_barcodes).  Contexts that share a device (a logical split: --devices 0,0 or 0,0,1,1) are summed by a kernel
 * on that device into its first context first; the all-reduce then runs over one context per distinct device (none when there is
 * only one), and the totals are handed back to every context.  The communicators of a device list
 * are created by the first call that names it and kept until the process ends (later calls only enqueue the all-reduce). */
hast_status hast_counts_allreduce(hast_ctx *const *ctxs, int n_ctx);
/* New counters of n_new records (zeroed): record i < n_perm of the old ones is ADDED to record perm[i] (perm: host array; several old
 * records may name one new record; 0xFFFFFFFF: dropped), the old records from n_perm on keep their places.  How contexts whose
 * dictionaries numbered the barcodes differently -- one device dictionary per GPU -- are brought into one id space (hast_names_merge
 * gives perm) before hast_counts_allreduce sums them. */
hast_status hast_counts_permute(hast_ctx *, const uint32_t *perm, size_t n_perm, size_t n_new);

/* ---- classification: MultiThread::process_reads (classify.cpp:186-209) ---------------------
 * For each read: whole-read skip when it holds an upper-case 'N' (containN, :182-185,190-193);
 * otherwise every window of K bases is 2-bit coded ((c&6)>>1, kmer.h:11), canonicalised
 * (kmer.h:169-194) and looked up in both sets (:195-202); votes go to the read's barcode (:203-208).
 *
 *   d_bases        ASCII bases of all reads, back to back (device)
 *   d_offsets      n_reads+1 byte offsets into d_bases, or NULL => fixed length: read i at i*read_len
 *   read_len       fixed read length (d_offsets==NULL) or an upper bound on every read's length
 *   d_barcode_ids  per-read dense barcode id (< n_barcodes), or NULL => counters untouched
 *   d_votes        optional [n_reads][2] per-read (vote0, vote1) output (per-read mode), 8-byte aligned, or NULL
 *   bases_bytes    total bytes readable at d_bases.  The kernel loads whole aligned dwords: up to 3 bytes in front of
 *                  d_bases (when it is not 4-byte aligned) and up to 3 bytes behind d_bases + bases_bytes are loaded and
 *                  ignored; they must be mapped device memory, which holds for any pointer into an allocation made by
 *                  hipMalloc or a sub-allocator with >= 4-byte granules (torch's: 512 B).
 * A read shorter than K has no windows (the reference aborts, kmer.h:171): it votes 0/0.
 * Reads of any length: with read_len > 4096 (with or without d_offsets) the reads are cut into segments on the device (same
 * result; the segment count stays on the device, nothing waits for the host).
 * Asynchronous on `stream`.  Per call: the probes (k_classify_f) write per-read votes -- to d_votes, or to library scratch that
 * grows on demand (a larger batch than ever before synchronises once) -- and a second step turns them into the per-barcode
 * counters: one atomic per read (k_commit_votes), or, for batches of >= 2M reads over many barcodes, the pairs grouped by barcode
 * range and summed in LDS (k_commit_partition + k_commit_bins) -- DESIGN.md section 3: updates interleaved with the probes' reads
 * cost four times as much, hence kernels of their own. */
hast_status hast_classify_device(hast_ctx *, const uint8_t *d_bases, size_t bases_bytes,
                                 const uint64_t *d_offsets, uint32_t read_len,
                                 const uint32_t *d_barcode_ids, uint32_t *d_votes,
                                 size_t n_reads, hast_stream);
/* Kernel timing for measurements (bench.py's roofline): with n_slots > 0 every hast_classify_device call records HIP
 * events around its two kernels (k_classify, k_commit_votes) on the launch stream, for the last n_slots calls;
 * hast_classify_times waits for them and returns the durations in call order (ms), oldest first, and forgets them. */
hast_status hast_classify_timing(hast_ctx *, int n_slots);
hast_status hast_classify_times(hast_ctx *, float *classify_ms, float *commit_ms, int max, int *n_out);
/* Same with HOST buffers: staged to the device through the context's pinned double buffer
 * (what the classify CLI uses).  Returns once the batch is enqueued; buffers may be reused on return. */
hast_status hast_classify_batch(hast_ctx *, const uint8_t *bases, const uint64_t *offsets,
                                const uint32_t *barcode_ids, size_t n_reads, uint32_t max_read_len);

/* Per-read mode (BASELINE config 5; reference: the per-read classifier of stage 03,
 * 03.mkoutput_by_fabulous2.0/src_main/classify.cpp:203-218): no barcodes, no whole-read N skip; a window
 * counts for haplotype h when its K bytes are upper-case A/C/G/T and its canonical k-mer is in set h (== the
 * reference's string lookup of the window against every k-mer line and its reverse complement, given
 * upper-case ACGT k-mer lines).  Reads may have any length (20 kb PacBio-style reads are cut into segments on
 * the device).  d_votes[n_reads][2] is overwritten with (hits0, hits1). */
hast_status hast_classify_perread_device(hast_ctx *, const uint8_t *d_bases, size_t bases_bytes,
                                         const uint64_t *d_offsets, size_t n_reads, uint32_t *d_votes, hast_stream);
/* Same with host buffers, synchronous (H2D, classify, D2H of the votes). */
hast_status hast_classify_perread(hast_ctx *, const uint8_t *bases, const uint64_t *offsets, size_t n_reads,
                                  uint32_t *votes_out);

/* Zero-copy variant for host-fed callers (the CLI's parser threads write straight into pinned memory):
 * hast_batch_begin hands out the pinned staging arrays of the next batch (waiting for that buffer's previous
 * batch to finish on the GPU); the caller fills bases back to back, offsets[0..n_reads] and barcode ids, then
 * hast_batch_submit enqueues H2D + classification.  Capacities: bases_capacity bytes, reads_capacity reads. */
hast_status hast_batch_begin(hast_ctx *, size_t bases_capacity, size_t reads_capacity,
                             uint8_t **bases, uint64_t **offsets, uint32_t **barcode_ids);
hast_status hast_batch_submit(hast_ctx *, size_t n_reads, uint32_t max_read_len);

/* ---- FASTQ framing on the GPU: processFastq (classify.cpp:238-278) --------------------------------
 * The reference's producer thread reads a record as four getlines (no '@'/'+' validation, no CR stripping), takes the
 * barcode out of line 1 (parseName, :112-119) and hands line 2 to a worker.  hast_fq does that framing for whole blocks of
 * raw file bytes on the device: the caller only moves bytes (pread / inflate straight into the pinned buffer it is given)
 * and names barcodes; the reads are classified where they lie in the raw block.  Per block, in this order:
 *     hast_fq_acquire   pinned host memory for the next block_bytes of the file (waits until that buffer is free again)
 *     hast_fq_submit    n_bytes are in it; last != 0: the file ends here (the EOF rules of classify.cpp:257-268 apply:
 *                       a final record counts when its header line is terminated).  Enqueues the copy and the framing.
 *     hast_fq_next      oldest submitted block: waits for its record table (hast_fq_poll tells whether it is there), starts the classification of its reads, and
 *                       gives the barcode text extents of its records: record i's barcode = bytes[bc_pos[i] .. +bc_len[i])
 *     (caller)          ids[i] = dense id of that barcode (one dictionary per job, shared by all GPUs; < n_barcodes of
 *                       the context's counters)
 *     hast_fq_commit    copies the ids over and runs the per-barcode bookkeeping (classify.cpp:203-208); frees the buffer
 * Blocks may be submitted ahead of hast_fq_next (n_buffers of them); records that straddle two blocks are handled on the
 * device (the unfinished tail of a block is put in front of the next one), up to 4 MB per record.  After a block submitted
 * with last != 0 the next one starts a new file.  One hast_fq per input stream; several may share a context. */
typedef struct hast_fq hast_fq;
typedef struct {
    uint64_t n_records;        /* records framed in this block */
    uint64_t n_bases;          /* sum of their base-line lengths */
    uint32_t max_read_len;
    uint32_t short_read;       /* != 0: some read is shorter than K and holds no 'N' (the reference aborts, kmer.h:171);
                                  nothing of this block has been classified */
    const uint8_t *bytes;      /* host view of the block (with the previous block's tail in front of it); NULL for a block submitted
                                  with hast_fq_submit_device (hast_fq_block_host_bytes fetches it) */
    const uint32_t *bc_pos;    /* [n_records] */
    const uint32_t *bc_len;    /* [n_records] */
    const uint8_t *bc_text;    /* [n_records][16] or NULL: the barcode text itself, byte 0 = its length, bytes 1.. = the text;
                                  length byte 0xFF = longer than 15 bytes, take it from bytes[bc_pos ..) */
    uint32_t *ids;             /* [n_records]: ids the device-side name cache knew are filled in; the caller fills the others */
    const uint32_t *unknown;   /* [n_unknown] indices of the records whose ids the caller has to fill in, or NULL: all of them */
    uint64_t n_unknown;
    uint64_t dict_ids;         /* a stream over a device dictionary (hast_names_create_dict): ids it had handed out when this block was
                                  named -- every id of the block is below; the caller's counters must hold them before hast_fq_commit */
} hast_fq_block;
/* Device-side cache barcode text -> id of one GPU, shared by the FASTQ streams of all contexts on that GPU: barcodes repeat (hundreds of
 * reads each), so after the first blocks the framer names almost every record itself and the host only sees new barcodes
 * (and the ones longer than 15 bytes).  The ids still come from the caller's dictionary -- one per job, the same on every
 * GPU -- and hast_fq_commit teaches the cache what the caller named.  max_barcodes sizes it (2 x 32 B per barcode); more
 * barcodes than that are simply not cached. */
typedef struct hast_names hast_names;
hast_status hast_names_create(hast_ctx *, size_t max_barcodes, hast_names **out);
/* The table as the job's DICTIONARY on its GPU (round 6; classify.cpp:52-56: a barcode gets its map entry at its first sighting): the
 * framer's naming kernel hands out the dense ids itself -- 0 .. hast_names_limit() - 1 in the order in which new texts are met, one atomic
 * counter -- so no first sighting goes through the host.  Left to the caller (hast_fq_block.unknown, as before): texts longer than 15
 * bytes and what arrives once every id is out; the caller names those in an id range of its own at or above hast_names_limit().
 * AT EXHAUSTION the dictionary gives ONE ANSWER PER TEXT: a text of at most 15 bytes either has a device id -- then every record that
 * carries it, in this block and in every later one, on whichever context of the GPU, comes back with that id -- or it has none and
 * never will, and every record that carries it is left to the caller.  No text is ever numbered by both sides, also not in the
 * block(s) in which the last ids go, so one dictionary plus the caller's range is one numbering without a merge by text.  (That holds
 * per dictionary: a caller that runs SEVERAL -- one per GPU -- may see a text left to it by one that has run out and numbered by
 * another that has not, and must sum such rows by text itself.)  Nothing of at most 15 bytes is left to the caller before
 * hast_fq_block.dict_ids has reached hast_names_limit().
 * hast_names_count: ids handed out so far; hast_names_texts: the text records (16 bytes: length byte + text) of ids [first, first + n),
 * read once at the end for printing.  Dictionaries of different GPUs number independently: their counters are merged by text
 * (hast_names_merge into the first dictionary's numbering, hast_counts_permute, then hast_counts_allreduce). */
hast_status hast_names_create_dict(hast_ctx *, size_t max_barcodes, hast_names **out);
size_t      hast_names_limit(const hast_names *);
hast_status hast_names_count(hast_names *, size_t *n_ids);
hast_status hast_names_texts(hast_names *, size_t first, size_t n, uint8_t *out16);
/* Two dictionaries, one numbering: ids_out[i] = the id that dst has for src's text of id first + i (i < n) -- a text dst does not know
 * yet gets dst's next id there and then.  On the GPU: src's text records are copied to dst's device (peer to peer when that is another
 * GPU) and go through dst's naming kernel; no host map.
 * HAST_ERR_TABLE_FULL when dst has no id left for some new text.  ids_out is then COMPLETE all the same: the entries of the texts dst
 * knows or could still take hold their ids (below hast_names_limit(dst), dense as ever), the entries of the texts that did not fit
 * hold HAST_NAME_NONE.  Nothing is undone and nothing is lost: dst keeps what it took, the same call again returns the same status
 * and the same ids_out, and the caller numbers the HAST_NAME_NONE texts itself (hast_names_texts(src, ...) has them), as it does
 * for what a stream leaves to it. */
#define HAST_NAME_NONE 0xFFFFFFFFu
hast_status hast_names_merge(hast_names *dst, hast_names *src, size_t first, size_t n, uint32_t *ids_out);
void        hast_names_destroy(hast_names *);
/* Entries the caller knows: n text records (16 bytes each: length byte + up to 15 bytes of text, the format of hast_fq_block.bc_text)
 * with their ids -- e.g. a table barcode -> class for a routing stream (hast_fq_set_route).  Returns when they are on the device. */
hast_status hast_names_insert(hast_names *, const uint8_t *text16, const uint32_t *ids, size_t n);
hast_status hast_fq_create(hast_ctx *, size_t block_bytes, int n_buffers, hast_names *names_or_null, hast_fq **out);
/* device_blocks != 0: a stream of device-side blocks only (hast_fq_device_block / hast_fq_submit_device, below): no pinned host
 * copy of the block buffers is set up (hast_fq_acquire hands out NULL), which saves ~0.1 s of page pinning per stream. */
hast_status hast_fq_create_ex(hast_ctx *, size_t block_bytes, int n_buffers, hast_names *names_or_null, int device_blocks, hast_fq **out);
/* The blocks of ONE input stream on several contexts in turn (block i -> ctxs[i % n_ctx], one context per GPU; several
 * contexts on one GPU also work): the reference spreads the reads of one file over all its workers (classify.cpp:211-219),
 * one process per file would leave all GPUs but two idle on HAST's two input files (HAST.sh:162-166).  A block is framed
 * on its own GPU from the number of newlines in front of it in the file -- each block's own count is a kernel queued behind
 * its upload, the host adds them up -- so no GPU waits for another one's framing.  A block owns the records that START in
 * it; their header and base lines may reach into the first bytes of the next block (at most min(1 MB, block_bytes): a
 * larger record is HAST_ERR_FORMAT), which are uploaded to both GPUs.  Differences to hast_fq_create streams: every block
 * but the last of a file must be full (n_bytes == hast_fq_block_bytes), and a block can be opened (hast_fq_poll /
 * hast_fq_next) once the block behind it has been submitted.  n_buffers_per_ctx >= 2 and at least 3 buffers in all.  names: one
 * cache per context, or NULL. */
hast_status hast_fq_create_striped(hast_ctx *const *ctxs, int n_ctx, size_t block_bytes, int n_buffers_per_ctx,
                                   hast_names *const *names_or_null, hast_fq **out);
/* device_blocks != 0: a striped stream of device-side blocks (hast_fq_device_block / hast_fq_submit_device) -- what a .gz file
 * inflated on the GPUs feeds (hast_gz_open_multi): block i's bytes are written on GPU i % n_ctx by the caller's kernels, the first
 * bytes of block i + 1 reach block i's view by a copy from that GPU to this one, no pinned host copy of the blocks is set up. */
hast_status hast_fq_create_striped_ex(hast_ctx *const *ctxs, int n_ctx, size_t block_bytes, int n_buffers_per_ctx,
                                      hast_names *const *names_or_null, int device_blocks, hast_fq **out);
int         hast_fq_lanes(const hast_fq *);                      /* contexts the stream's blocks rotate over (1 for hast_fq_create) */
uint64_t    hast_fq_lane_records(const hast_fq *, int lane);     /* records opened so far on that context (striped streams) */
void        hast_fq_destroy(hast_fq *);
size_t      hast_fq_block_bytes(const hast_fq *);
hast_status hast_fq_acquire(hast_fq *, uint8_t **host_buf);
hast_status hast_fq_submit(hast_fq *, size_t n_bytes, int last);
/* Blocks whose bytes are written ON THE DEVICE (e.g. by hast_gz_read_device: a .gz input inflated on the GPU): after
 * hast_fq_acquire (its host buffer stays unused), hast_fq_device_block gives the device address the block's bytes belong at and
 * the stream the writes must be enqueued on; hast_fq_submit_device then frames them where they lie -- no upload.  At most
 * n_buffers - 1 blocks may be in hand (hast_fq_device_block called, not yet submitted) at a time.  A stream takes
 * host blocks or device blocks, not both.  On a striped stream block i's address lies on GPU i % n_ctx and the stream is that
 * GPU's.  hast_fq_block.bytes is NULL for such a block:
 * hast_fq_block_host_bytes (valid between hast_fq_next and hast_fq_commit, for any block) fetches the host copy when the caller
 * needs the text behind bc_pos / bc_len -- a barcode longer than the 15 bytes bc_text holds. */
hast_status hast_fq_device_block(hast_fq *, uint8_t **d_block, hast_stream *fill_stream);
hast_status hast_fq_submit_device(hast_fq *, size_t n_bytes, int last);
hast_status hast_fq_block_host_bytes(hast_fq *, const uint8_t **bytes);
int         hast_fq_poll(hast_fq *);      /* 1: hast_fq_next would not have to wait for the framing of the oldest submitted block */
hast_status hast_fq_next(hast_fq *, hast_fq_block *out);
/* HAST_ERR_INVALID when an id is outside the context's counters: one the caller filled in, or -- on a stream over a device dictionary --
 * when the counters are fewer than hast_fq_block.dict_ids (the dictionary's own ids are not looked at one by one: the bound is checked
 * on the host before anything is queued, so no add outside the counters is ever issued).  Nothing has happened then: the block is
 * still open, its votes are kept; once the counters are large enough (read them, then hast_counts_resize: it zeroes) or the ids are
 * corrected, hast_fq_commit may be called again. */
hast_status hast_fq_commit(hast_fq *);

/* ---- routing: steps 10 and 11 of the wrapper (classify_stlfr_reads.sh:155-190, quartering_fastq.awk:12-61) --------------------
 * After `classify` the wrapper runs a single-threaded awk program over every input once more: each record (four lines) goes to
 * <name>.{nobarcode,paternal,maternal,homozygous}.fastq by the list its barcode is in.  awk splits the header at every '#' or '/'
 * (-F '#|/'): NF > 1 and $2 != "0_0_0" -> $2 is looked up in the paternal, maternal, homozygous list (:22-35; in none: an ERROR
 * line, the record is dropped), otherwise the read has no barcode (:36-39).  A stream put into routing mode frames its blocks as
 * before (plain or striped, host or device blocks), does not classify them, and sorts the records of a block on the GPU into four
 * runs of whole records in input order, which arrive in pinned host memory:
 *     hast_fq_set_route     tables: text record of $2 -> class (1 paternal, 2 maternal, 3 homozygous; hast_names_create +
 *                           hast_names_insert), one per lane of a striped stream.  Between files only.  NULL: classify again.
 *     hast_fq_acquire / _submit / _device_block / _submit_device     as before
 *     hast_fq_next_routed   oldest submitted block: waits for its runs
 *     hast_fq_commit        the caller is through with the runs: the buffer is free again
 * What the device cannot decide stays exact because the caller decides it: a block holding a record whose $2 is longer than the 15
 * bytes a text record holds, or is in no table entry, comes back with host_block != 0 -- the view's bytes and every record's extent
 * and class (0..3; 0xFE: in no list; 0xFF: longer than 15 bytes; 0xFD: not a record of this block) -- and the caller routes that
 * block itself (the ERROR line needs the text); the partial record at the end of a file (fewer than four newlines; awk still
 * prints its lines) is handed over as `tail`. */
typedef struct {
    uint64_t n_records;            /* records in the four runs */
    uint64_t count[4];             /* per class: 0 nobarcode, 1 paternal, 2 maternal, 3 homozygous */
    const uint8_t *run[4];         /* pinned host memory, valid until hast_fq_commit */
    uint64_t run_bytes[4];
    int host_block;                /* != 0: route this block from bytes / rec_* instead (the runs hold the decided records only) */
    const uint8_t *bytes;
    const uint32_t *rec_start, *rec_len;
    const uint8_t *rec_class;
    uint64_t n_slots;
    const uint8_t *tail;           /* the partial record at the end of the file, or NULL */
    uint64_t tail_bytes;
} hast_fq_routed;
hast_status hast_fq_set_route(hast_fq *, hast_names *const *tables, int n_tables);
hast_status hast_fq_next_routed(hast_fq *, hast_fq_routed *out);
/* Routed runs that leave the GPU as gzip members (hast_amd/csrc/dz_core.h, dz_kernels.hip).  on != 0: the four run[c] of
 * hast_fq_next_routed hold one complete gzip member each instead of plain records and run_bytes[c] are the members' sizes; an empty
 * run stays 0 bytes (no member).  count[] and n_records are as before.  Only the compressed bytes are copied to the host: their sizes
 * are known on the device only, so hast_fq_next_routed reads them first and then waits for that one copy.  Blocks that come back
 * with host_block != 0, and the tail, are the caller's and stay plain, as without the switch (such a block is not compressed at all).
 * Memory while the switch is on, per buffer slot of the stream: about two blocks of device memory (the members' buffer and the
 * encoder's workspace) and one block of pinned host memory; on = 0 gives them back.  Only between files, like
 * hast_fq_set_route, and only on a stream that routes.
 * on = 2: the same with BLOCKED gzip (BGZF, hast_dz_compress_blocked_device below): run[c] holds a whole number of BGZF members
 * back to back, one per 49 152 bytes of the run, and no end-of-file block (the caller writes one where its file ends).
 * hast_fq_routed_raw_bytes: the uncompressed bytes of the open block's four runs (what run_bytes[] would have been). */
hast_status hast_fq_set_route_gz(hast_fq *, int on);
hast_status hast_fq_routed_raw_bytes(hast_fq *, uint64_t out[4]);

/* ---- tallies: stage 02's per-barcode read count (assemble_by_supernova.sh, the awk line that writes barcode_freq.txt) -----------
 * Lines are numbered from 1; of every line 4i + 1 (nothing is validated) the header is split at every '#' and '/', and a line with
 * at least one separator counts one for its second field: the bytes between the first separator and the next, or the line's end
 * (possibly empty; any byte but the separators and '\n' belongs to it; hast_amd/csrc/bf_core.h).  A hast_tally is a device dictionary
 * (as hast_names_create_dict makes) of exactly max_texts ids with a 64-bit counter per id.  A stream put into tally mode frames its
 * blocks as before (plain or striped, host or device blocks), classifies nothing -- no k-mer table is needed, read lengths are not
 * looked at -- and counts the keys of a block's header lines on the GPU:
 *     hast_fq_set_tally     one tally per lane of the stream (contexts of one GPU, and several streams, may share one).  Between
 *                           files only.  NULL: classify again.
 *     hast_fq_acquire / _submit / _device_block / _submit_device     as before
 *     hast_fq_next_tallied  oldest submitted block: returns once its keys are counted
 *     hast_fq_commit        the caller is through with the block: the buffer is free again
 * hast_fq_next and hast_fq_next_routed fail with HAST_ERR_INVALID on such a stream, hast_fq_next_tallied on any other; nothing
 * happens then.  Left to the caller, exactly: keys longer than 15 bytes, keys that arrive once the tally has handed out its last id
 * (one answer per text, as for hast_names_create_dict: a key is counted on the device in every block or left in every block, per
 * tally), and the partial record at the end of a file (`tail`: it starts at a record boundary).  For every block
 * n_counted + n_left + n_nofield == n_records.
 * hast_tally_size: ids handed out; hast_tally_read: text records (16 bytes: length byte + text) and counts of ids [first, first + n). */
typedef struct hast_tally hast_tally;
typedef struct {
    uint64_t n_records;            /* header lines this block owns */
    uint64_t n_counted;            /* ... counted on the device */
    uint64_t n_nofield;            /* ... without a separator: counted by nobody */
    uint64_t n_left;               /* ... left to the caller */
    const uint32_t *left_pos;      /* [n_left] where their keys start in the block's view */
    const uint32_t *left_len;      /* [n_left] and how long they are */
    const uint8_t *bytes;          /* the view; NULL for a block submitted with hast_fq_submit_device: hast_fq_block_host_bytes
                                      fetches it (needed only when n_left > 0) */
    const uint8_t *tail;           /* the partial record at the end of the file, or NULL */
    uint64_t tail_bytes;
} hast_fq_tallied;
hast_status hast_tally_create(hast_ctx *, size_t max_texts, hast_tally **out);
size_t      hast_tally_limit(const hast_tally *);
hast_status hast_tally_size(hast_tally *, size_t *n_ids);
hast_status hast_tally_read(hast_tally *, size_t first, size_t n, uint8_t *text16, uint64_t *counts);
void        hast_tally_destroy(hast_tally *);
hast_status hast_fq_set_tally(hast_fq *, hast_tally *const *tallies, int n_tallies);
hast_status hast_fq_next_tallied(hast_fq *, hast_fq_tallied *out);

/* ---- deflate on the GPU: device memory -> one gzip member -----------------------------------------------------------------
 * hast_dz_compress_device writes ONE complete gzip member (RFC 1952: what gzip -dc, zlib and hast_gz read) for the n_bytes at
 * d_src, n_bytes == 0 included (an empty member), to d_dst, and waits for it; *n_out = its size.  The input is cut into pieces of
 * 16 KB that a wave each compresses on its own (hashed match search verified byte by byte, greedy parse, dynamic Huffman codes
 * limited to 15 bits; a piece that would not get smaller is a stored block), every piece ends on a byte boundary with an empty
 * stored block, CRC-32 is computed on the device.  The bytes written are a function of the input bytes alone.
 * hast_dz_bound(n): the most bytes a call can write for n bytes of input (host arithmetic).  cap < hast_dz_bound(n_bytes) is
 * HAST_ERR_INVALID; nothing is ever written at or behind d_dst + cap.
 * hast_dz_compress_device_ex / HAST_DZ_LITERALS_ONLY are a TEST HOOK, not part of the interface a caller should build on and not
 * promised to stay: flags = HAST_DZ_LITERALS_ONLY switches the match search off (Huffman coding of the bytes alone), which is how
 * tests/test_dz_gpu.py gets a block whose symbol histogram is the input's byte histogram (code lengths that have to be limited to
 * 15 bits); no program of this tree passes it.
 * BLOCKED gzip (BGZF: what bgzip / htslib write and seek in, what hast_gz_open_blocked inflates a wave per member):
 * hast_dz_compress_blocked_device writes the same pieces, three to a member: 18 bytes of header with the BC subfield, at most
 * 49 152 bytes of input, CRC-32 and ISIZE of that member alone; ceil(n_bytes / 49 152) members back to back, each at most 64 KB.
 * n_bytes == 0 writes the 28 bytes of BGZF's end-of-file block.  hast_dz_bound_blocked(n) is its bound; cap below it is
 * HAST_ERR_INVALID.  gzip -dc and zlib read the result as they read any series of members. */
#define HAST_DZ_LITERALS_ONLY 1u
size_t      hast_dz_bound(size_t n_bytes);
hast_status hast_dz_compress_device(hast_ctx *, const uint8_t *d_src, size_t n_bytes, uint8_t *d_dst, size_t cap, size_t *n_out, hast_stream);
hast_status hast_dz_compress_device_ex(hast_ctx *, const uint8_t *d_src, size_t n_bytes, uint8_t *d_dst, size_t cap, size_t *n_out, unsigned flags,
                                       hast_stream);
size_t      hast_dz_bound_blocked(size_t n_bytes);
hast_status hast_dz_compress_blocked_device(hast_ctx *, const uint8_t *d_src, size_t n_bytes, uint8_t *d_dst, size_t cap, size_t *n_out, hast_stream);

/* ---- the output table on the GPU: printBarcodeInfos (classify.cpp:93-102) and the wrapper's three barcode lists ----------------
 * From the text records of n barcodes (16 bytes each: length byte + up to 15 bytes of text, as a device dictionary keeps them by id)
 * and their counters ([n][4] 64-bit words, {c0, c1, ..}), both in device memory: the table `text \t hap \t c0 \t c1 \n`, one row per
 * id, sorted byte-wise by text (a prefix in front of what it is a prefix of), the call by hast_get_hap's rule (n0, n1: the set
 * sizes, w0, w1: the weights); with_lists != 0 also the three lists `text \n` of the barcodes called 0 (list 1, paternal), 1 (list
 * 2, maternal) and -1 (list 3, homozygous), each in row order.  Keyed, sorted, sized and formatted on the device; only the finished
 * text is read back.  The bytes are those `classify` writes on the host (hast_amd/csrc/rows_core.h has the rules).
 * hast_rows_build_device takes raw device pointers (d_text16 16-byte aligned, d_counts 32-byte aligned; n < 2^32; n == 0 is valid
 * and gives empty texts); hast_rows_build takes the texts of ids [0, n) of a device dictionary (hast_names_create_dict) and the
 * counters bound to the context, which must be on the dictionary's GPU and hold at least n barcodes.  Both wait for the work.
 * HAST_ERR_OOM when the device has no room (what closed streams have parked is freed first): the caller makes the table on the host.
 * hast_rows_get_info: the sizes; any_sep: a barcode holds '#' or '/'; past_int: a count is above INT_MAX; the seconds of the three
 * steps.  hast_rows_read: n bytes from `offset` of the table (which = 0) or of list 1..3, through pinned staging of the handle's
 * own (one call at a time per handle); beyond the text's end: HAST_ERR_INVALID.  hast_rows_order: the n ids in row order.
 * hast_rows_classes: the list (1..3) of every id. */
typedef struct hast_rows hast_rows;
typedef struct {
    uint64_t n_rows, table_bytes, list_bytes[3];
    int      any_sep, past_int;
    double   keys_s, sort_s, format_s;
} hast_rows_info;
hast_status hast_rows_build_device(hast_ctx *, const uint8_t *d_text16, const uint64_t *d_counts, size_t n, uint64_t n0, uint64_t n1, double w0, double w1,
                                   int with_lists, hast_rows **out);
hast_status hast_rows_build(hast_ctx *, hast_names *dict, size_t n, uint64_t n0, uint64_t n1, double w0, double w1, int with_lists, hast_rows **out);
hast_status hast_rows_get_info(hast_rows *, hast_rows_info *);
hast_status hast_rows_read(hast_rows *, int which, uint64_t offset, size_t n, void *host);
hast_status hast_rows_order(hast_rows *, uint32_t *ids_in_row_order);
hast_status hast_rows_classes(hast_rows *, uint8_t *cls_by_id);
void        hast_rows_destroy(hast_rows *);

/* ---- gzip input decoded on the device (gzstream.h:47, classify.cpp:245-254: one zlib stream per .gz file) -----------------
 * HAST's real inputs are ordinary .fq.gz files: ONE deflate stream per file, which the reference inflates on the thread that
 * also frames the records.  hast_gz inflates such a file on the GPU: the COMPRESSED bytes cross PCIe (5-6 x fewer than the
 * FASTQ text) and the inflated bytes are written where the caller wants them in HBM -- e.g. straight into a block of the FASTQ
 * framer (hast_fq_submit_device), which reads them where they lie.  Method (hast_amd/csrc/gz_core.h, gz_chain.h, gz_kernels.hip):
 * every 16-KB chunk of the compressed bytes (round 6; 32 KB until then) searches its first dynamic-block header and is decoded by ONE WAVE into 16-bit
 * symbols with the 32 KB in front of it unknown ("marker" symbols); a chunk counts iff the chunk in front of it ended exactly
 * at its start (holes are decoded by follow-up jobs); windows are resolved in stream order, markers translated, and every
 * member's CRC-32 and ISIZE are checked (CRC by slices on the device, combined with GF(2) operators), so a decoding bug or a
 * damaged file cannot pass as data.  Any gzip file is taken: all block types, several members, header fields, trailing garbage
 * (ignored, as gzread does).
 * hast_gz_open: HAST_ERR_UNSUPPORTED when the path is not a regular file, does not start with a gzip member (zlib passes such a
 * file through as it is) or the device has no room -- the caller then inflates on the host; HAST_ERR_IO when it cannot be read.
 * hast_gz_read_device: the next up to `cap` bytes of the inflated stream, written to d_dst by a kernel on `stream` (NULL: the
 * context's); *n_out < cap at the end of the stream (0 = nothing left) -- or when damage follows what was delivered: a damaged or
 * truncated file is HAST_ERR_IO only AFTER what could be decoded in front of the damage has been handed over, as gzread does, i.e.
 * with the call behind a short one.  A caller must therefore read on until a call returns 0 bytes (or an error) before it takes the
 * stream for complete.  Blocks until the bytes it returns are decoded.  HAST_GZ_CHUNK_BYTES / HAST_GZ_PASS_CHUNKS in the environment
 * set the geometry of hast_gz_open (tests: many passes over a small file).
 * A file of more than 2 GB is not kept whole on the device: its compressed bytes go round a ring there (hast_gz_stats.ring_bytes).
 * One reader per object; several of them -- one per input file -- run side by side. */
typedef struct hast_gz hast_gz;
typedef struct {
    uint64_t compressed_bytes, out_bytes;
    uint64_t chunks, accepted, followup_jobs, followup_rounds, followup_accepted, members;
    double decode_s;           /* search + decode passes (host wall time of the producer thread) */
    double windows_crc_s;      /* windows + CRC passes */
    double wait_upload_s;      /* the producer waited for compressed bytes to reach the device */
    double wait_consumer_s;    /* ... for the reader to be through with a symbol arena */
    double wait_decode_s;      /* the reader waited for decoded bytes */
    double open_s;             /* hast_gz_open itself: device buffers (the first symbol arena), streams, threads */
    uint64_t ring_bytes;       /* 0: the whole compressed file lies on the device; else the size of the ring it goes round in
                                * (files beyond 2 GB; HAST_GZ_RING_BYTES / HAST_GZ_PIECE_BYTES set the geometry in tests) */
    uint64_t upload_waited_for_ring;   /* pieces whose upload had to wait for the chain to move on */
    double chain_walk_s;       /* host time between the kernels: accepting chunks, planning follow-up jobs, combining CRC-32s -- the part
                                * of ONE deflate stream that stays serial however many GPUs decode its passes */
    uint64_t ring_laps;        /* times the upload position wrapped round the ring */
} hast_gz_stats;
hast_status hast_gz_open(hast_ctx *, const char *path, hast_gz **out);
/* test / tuning entry: compressed bytes per chunk (0 = 16384), chunks per pass (0 = 6144; 4096 with a chunk size given), symbols of room per
 * compressed byte (0 = 20 with the default geometry, else 12).  A pass's arena holds symbol slots for 70 % of its chunks (those WITH a block
 * start take one on the device; HAST_GZ_SLOT_FRACTION fixes the share, by default it follows what the passes find).  Two passes of a
 * stream are on the GPU at a time, on two streams, with three arenas to take turns (HAST_GZ_AHEAD=0: one pass, two arenas). */
hast_status hast_gz_open_ex(hast_ctx *, const char *path, size_t chunk_bytes, size_t chunks_per_pass, double room, hast_gz **out);
/* ONE .gz file inflated by several GPUs (the reference deals the reads of one file to all its workers whatever the file's encoding,
 * classify.cpp:211-219,245-254; HAST's inputs are two .fq.gz files, HAST.sh:162-166): the passes of the one deflate stream (4096
 * chunks each) go to the GPUs of ctxs[] in turn -- a chunk's decode into marker symbols needs nothing from its neighbours -- one
 * "unit" per distinct device (contexts that share a GPU share it), each with the whole compressed file, its own symbol arenas and
 * streams; the chain of accepted chunks is one, the 32-KB window a pass leaves travels to the next pass's GPU through pinned host
 * memory, CRC-32 / ISIZE are checked as for one GPU.  hast_gz_read_device then takes a destination on ANY of those GPUs (it asks
 * the runtime where the pointer lives): the bytes are translated on the unit that decoded them and, when that is another GPU,
 * copied over peer to peer -- e.g. into the device-side blocks of a striped FASTQ stream (hast_fq_create_striped).
 * HAST_GZ_SPLIT=contexts in the environment: one unit per CONTEXT even where contexts share a GPU, and every read through the
 * hand-over buffer + peer copy (the several-GPU paths on one GPU, for tests).  hast_gz_units: how many units the stream has. */
hast_status hast_gz_open_multi(hast_ctx *const *ctxs, int n_ctx, const char *path, hast_gz **out);
hast_status hast_gz_open_multi_ex(hast_ctx *const *ctxs, int n_ctx, const char *path, size_t chunk_bytes, size_t chunks_per_pass, double room, hast_gz **out);
int         hast_gz_units(const hast_gz *);
hast_status hast_gz_read_device(hast_gz *, uint8_t *d_dst, size_t cap, size_t *n_out, hast_stream);
hast_status hast_gz_get_stats(hast_gz *, hast_gz_stats *out);
void        hast_gz_close(hast_gz *);
/* BLOCKED gzip (BGZF: bgzip, htslib, many sequencer pipelines) inflated on the device PER MEMBER.  Every member's header says how
 * long the member is (the `BC` extra subfield), its trailer what it inflates to, and no match reaches in front of its member: the
 * members of a piece of the file are found without inflating anything (hast_amd/csrc/bz_core.h), their places in the output are one
 * prefix sum, and each is decoded by ONE WAVE from a known start straight to bytes (bz_kernels.hip k_bz_inflate) -- none of the
 * search, chain, marker symbols, windows and translate that hast_gz_open needs for "any gzip".  CRC-32 and ISIZE of every member are
 * checked on the device (k_bz_crc); the host reads 8 bytes per batch.  Batches of whole members (batch_in_bytes of compressed input,
 * batch_out_bytes of output; 0 = 32 MB / 192 MB; both at least one member) go through three sets of buffers: one is read and uploaded
 * while one is decoded and the reader copies out of the third.
 * The handle is a hast_gz: hast_gz_read_device (same contract: filled to cap except at the end, damage reported by the call BEHIND
 * the one that delivered the bytes of all members in front of the first bad one), hast_gz_get_stats (compressed_bytes, out_bytes,
 * members, open_s; the rest 0), hast_gz_units (1) and hast_gz_close work on it.
 * hast_gz_open_blocked: HAST_ERR_UNSUPPORTED when the path is not a regular file, is empty, does not start with a BGZF member or
 * the device has no room -- the caller then uses hast_gz_open or the host; HAST_ERR_IO when it cannot be read.  A gzip member that
 * is not BGZF met in mid-file: the bytes in front of it are delivered, the next call returns HAST_ERR_UNSUPPORTED with the file
 * offset in hast_last_error() (and in hast_gz_blocked_stats.unsupported_offset).  Bytes that do not start a gzip member end the
 * stream, as for gzread.
 * ONE caller stream per handle: every hast_gz_read_device call on a blocked handle must name the same stream (or NULL every time).  A
 * batch's buffer goes back to the producer behind an event recorded on the stream of the call that finished the batch; copies that
 * earlier calls put on another stream would not be waited for. */
typedef struct {
    uint64_t members, batches;
    uint64_t carried;              /* members cut by the end of a piece of the file and carried to the front of the next one */
    double read_s;                 /* pread into pinned memory + the walk over the members (producer thread, wall time) */
    double upload_s, kernels_s;    /* event pairs on the stream's own HIP stream, over the batches the reader has taken */
    double wait_reader_s;          /* the producer waited for the reader to be through with a set of buffers */
    uint64_t unsupported_offset;   /* file offset of a gzip member that is not BGZF, or 0 */
} hast_gz_blocked_stats;
hast_status hast_gz_open_blocked(hast_ctx *, const char *path, hast_gz **out);
hast_status hast_gz_open_blocked_ex(hast_ctx *, const char *path, size_t batch_in_bytes, size_t batch_out_bytes, hast_gz **out);
/* HAST_ERR_INVALID on a handle of hast_gz_open */
hast_status hast_gz_get_blocked_stats(hast_gz *, hast_gz_blocked_stats *out);

/* ---- host-side pieces of the path (no device work) ---------------------------------------- */
/* parseName (classify.cpp:112-119): barcode = head[last '#' + 1 .. last '/'). */
void     hast_parse_barcode(const char *head, size_t len, size_t *start, size_t *n);
/* getHap (classify.cpp:66-86). */
int      hast_get_hap(const char *barcode, size_t blen, uint64_t c0, uint64_t c1,
                      uint64_t n_hap0, uint64_t n_hap1, double w0, double w1);
/* Kmer::str2Kmer (kmer.h:153-166) / chopRead2Kmer (kmer.h:169-194) on the host, used for the
 * <=2x(45-K+1) adaptor keys of InitAdaptor. */
uint64_t hast_canon_kmer(const char *s, int k);
size_t   hast_chop_read(const char *seq, size_t len, int k, uint64_t *out);
void     hast_kmer_to_str(uint64_t kmer, int k, char *out /* k+1 */);

/* ---- synthetic workload; identical generator on host and device -------------- */
typedef struct {
    uint64_t seed_k, seed_r, seed_b; /* 0 => defaults 0x4841535401/02/03 */
    uint64_t n_keys_per_hap;
    uint32_t n_barcodes;
    uint32_t read_len;
    uint32_t k;
    uint32_t reserved;               /* 0 = independent random keys; 1 = clustered keys: runs of K
                                        overlapping windows around variant sites, like real parent-specific k-mers */
} hast_synth_params;

hast_status hast_synth_keys_host(const hast_synth_params *, int hap, uint64_t first, size_t n, uint64_t *out);
hast_status hast_synth_reads_host(const hast_synth_params *, uint64_t first_read, size_t n_reads,
                                  uint8_t *bases /* n*read_len */, uint32_t *barcode_ids);
hast_status hast_synth_keys_device(hast_ctx *, const hast_synth_params *, int hap, uint64_t first, size_t n,
                                   uint64_t *d_out, hast_stream);
hast_status hast_synth_reads_device(hast_ctx *, const hast_synth_params *, uint64_t first_read, size_t n_reads,
                                    uint8_t *d_bases, uint32_t *d_barcode_ids, hast_stream);
/* generate + insert both haplotypes' keys on the device (no host copy of the keys) */
hast_status hast_synth_table_build(hast_ctx *, const hast_synth_params *);

/* ==== stage 00: parent-unique k-mer sets ======================================
 * Replaces the compute of 00.build_unshare_kmers_by_jellyfish/build_unshared_kmers.sh:165-291, which drives a
 * third-party CPU hash counter (jellyfish 2.3.0, vendored there as a binary) through seven count/dump passes over text
 * files.  Here ONE table in HBM holds, for every canonical k-mer of either parent, its paternal and its maternal count;
 * the histograms (analysis_kmercount.sh:7-9), and the two final sets (script lines 246-291)
 *     paternal.unique.filter = { x : p_lower <= count_pat(x) <= p_upper and count_mat(x) == 0 }   (and vice versa)
 * are read out of it directly.  Counting rules = `jellyfish count -m K -C`: every window of K consecutive bases,
 * both cases of ACGT are bases, any other byte ends the run; a k-mer and its reverse complement are one key.
 * parent: 0 = paternal, 1 = maternal.
 *
 * Key space slices: when the table cannot hold every distinct k-mer, hast_kc_sync reports HAST_ERR_TABLE_FULL;
 * the caller then processes the key space in n_slices passes over the input (hast_kc_set_slice), each pass
 * counting only the k-mers of its slice; histograms add up and selections concatenate over the slices.  The
 * same call shards the key space over several GPUs (one context per GPU, disjoint slices, no collective). */
typedef struct hast_kc hast_kc;
#define HAST_KC_HISTO_HIGH 10000u          /* counts above are lumped into bin HIGH+1 (jellyfish histo default) */

/* table_bytes == 0 (or more than that): 85 % of the free device memory.  k in [1,32]. */
hast_status hast_kc_create(int device_ordinal, int k, size_t table_bytes, hast_kc **out);
/* expected_windows: an upper bound on the k-mer occurrences the caller is going to count into this table (0 = unknown), e.g. from
 * the input files' sizes: the record buffers of the partitioned path then take room for that many windows' records instead of what
 * happens to be free on the device (tens of GB that a 20-Mbp job never fills, and that are slow to get right after another process
 * gave them back). */
hast_status hast_kc_create_ex(int device_ordinal, int k, size_t table_bytes, uint64_t expected_windows, hast_kc **out);
void        hast_kc_destroy(hast_kc *);
hast_stream hast_kc_stream(hast_kc *);
/* empties the table and restricts counting to slice `slice` of `n_slices` (1 slice = everything) */
hast_status hast_kc_set_slice(hast_kc *, uint32_t slice, uint32_t n_slices);
/* Count the k-mers of a byte stream for one parent.  The stream is a sequence of records' bases with at least one
 * non-base byte (e.g. '\n') between records; windows start at [0, n_bytes).  _device: bytes already in HBM,
 * asynchronous on the context's stream.  Host variant: copies through pinned staging, double-buffered; it may
 * return HAST_ERR_TABLE_FULL early (the device's word is polled without waiting), hast_kc_sync reports it for sure. */
hast_status hast_kc_count_device(hast_kc *, int parent, const uint8_t *d_bytes, size_t n_bytes);
hast_status hast_kc_count(hast_kc *, int parent, const uint8_t *bytes, size_t n_bytes);
/* wait for all counting submitted so far; HAST_ERR_TABLE_FULL when some k-mer found no slot */
hast_status hast_kc_sync(hast_kc *);
/* How the windows reach the table.  Tables of >= 2^20 buckets (128 MB) with a K a record has room for (K <= 27 at the default
 * minimizer length) count by PARTITIONING (hast_amd/csrc/kc_kernels.hip; kc_common.h "records", "PLACEMENT"): the windows are written
 * out as 8-byte records of a minimizer run each, the records are partitioned by bucket range in two levels down to slices of 512 or
 * 1024 buckets, and one workgroup per slice counts its records in LDS -- the table is read and written once per flush, sequentially,
 * instead of one memory-side atomic per minimizer run (k_kc_count, the DIRECT path of smaller tables and larger K, which stands at
 * the rate at which this part executes atomics).  Same counts, histograms and selections (tests); the two paths file a key in
 * different buckets, so a table is filled by one of them only.  HAST_KC_COUNT=atomic|partition in the environment at hast_kc_create
 * forces either.  Flushes happen at hast_kc_sync, before the table is read, and when the record buffer is nearly full (it takes what
 * is left of the device memory next to the table, at most one record per slot of the table; HAST_KC_RECORD_MB caps it); a flush of
 * few records for the table's size goes through the direct path where the records lie (HAST_KC_FLUSH=sweep|atomic pins that).
 * out[0] = 1: partitioned; out[1] flushes; out[2] records applied; out[3] windows that took the direct path after all (their four
 * buckets in the slice full); out[4] record capacity. */
hast_status hast_kc_partition_info(hast_kc *, uint64_t out[5]);
/* out[0..1] distinct k-mers per parent, out[2] keys in the table, out[3] table capacity (slots),
 * out[4..5] k-mer occurrences counted per parent */
hast_status hast_kc_stats(hast_kc *, uint64_t out[6]);
/* ADDS the count histogram of one parent to histo[0 .. HAST_KC_HISTO_HIGH+1] (`jellyfish histo`) */
hast_status hast_kc_histo(hast_kc *, int parent, uint64_t *histo);
/* find_bounds.awk:1-33 over the non-empty rows of a histogram: out = MIN_INDEX, MAX_INDEX, LOWER_INDEX, UPPER_INDEX.
 * Host-only arithmetic (no GPU needed). */
void        hast_kc_find_bounds(const uint64_t *histo, long out[4]);
/* Append to the context's selection of `parent` the keys of the current table with lower <= count <= upper that the
 * other parent does not have.  n_added may be NULL. */
hast_status hast_kc_select(hast_kc *, int parent, uint32_t lower, uint32_t upper, size_t *n_added);
/* forget what has been selected so far (e.g. before starting over with more slices) */
hast_status hast_kc_selection_clear(hast_kc *);
/* move what `src` has selected so far to the end of `dst`'s selections (key space split over several contexts) */
hast_status hast_kc_selection_adopt(hast_kc *dst, hast_kc *src);
/* free the table (the selections stay) */
hast_status hast_kc_release_table(hast_kc *);
/* sort the selection of `parent` (ascending = lexicographic order of the printed k-mers) and keep it on the device */
hast_status hast_kc_selection_sort(hast_kc *, int parent, size_t *n);
/* rows [first, first+count) of the sorted selection as text: count lines of K upper-case letters + '\n', the member of
 * {k-mer, reverse complement} that comes first in the order A<C<G<T (what the reference's .mer files hold) */
hast_status hast_kc_selection_text(hast_kc *, int parent, size_t first, size_t count, char *out);
/* the same rows as stage-01 table keys (hast_table_insert_keys), no text round trip */
hast_status hast_kc_selection_keys(hast_kc *, int parent, size_t first, size_t count, uint64_t *out);

/* synthetic trio for benches and tests: two parental genomes = one random genome + parent-specific SNPs; reads are
 * sampled with substitution errors on a random strand; the stream is read_len bases + '\n' per read */
typedef struct hast_kc_synth {
    uint64_t seed;            /* 0 => default */
    uint64_t genome_len;
    uint32_t read_len;
    uint32_t snp_per_1024;    /* parent-specific SNPs per 1024 bases */
    uint32_t err_per_4096;    /* substitution errors per 4096 bases */
    uint32_t n_per_4096;      /* reads with one 'N' per 4096 reads */
} hast_kc_synth;
hast_status hast_kc_synth_host(const hast_kc_synth *, int parent, uint64_t first_read, size_t n_reads, uint8_t *out);
hast_status hast_kc_synth_device(hast_kc *, const hast_kc_synth *, int parent, uint64_t first_read, size_t n_reads, uint8_t *d_out);

/* ---- stage 00 ingest on the device: raw four-line FASTQ in HBM -> the base stream hast_kc_count_device takes --------------------
 * The stream is what the host parser (hast_amd/csrc/seqstream.h) hands the counter: per record the bytes of the sequence line, the
 * '\r's of the line break stripped, then one '\n'.  A block is taken only when "a record is four lines" and that parser agree on it
 * (hast_amd/csrc/sq_core.h: header starts with '@'; a non-empty sequence does not start with '+'; the third line starts with '+';
 * quality as long as the sequence) and is refused as a whole otherwise: HAST_SQ_NOT_FOUR_LINE, first_bad = index of the first record
 * that breaks a rule, nothing written, every count 0.  consumed = the byte behind the last 4n-th newline: the caller puts
 * [consumed, n_in) in front of the next bytes.  A block with fewer than four newlines frames nothing (HAST_SQ_NO_RECORD, consumed 0).
 * first_bad is 0xFFFFFFFF when no record breaks a rule.
 * hast_sq_create: on the device and the stream of the count table (hast_kc_stream); scratch for the worst block of max_in_bytes
 * (< 4 GB; all newlines: ~6 bytes per byte of input).  Destroy it before the table.
 * hast_sq_frame_device: asynchronous on that stream up to the copy of *res, returns when *res is valid; d_in and d_out at any
 * alignment; cap_out >= n_in; nothing is written at or behind d_out + out_bytes, nothing read outside [d_in, d_in + n_in). */
typedef struct hast_sq hast_sq;
typedef struct { uint64_t consumed, out_bytes, records, bases; uint32_t flags, first_bad; } hast_sq_result;
#define HAST_SQ_NOT_FOUR_LINE 1u   /* a record breaks a rule: nothing written */
#define HAST_SQ_NO_RECORD     2u   /* fewer than four newlines in the input */
hast_status hast_sq_create(hast_kc *, size_t max_in_bytes, hast_sq **out);
hast_status hast_sq_frame_device(hast_sq *, const uint8_t *d_in, size_t n_in, uint8_t *d_out, size_t cap_out, hast_sq_result *res);
void        hast_sq_destroy(hast_sq *);
/* FASTA, by the same framer: the stream that parser hands the counter in FASTA mode (hast_amd/csrc/sq_core.h, namespace sqfa).  A view
 * is [bytes carried from the view before | new bytes]; its lines are the newline-terminated ones and, with HAST_SQ_FA_LAST, the bytes
 * behind the last newline.  An empty line (its trailing '\r's stripped) gives nothing; a '>' line counts one record and gives one '\n'
 * if a record is open -- a header came earlier in this input: HAST_SQ_FA_OPEN says "in an earlier view"; every other line gives its
 * bytes as they lie.  With HAST_SQ_FA_LAST one closing '\n' follows if a record is open.  consumed = the byte behind the last newline,
 * or n_in with HAST_SQ_FA_LAST; bases = the bytes written that are no separators; flags 0, first_bad 0xFFFFFFFF: FASTA has no format
 * error behind its first byte.  n_in == 0 is valid.  cap_out >= n_in + 1; alignment, reads and writes as hast_sq_frame_device.  The
 * scratch (~8 bytes per byte of max_in_bytes) is allocated by the first call. */
#define HAST_SQ_FA_OPEN 1u
#define HAST_SQ_FA_LAST 2u
hast_status hast_sq_frame_fasta_device(hast_sq *, const uint8_t *d_in, size_t n_in, uint8_t *d_out, size_t cap_out, unsigned in_flags, hast_sq_result *res);

/* The feed of one input stream of `unshared_kmers --ingest device`: two input and two output buffers on the device and two pinned
 * staging blocks, so that the upload of block n+1 (a stream of the feed's own) overlaps the framing and counting of block n.
 *   hast_sq_feed_host_block    pinned memory for the next up to block_bytes raw bytes (waits until it is free), uploaded by _submit
 *   hast_sq_feed_device_block  where the caller's kernels on hast_kc_stream write them instead (hast_gz_read_device), block_bytes of room
 *   hast_sq_feed_submit        n_bytes > 0 of the block just handed out are valid; at most two blocks are submitted and not yet taken by _next
 *   hast_sq_feed_next          frames the bytes carried from the block before + the oldest submitted block, counts the stream for
 *                              `parent` (hast_kc_count_device) and carries [consumed, n) to the front of the next block.  *res as
 *                              hast_sq_frame_device; nothing is counted when res->flags has HAST_SQ_NOT_FOUR_LINE or
 *                              HAST_SQ_TAIL_TOO_LONG (more than block_bytes would have to be carried: a full buffer without a record).
 *                              Calls into the count table: the caller serialises it with the table's other users.
 *   hast_sq_feed_take_tail     the carried bytes (fewer than four newlines) to dst (block_bytes of room) at the end of an input; the
 *                              feed then starts the next input with nothing carried. */
typedef struct hast_sq_feed hast_sq_feed;
#define HAST_SQ_TAIL_TOO_LONG 4u
hast_status hast_sq_feed_create(hast_kc *, size_t block_bytes, hast_sq_feed **out);
hast_status hast_sq_feed_host_block(hast_sq_feed *, uint8_t **h_buf);
hast_status hast_sq_feed_device_block(hast_sq_feed *, uint8_t **d_buf);
hast_status hast_sq_feed_submit(hast_sq_feed *, size_t n_bytes);
hast_status hast_sq_feed_next(hast_sq_feed *, int parent, hast_sq_result *res);
hast_status hast_sq_feed_take_tail(hast_sq_feed *, uint8_t *dst, size_t *n_bytes);
void        hast_sq_feed_destroy(hast_sq_feed *);
/* FASTA through the feed:
 *   hast_sq_feed_set_formats   HAST_SQ_TAKE_FASTQ (the default), or HAST_SQ_TAKE_FASTQ | HAST_SQ_TAKE_FASTA; only while nothing is
 *                              submitted and nothing is carried.  With FASTA taken, the first byte of an input's first view decides as
 *                              it does for the host parser: '>' makes the input FASTA until its end, anything else goes the FASTQ way.
 *   hast_sq_feed_format        of the current input: 0 undecided, 1 FASTQ, 2 FASTA
 *   hast_sq_feed_next          on a FASTA input: frames the view with the feed's own open state and counts its stream with the last
 *                              min(K - 1, stream so far) bytes emitted for this input in front, so that the windows across a view
 *                              boundary are counted exactly once; records of any length pass, only a LINE longer than block_bytes
 *                              is HAST_SQ_TAIL_TOO_LONG.
 *   hast_sq_feed_finish        ends a FASTA input: frames what is carried as the last view (possibly no byte), counts it, and starts
 *                              the next input undecided.  HAST_ERR_INVALID on a FASTQ or undecided input (hast_sq_feed_take_tail). */
#define HAST_SQ_TAKE_FASTQ 1u
#define HAST_SQ_TAKE_FASTA 2u
hast_status hast_sq_feed_set_formats(hast_sq_feed *, unsigned mask);
int         hast_sq_feed_format(hast_sq_feed *);
hast_status hast_sq_feed_finish(hast_sq_feed *, int parent, hast_sq_result *res);

/* ---- stage 03 ingest on the device: raw FASTA / four-line FASTQ in HBM -> per-read votes (`classify_read --ingest device`) ------
 * The "read stream" feed frames the reads of the per-read classifier on the GPU and classifies them where they lie
 * (hast_classify_perread's semantics: per-window validity, reads of any length).  The rules are the reference reader's
 * (03.mkoutput_by_fabulous2.0/src_main/classify.cpp:248-302; hast_amd/csrc/rs_core.h restates them, rs_host.h is the model):
 *   FASTQ  record i = lines 4i .. 4i+3; name = the header line minus its first byte; sequence = line 4i+1 as it lies; a non-empty
 *          header that starts with '>' is the format error; what a file's end leaves (fewer than four newlines) is the caller's
 *          (hast_rs_take_tail).
 *   FASTA  only newline-terminated lines count; empty lines are skipped; '>' starts a record, a line that starts with '@' or '+' is
 *          the format error, any other line is appended to the open record (to none before the file's first header); the reads are
 *          compacted into one base buffer on the device, because a k-mer straddles the line breaks.
 * One feed per context: two view buffers on the device, two pinned staging blocks, pinned result buffers; the upload of block n+1
 * (a stream of the feed's own) overlaps the framing and classification of block n (the context's stream).
 *   hast_rs_create        block_bytes from 64 to 2^30; device scratch for the worst view of 2 x block_bytes (all newlines, FASTA
 *                         records of two bytes: about 30 bytes per byte of a view), so no input has "too many records".
 *   hast_rs_host_block    pinned memory for the next up to block_bytes raw bytes (waits until it is free), uploaded by _submit
 *   hast_rs_device_block  where the caller's kernels write them instead, on the stream *fill (the context's; hast_gz_read_device)
 *   hast_rs_submit        n_bytes of the block just handed out are valid; last != 0: the file ends with them (n_bytes may then be
 *                         0).  At most two blocks are submitted and not yet taken by _next.
 *   hast_rs_next          frames [what the block before left | the oldest submitted block], classifies the complete records and
 *                         carries [consumed, n) to the front of the next block.  Returns when *out is valid: votes[2 r], votes[2 r + 1]
 *                         = the hits of read r against haplotype 0 / 1, names[name_off[r] .. name_off[r + 1]) its name; the pointers
 *                         are the feed's pinned buffers, valid until the next hast_rs_next.  flags != 0: nothing was classified and
 *                         the file is given up (records = 0) -- HAST_RS_FORMAT_ERROR as above, HAST_RS_RECORD_TOO_LONG when more
 *                         than block_bytes would have to be carried.  The file's other blocks, up to its `last` one, come back with
 *                         the same flags, unframed: a caller that stops reading submits an empty `last` block and takes it.
 *                         After a `last` block the next one starts a new file.
 *   hast_rs_take_tail     FASTQ, after the `last` block: the bytes behind the last complete record to dst (block_bytes of room).
 * The read bins (`classify_read --bin-reads`; rules: hast_amd/csrc/rb_core.h, model: rb_host.h): every record of a view, as its bytes
 * lie in the input (FASTQ: its four lines; FASTA: from its header line to the next header line, blank lines and '\r' included; the last
 * record of a file ends behind the last newline), goes to the run of its class -- 0 haplotype0, 1 haplotype1, 2 ambiguous, by the rule
 * of the rows: d = votes / total, neither above 0: ambiguous, else d1 > d0: haplotype1, else haplotype0.  A run is the records of one
 * class back to back in input order.  Bytes of no record (junk before a file's first header, an unterminated last FASTA line) go
 * nowhere; a FASTQ file's tail is the caller's, as before.
 *   hast_rs_set_bins      mode 0 off, 1 plain, 2 every run deflated on the GPU into one gzip member; total0 / total1: the two set
 *                         sizes.  Only while no submitted block waits for _next (HAST_ERR_INVALID otherwise).  The buffers of the bins
 *                         are allocated at the first switch-on and go with hast_rs_destroy: a feed that never asks has none.
 *   hast_rs_next_binned   hast_rs_next plus the bins of the same view; returns when the runs lie in pinned memory.  With flags != 0,
 *                         or with the bins switched off, *bins is all zero.
 * The rows (`classify_read --rows device`; rules: hast_amd/csrc/rr_core.h, model: rr_host.h): the text the program prints per read,
 * "name \t haplotype0|haplotype1 \t D \n" or "name \t ambiguous \t 0.0 \n", made on the GPU from the names and votes where the framer
 * and the classifier leave them, in read order.  The class is the bins' (rb_core.h); D is what printf("%0.6f") prints for
 * (double)votes / (double)total, worked out from the double's bits in integers (rounded to nearest, ties to even).  Both set sizes must
 * be at least 1: the rows of an empty set ("inf", "nan") are the host's.
 *   hast_rs_rows_device   the rows of n reads from device arrays (names back to back, name_off[n + 1], votes[n][2]) to d_out, on the
 *                         context's stream; returns when they are written.  *bytes = their size, count[] = reads per class.  More than
 *                         cap bytes (or 2^32 and more): HAST_ERR_UNSUPPORTED, *bytes = what is needed, nothing written.  A set size of
 *                         0: HAST_ERR_INVALID.
 *   hast_rs_set_rows      mode 0 off, 1 on; total0 / total1: the two set sizes, at least 1 each, and the bins' if those are on
 *                         (HAST_ERR_INVALID otherwise).  Only while no submitted block waits for _next.  The row buffers, device and
 *                         pinned, hold block_bytes of text (half a view; real reads need about 0.15 x their bytes); they are allocated
 *                         at the first switch-on and go with hast_rs_destroy.
 *   hast_rs_next_rows     hast_rs_next_binned (bins may be NULL) plus the rows of the same view: rows->text (pinned, valid until the next
 *                         call), rows->bytes, rows->count[].  Names and votes are then NOT downloaded: out->names, name_off and votes
 *                         are NULL.  A view whose rows outgrow the buffer -- records of a few bytes each: ">\nA\n" needs 3.75 x its
 *                         bytes -- comes back with rows->on_host = 1, text = NULL and names and votes as hast_rs_next gives them, for the
 *                         caller to format.  flags != 0 as in hast_rs_next, *rows all zero; so it is with the rows switched off. */
typedef struct hast_rs hast_rs;
typedef struct {
    uint64_t consumed, records, bases, name_bytes;
    uint32_t flags;
    const uint32_t *votes;     /* [records][2], pinned: hits0, hits1 */
    const uint32_t *name_off;  /* [records + 1] */
    const uint8_t *names;
} hast_rs_block;
#define HAST_RS_FASTA 0
#define HAST_RS_FASTQ 1
#define HAST_RS_FORMAT_ERROR    1u   /* '>' header in fastq / '@','+' line in fasta: nothing classified */
#define HAST_RS_RECORD_TOO_LONG 4u
hast_status hast_rs_create(hast_ctx *, int format, size_t block_bytes, hast_rs **out);
hast_status hast_rs_host_block(hast_rs *, uint8_t **h_buf);
hast_status hast_rs_device_block(hast_rs *, uint8_t **d_buf, hast_stream *fill);
hast_status hast_rs_submit(hast_rs *, size_t n_bytes, int last);
hast_status hast_rs_next(hast_rs *, hast_rs_block *out);
typedef struct {
    const uint8_t *run[3];      /* pinned, valid until the next hast_rs_next_binned; class 0, 1, 2 */
    uint64_t run_bytes[3];      /* plain: the run; gzip: ONE complete gzip member, 0 bytes for an empty run */
    uint64_t raw_bytes[3];      /* the runs' plain sizes either way */
    uint64_t count[3];          /* records per class */
} hast_rs_binned;
hast_status hast_rs_set_bins(hast_rs *, int mode /* 0 off, 1 plain, 2 gzip */, uint32_t total0, uint32_t total1);
hast_status hast_rs_next_binned(hast_rs *, hast_rs_block *out, hast_rs_binned *bins);
typedef struct {
    const uint8_t *text;        /* pinned, valid until the next hast_rs_next_rows; NULL with on_host */
    uint64_t bytes;
    uint64_t count[3];          /* reads per class */
    uint32_t on_host;           /* 1: the rows did not fit; names and votes of *out are there instead */
} hast_rs_rows;
hast_status hast_rs_rows_device(hast_ctx *, const uint8_t *d_names, const uint32_t *d_name_off, const uint32_t *d_votes, size_t n, uint32_t total0,
                                uint32_t total1, uint8_t *d_out, size_t cap, uint64_t *bytes, uint64_t count[3]);
hast_status hast_rs_set_rows(hast_rs *, int mode /* 0 off, 1 on */, uint32_t total0, uint32_t total1);
hast_status hast_rs_next_rows(hast_rs *, hast_rs_block *out, hast_rs_binned *bins_or_null, hast_rs_rows *rows);
hast_status hast_rs_take_tail(hast_rs *, uint8_t *dst, size_t *n_bytes);
void        hast_rs_destroy(hast_rs *);

/* ---- stage 02: stLFR pairs -> 10x FASTQ (02.assemble_by_supernova/fake_10x.pl) ----------------------------------------------
 * The script's conversion, on the host (hast_tx_pair_host: no GPU is touched) and over device memory (hast_tx_pair_device):
 * record i of read 1 goes with record i of read 2; the key in read 1's
 * header (the text after the first '#' of the header's first tab field, up to the next '#' or '/') is looked up in the map file; a
 * pair whose key the map lacks is dropped, a pair it holds is numbered (N, from 1) and both records rewritten
 * (hast_amd/csrc/tx_core.h has the rules, tx_host.h the model).
 * hast_tx_map_load / hast_tx_map_parse read the map as perl does (split at tabs, a later line wins, no tab: the empty value).
 * info.device_ok == 0 with info.reason: a device path with 16-byte text records could not take this map (an empty key, a key over 15
 * bytes, a value over 16).
 * hast_tx_pair_host converts r1[0, n1) / r2[0, n2) with the running state (*state: N so far, read-1 headers so far; updated).
 * final == 0: the whole pairs only, res->consumed1/2 = the byte behind them, the caller carries the rest in front of the next bytes.
 * final == 1: the inputs end here; everything is converted the way the script ends (missing lines are empty, an unterminated line
 * gets no newline, a partial read-1 record whose key the map holds is numbered).  final == 2: read 2 has ended (r2 is all that is
 * left of it, less than a record) while read 1 goes on: the whole records of r1, paired with what r2 still has and then with nothing.
 * *out1 / *out2 are malloc'ed (hast_tx_free), res->raw_bytes = res->out_bytes = their sizes, res->pairs = the read-1 headers
 * converted, res->used = the pairs kept, res->lines = the newlines of the two inputs.  The script's progress line is due whenever
 * state->headers passes a multiple of 1 000 000. */
typedef struct hast_tx_map hast_tx_map;
typedef struct { uint64_t n_keys; int device_ok; char reason[60]; } hast_tx_map_info;
typedef struct { uint64_t used, headers; } hast_tx_state;
typedef struct { uint64_t consumed1, consumed2, pairs, used, out_bytes[2], raw_bytes[2]; uint32_t lines[2]; } hast_tx_result;
hast_status hast_tx_map_load(const char *path, hast_tx_map **out, hast_tx_map_info *info);
hast_status hast_tx_map_parse(const uint8_t *text, size_t n_bytes, hast_tx_map **out, hast_tx_map_info *info);
void        hast_tx_map_destroy(hast_tx_map *);
hast_status hast_tx_pair_host(const hast_tx_map *, const uint8_t *r1, size_t n1, const uint8_t *r2, size_t n2, int final, hast_tx_state *state,
                              uint8_t **out1, uint8_t **out2, hast_tx_result *res);
void        hast_tx_free(void *);
/* the `final` of the next hast_tx_pair_host call over what a caller has read and not converted yet; eof1 / eof2: that input has been
 * read to its end.  1 also when read 1 has ended without a whole record and read 2 holds one (the script takes no more than that). */
int         hast_tx_step_mode(int eof1, int eof2, const uint8_t *r1, size_t n1, const uint8_t *r2, size_t n2);
/* The same conversion over device memory (hast_amd/csrc/tx_kernels.hip; what is decided per record: tx_plan.h).
 * hast_tx_create uploads the map as a read-only table and allocates, once, the scratch of the worst step of max_in_bytes a side
 * (at most 128 MB: offsets inside a step are 32 bits wide; more is HAST_ERR_INVALID).  A map with info.device_ok == 0 is
 * HAST_ERR_UNSUPPORTED, with info.reason in hast_last_error().
 * hast_tx_pair_device is hast_tx_pair_host with final == 0 over d_r1[0, n1) / d_r2[0, n2), which may lie at any address: every field
 * of *res, the updated *state and every byte written to d_out1 / d_out2 equal the host call's.  It runs on the given stream (NULL: the
 * context's), allocates nothing, and returns when *res is valid and the outputs are written.  n1 or n2 above max_in_bytes:
 * HAST_ERR_INVALID.  An output larger than its room (cap1, cap2): HAST_ERR_UNSUPPORTED, res->out_bytes = what would have been
 * needed, *state unchanged, not one byte written -- the caller converts this step another way.  No whole pair: HAST_OK, *res all zeros
 * but lines, nothing written.  The end-of-input modes (final 1 and 2: a few records per run) stay with hast_tx_pair_host. */
typedef struct hast_tx hast_tx;
hast_status hast_tx_create(hast_ctx *, const hast_tx_map *, size_t max_in_bytes, hast_tx **out);
hast_status hast_tx_pair_device(hast_tx *, const uint8_t *d_r1, size_t n1, const uint8_t *d_r2, size_t n2, hast_tx_state *state,
                                uint8_t *d_out1, size_t cap1, uint8_t *d_out2, size_t cap2, hast_tx_result *res, hast_stream);
void        hast_tx_destroy(hast_tx *);
/* A step from host memory to host memory, as `fake_10x --convert device` takes it: r1 / r2 go through pinned staging to the device,
 * are converted there (hast_tx_pair_device with room for 2 x the bytes given + 4 KB a side), each run is, with gz != 0, made one gzip
 * member by hast_dz_compress_device (an empty run: no member), and what results comes back to pinned memory: *out1 / *out2, the
 * library's, res->out_bytes[] bytes, valid until the next call BUT ONE returns -- whoever writes them out may do so beside the next
 * step.  res->raw_bytes[] = the runs' sizes before deflate.  The buffers are allocated at the first call.  Inputs larger than the
 * converter was created for, or outputs larger than that room: HAST_ERR_UNSUPPORTED, *state unchanged, the caller takes
 * hast_tx_pair_host.  *times is ADDED to: seconds of upload, of the kernels (a hipEvent pair around them), of deflate, of download. */
typedef struct { double upload_s, kernel_s, deflate_s, download_s; } hast_tx_times;
hast_status hast_tx_pair_staged(hast_tx *, const uint8_t *r1, size_t n1, const uint8_t *r2, size_t n2, hast_tx_state *state, int gz,
                                const uint8_t **out1, const uint8_t **out2, hast_tx_result *res, hast_tx_times *times);
/* The paired, pipelined device route of one fake_10x run (`fake_10x --convert device --inflate device`; hast_amd/csrc/tx_feed.cpp,
 * the reading rule: tx_feed_plan.h): both inputs' bytes are WRITTEN IN HBM (hast_gz_read_device) or uploaded from pinned memory, the
 * whole pairs of every step converted there, both runs deflated as ONE job of the GPU's encoder on a second stream and downloaded
 * while the next step is read and converted.  side: 0 = read 1, 1 = read 2.  One feed per hast_tx; the map the hast_tx was created from
 * must outlive the feed (a step whose outputs outgrow their room is converted by hast_tx_pair_host).
 *   hast_tx_feed_create        ALL device and pinned memory, once: per side two input slots of room bytes (room = 2 * block_bytes + 4096,
 *                              at least 1 MB; above 128 MB or above what the hast_tx was created for: HAST_ERR_UNSUPPORTED), two output
 *                              slots for both runs (2 x room + 4 KB a side), with gz_out the encoder's workspace and member buffers, two
 *                              pinned result slots.  No later call allocates or frees device memory.
 *   hast_tx_feed_wants         1: this side reads for the next step (up to block_bytes); 0: it has been read to its end (a submit of
 *                              fewer than block_bytes), has read already, or holds more than a block with a whole record in it -- known
 *                              from the step before (lines - 4 * pairs >= 4), no byte is looked at on the host
 *   hast_tx_feed_device_block  where the caller's kernels on *fill_stream (the feed's converting stream) write the side's next up to
 *                              block_bytes: directly behind the bytes the side carries, so a step sees one contiguous range
 *   hast_tx_feed_host_block    pinned memory for them instead (plain FASTQ, a pipe); _submit uploads it on a stream of the feed's own
 *   hast_tx_feed_submit        n_bytes (0 .. block_bytes) of the block just handed out are valid; fewer than block_bytes: the side's end
 *   hast_tx_feed_step          hast_tx_pair_host(final = 0) over carry + submitted bytes of both sides (a side that did not read: its
 *                              carry alone): *res (out_bytes = raw_bytes = the runs' sizes) and *state are exactly its.  What is left
 *                              is copied to the front of the side's other slot, the runs' deflate (gz_out: one job of two runs) is
 *                              enqueued on a second stream, and the call returns; the download, whose size only the encoder knows,
 *                              is _collect's, on a stream of its own.  *flags: HAST_TX_ON_HOST the outputs outgrew their room and
 *                              the step was converted by hast_tx_pair_host (deflated by zlib, level 6, with gz_out), results handed on
 *                              the same way; HAST_TX_ENDS hast_tx_step_mode over what this step was given is 1 or 2 (an input has ended
 *                              and left no whole record): nothing was converted, NO collect is due for this step, the caller takes both
 *                              tails and ends on the host; HAST_TX_TAIL_TOO_LONG the step stands, but a side that has to read next
 *                              carries more than room - block_bytes (a record longer than the buffers): collect, take the tails, go on
 *                              on the host.  At most two steps may be waiting for _collect.
 *   hast_tx_feed_collect       waits for the oldest step not yet collected: *out1 / *out2 (pinned, the feed's) hold out_bytes[] bytes --
 *                              with gz_out one gzip member per run that had bytes, else the runs as they are -- and stay valid until the
 *                              next collect BUT ONE returns; raw_bytes[] = the runs' sizes.  A caller that steps n + 1 before it
 *                              collects n has n's deflate and download run beside n + 1's inflate, upload and conversion.
 *   hast_tx_feed_take_tail     the bytes a side holds -- what the last step left, and after a step that said HAST_TX_ENDS everything that
 *                              step was given -- to dst (hast_tx_feed_room bytes of room); the side then holds nothing.
 *   hast_tx_feed_times         *times is ADDED to as by hast_tx_pair_staged (deflate_s / download_s: what the collects waited for);
 *                              *collect_wait_s = the seconds spent waiting inside hast_tx_feed_collect */
typedef struct hast_tx_feed hast_tx_feed;
#define HAST_TX_ON_HOST 1u
#define HAST_TX_TAIL_TOO_LONG 4u
#define HAST_TX_ENDS 8u
hast_status hast_tx_feed_create(hast_tx *, size_t block_bytes, int gz_out, hast_tx_feed **out);
int         hast_tx_feed_wants(const hast_tx_feed *, int side);
size_t      hast_tx_feed_room(const hast_tx_feed *);
hast_status hast_tx_feed_device_block(hast_tx_feed *, int side, uint8_t **d_buf, hast_stream *fill_stream);
hast_status hast_tx_feed_host_block(hast_tx_feed *, int side, uint8_t **h_buf);
hast_status hast_tx_feed_submit(hast_tx_feed *, int side, size_t n_bytes);
hast_status hast_tx_feed_step(hast_tx_feed *, hast_tx_state *state, hast_tx_result *res, int *flags);
hast_status hast_tx_feed_collect(hast_tx_feed *, const uint8_t **out1, const uint8_t **out2, uint64_t out_bytes[2], uint64_t raw_bytes[2]);
hast_status hast_tx_feed_take_tail(hast_tx_feed *, int side, uint8_t *dst, size_t *n_bytes);
hast_status hast_tx_feed_times(const hast_tx_feed *, hast_tx_times *times, double *collect_wait_s);
void        hast_tx_feed_destroy(hast_tx_feed *);

#ifdef __cplusplus
}
#endif
#endif
