"""ctypes binding of libhast.so (include/hast.h).  Loads the in-tree build; fails loudly if absent."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

u8p, u32p, u64p, vp = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.c_void_p

STATUS = {0: "OK", 1: "INVALID", 2: "NO_DEVICE", 3: "HIP", 4: "OOM", 5: "TABLE_FULL", 6: "FORMAT", 7: "RCCL", 8: "IO", 9: "UNSUPPORTED"}


class SynthParams(C.Structure):
    _fields_ = [("seed_k", C.c_uint64), ("seed_r", C.c_uint64), ("seed_b", C.c_uint64),
                ("n_keys_per_hap", C.c_uint64), ("n_barcodes", C.c_uint32), ("read_len", C.c_uint32),
                ("k", C.c_uint32), ("reserved", C.c_uint32)]


class KcSynth(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("genome_len", C.c_uint64), ("read_len", C.c_uint32), ("snp_per_1024", C.c_uint32),
                ("err_per_4096", C.c_uint32), ("n_per_4096", C.c_uint32)]


class FqBlock(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("n_bases", C.c_uint64), ("max_read_len", C.c_uint32), ("short_read", C.c_uint32),
                ("bytes", C.POINTER(C.c_uint8)), ("bc_pos", C.POINTER(C.c_uint32)), ("bc_len", C.POINTER(C.c_uint32)),
                ("bc_text", C.POINTER(C.c_uint8)), ("ids", C.POINTER(C.c_uint32)), ("unknown", C.POINTER(C.c_uint32)),
                ("n_unknown", C.c_uint64), ("dict_ids", C.c_uint64)]


class FqRouted(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("count", C.c_uint64 * 4), ("run", C.POINTER(C.c_uint8) * 4), ("run_bytes", C.c_uint64 * 4),
                ("host_block", C.c_int), ("bytes", C.POINTER(C.c_uint8)), ("rec_start", C.POINTER(C.c_uint32)), ("rec_len", C.POINTER(C.c_uint32)),
                ("rec_class", C.POINTER(C.c_uint8)), ("n_slots", C.c_uint64), ("tail", C.POINTER(C.c_uint8)), ("tail_bytes", C.c_uint64)]


class FqTallied(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("n_counted", C.c_uint64), ("n_nofield", C.c_uint64), ("n_left", C.c_uint64),
                ("left_pos", C.POINTER(C.c_uint32)), ("left_len", C.POINTER(C.c_uint32)), ("bytes", C.POINTER(C.c_uint8)),
                ("tail", C.POINTER(C.c_uint8)), ("tail_bytes", C.c_uint64)]


class GzStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("compressed_bytes", "out_bytes", "chunks", "accepted", "followup_jobs", "followup_rounds", "followup_accepted", "members")] + \
               [(n, C.c_double) for n in ("decode_s", "windows_crc_s", "wait_upload_s", "wait_consumer_s", "wait_decode_s", "open_s")] + \
               [(n, C.c_uint64) for n in ("ring_bytes", "upload_waited_for_ring")] + [("chain_walk_s", C.c_double), ("ring_laps", C.c_uint64)]


class GzBlockedStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("members", "batches", "carried")] + \
               [(n, C.c_double) for n in ("read_s", "upload_s", "kernels_s", "wait_reader_s")] + [("unsupported_offset", C.c_uint64)]


class SqResult(C.Structure):
    _fields_ = [("consumed", C.c_uint64), ("out_bytes", C.c_uint64), ("records", C.c_uint64), ("bases", C.c_uint64),
                ("flags", C.c_uint32), ("first_bad", C.c_uint32)]


class RsBlock(C.Structure):
    _fields_ = [("consumed", C.c_uint64), ("records", C.c_uint64), ("bases", C.c_uint64), ("name_bytes", C.c_uint64), ("flags", C.c_uint32),
                ("votes", C.POINTER(C.c_uint32)), ("name_off", C.POINTER(C.c_uint32)), ("names", C.POINTER(C.c_uint8))]


class RsBinned(C.Structure):
    _fields_ = [("run", C.POINTER(C.c_uint8) * 3), ("run_bytes", C.c_uint64 * 3), ("raw_bytes", C.c_uint64 * 3), ("count", C.c_uint64 * 3)]


class RsRows(C.Structure):
    _fields_ = [("text", C.POINTER(C.c_uint8)), ("bytes", C.c_uint64), ("count", C.c_uint64 * 3), ("on_host", C.c_uint32)]


class TxMapInfo(C.Structure):
    _fields_ = [("n_keys", C.c_uint64), ("device_ok", C.c_int), ("reason", C.c_char * 60)]


class TxState(C.Structure):
    _fields_ = [("used", C.c_uint64), ("headers", C.c_uint64)]


class TxResult(C.Structure):
    _fields_ = [("consumed1", C.c_uint64), ("consumed2", C.c_uint64), ("pairs", C.c_uint64), ("used", C.c_uint64),
                ("out_bytes", C.c_uint64 * 2), ("raw_bytes", C.c_uint64 * 2), ("lines", C.c_uint32 * 2)]


class TxTimes(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("upload_s", "kernel_s", "deflate_s", "download_s")]


class RowsInfo(C.Structure):
    _fields_ = [("n_rows", C.c_uint64), ("table_bytes", C.c_uint64), ("list_bytes", C.c_uint64 * 3), ("any_sep", C.c_int), ("past_int", C.c_int),
                ("keys_s", C.c_double), ("sort_s", C.c_double), ("format_s", C.c_double)]


SQ_NOT_FOUR_LINE, SQ_NO_RECORD, SQ_TAIL_TOO_LONG = 1, 2, 4
SQ_FA_OPEN, SQ_FA_LAST = 1, 2
SQ_TAKE_FASTQ, SQ_TAKE_FASTA = 1, 2
RS_FASTA, RS_FASTQ = 0, 1
RS_FORMAT_ERROR, RS_RECORD_TOO_LONG = 1, 4
KC_HISTO_HIGH = 10000

# every symbol include/hast.h declares: name -> (restype, argtypes)
ABI_SYMBOLS = {
    "hast_version": (C.c_char_p, []),
    "hast_last_error": (C.c_char_p, []),
    "hast_ctx_create": (C.c_int, [C.c_int, C.c_int, C.POINTER(vp)]),
    "hast_ctx_destroy": (None, [vp]),
    "hast_release_parked": (None, []),
    "hast_ctx_k": (C.c_int, [vp]),
    "hast_ctx_minimizer": (C.c_int, [vp]),
    "hast_ctx_set_minimizer": (C.c_int, [vp, C.c_int]),
    "hast_ctx_device": (C.c_int, [vp]),
    "hast_ctx_set_option": (C.c_int, [vp, C.c_char_p, C.c_long]),
    "hast_ctx_options": (C.c_int, [vp, C.c_char_p, C.c_size_t]),
    "hast_ctx_stream": (vp, [vp]),
    "hast_stream_sync": (C.c_int, [vp, vp]),
    "hast_dev_alloc": (C.c_int, [vp, C.c_size_t, C.POINTER(vp)]),
    "hast_dev_free": (C.c_int, [vp, vp]),
    "hast_memcpy_h2d": (C.c_int, [vp, vp, vp, C.c_size_t]),
    "hast_memcpy_d2h": (C.c_int, [vp, vp, vp, C.c_size_t]),
    "hast_memset_d": (C.c_int, [vp, vp, C.c_int, C.c_size_t, vp]),
    "hast_table_reserve": (C.c_int, [vp, C.c_uint64, C.c_double]),
    "hast_table_insert_text": (C.c_int, [vp, C.c_int, C.c_char_p, C.c_size_t, u64p]),
    "hast_table_insert_text_file": (C.c_int, [vp, C.c_int, C.c_char_p, u64p]),
    "hast_ctx_set_text_check": (C.c_int, [vp, C.c_int]),
    "hast_table_insert_keys": (C.c_int, [vp, C.c_int, vp, C.c_size_t]),
    "hast_table_insert_keys_device": (C.c_int, [vp, C.c_int, vp, C.c_size_t, vp]),
    "hast_table_erase": (C.c_int, [vp, vp, C.c_size_t, vp]),
    "hast_table_sizes": (C.c_int, [vp, u64p, u64p]),
    "hast_table_lookup": (C.c_int, [vp, vp, C.c_size_t, vp]),
    "hast_table_save": (C.c_int, [vp, C.c_char_p]),
    "hast_table_load": (C.c_int, [vp, C.c_char_p, C.c_double]),
    "hast_table_file_info": (C.c_int, [C.c_char_p, C.POINTER(C.c_int), u64p]),
    "hast_table_info": (C.c_int, [vp, u64p, u64p]),
    "hast_table_clone": (C.c_int, [vp, vp]),
    "hast_ctx_set_filter": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int]),
    "hast_filter_build": (C.c_int, [vp]),
    "hast_filter_info": (C.c_int, [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), u64p]),
    "hast_filter_dense": (C.c_int, [vp, C.POINTER(C.c_int)]),
    "hast_filter_request_ceiling": (C.c_int, [vp, C.POINTER(C.c_double)]),
    "hast_filter_lookups": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
    "hast_counts_resize": (C.c_int, [vp, C.c_size_t]),
    "hast_counts_bind": (C.c_int, [vp, vp, C.c_size_t]),
    "hast_counts_zero": (C.c_int, [vp, vp]),
    "hast_counts_read": (C.c_int, [vp, vp, vp, vp, C.c_size_t]),
    "hast_counts_pack": (C.c_int, [vp, vp, C.c_size_t, vp]),
    "hast_counts_unpack": (C.c_int, [vp, vp, C.c_size_t, vp]),
    "hast_counts_add_votes": (C.c_int, [vp, vp, vp, C.c_size_t, C.c_uint32, vp]),
    "hast_counts_allreduce": (C.c_int, [C.POINTER(vp), C.c_int]),
    "hast_classify_timing": (C.c_int, [vp, C.c_int]),
    "hast_classify_times": (C.c_int, [vp, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_int)]),
    "hast_classify_device": (C.c_int, [vp, vp, C.c_size_t, vp, C.c_uint32, vp, vp, C.c_size_t, vp]),
    "hast_classify_batch": (C.c_int, [vp, vp, vp, vp, C.c_size_t, C.c_uint32]),
    "hast_classify_perread_device": (C.c_int, [vp, vp, C.c_size_t, vp, C.c_size_t, vp, vp]),
    "hast_classify_perread": (C.c_int, [vp, vp, vp, C.c_size_t, vp]),
    "hast_batch_begin": (C.c_int, [vp, C.c_size_t, C.c_size_t, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]),
    "hast_batch_submit": (C.c_int, [vp, C.c_size_t, C.c_uint32]),
    "hast_names_create": (C.c_int, [vp, C.c_size_t, C.POINTER(vp)]),
    "hast_names_destroy": (None, [vp]),
    "hast_fq_create": (C.c_int, [vp, C.c_size_t, C.c_int, vp, C.POINTER(vp)]),
    "hast_fq_create_ex": (C.c_int, [vp, C.c_size_t, C.c_int, vp, C.c_int, C.POINTER(vp)]),
    "hast_fq_create_striped": (C.c_int, [C.POINTER(vp), C.c_int, C.c_size_t, C.c_int, C.POINTER(vp), C.POINTER(vp)]),
    "hast_fq_create_striped_ex": (C.c_int, [C.POINTER(vp), C.c_int, C.c_size_t, C.c_int, C.POINTER(vp), C.c_int, C.POINTER(vp)]),
    "hast_fq_lanes": (C.c_int, [vp]),
    "hast_fq_lane_records": (C.c_uint64, [vp, C.c_int]),
    "hast_fq_destroy": (None, [vp]),
    "hast_fq_block_bytes": (C.c_size_t, [vp]),
    "hast_fq_acquire": (C.c_int, [vp, C.POINTER(C.POINTER(C.c_uint8))]),
    "hast_fq_submit": (C.c_int, [vp, C.c_size_t, C.c_int]),
    "hast_fq_device_block": (C.c_int, [vp, C.POINTER(vp), C.POINTER(vp)]),
    "hast_fq_submit_device": (C.c_int, [vp, C.c_size_t, C.c_int]),
    "hast_fq_block_host_bytes": (C.c_int, [vp, C.POINTER(C.POINTER(C.c_uint8))]),
    "hast_fq_poll": (C.c_int, [vp]),
    "hast_fq_next": (C.c_int, [vp, C.POINTER(FqBlock)]),
    "hast_fq_commit": (C.c_int, [vp]),
    "hast_dev_mem_info": (C.c_int, [vp, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "hast_names_create_dict": (C.c_int, [vp, C.c_size_t, C.POINTER(vp)]),
    "hast_names_limit": (C.c_size_t, [vp]),
    "hast_names_count": (C.c_int, [vp, C.POINTER(C.c_size_t)]),
    "hast_names_texts": (C.c_int, [vp, C.c_size_t, C.c_size_t, C.POINTER(C.c_uint8)]),
    "hast_counts_read_range": (C.c_int, [vp, C.c_size_t, C.c_size_t, u64p, u64p, u64p]),
    "hast_names_merge": (C.c_int, [vp, vp, C.c_size_t, C.c_size_t, C.POINTER(C.c_uint32)]),
    "hast_counts_permute": (C.c_int, [vp, C.POINTER(C.c_uint32), C.c_size_t, C.c_size_t]),
    "hast_names_insert": (C.c_int, [vp, C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.c_size_t]),
    "hast_fq_set_route": (C.c_int, [vp, C.POINTER(vp), C.c_int]),
    "hast_fq_next_routed": (C.c_int, [vp, C.POINTER(FqRouted)]),
    "hast_fq_set_route_gz": (C.c_int, [vp, C.c_int]),
    "hast_fq_routed_raw_bytes": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
    # stage 02: per-barcode read counts (barcode_freq.txt)
    "hast_tally_create": (C.c_int, [vp, C.c_size_t, C.POINTER(vp)]),
    "hast_tally_limit": (C.c_size_t, [vp]),
    "hast_tally_size": (C.c_int, [vp, C.POINTER(C.c_size_t)]),
    "hast_tally_read": (C.c_int, [vp, C.c_size_t, C.c_size_t, C.POINTER(C.c_uint8), u64p]),
    "hast_tally_destroy": (None, [vp]),
    "hast_fq_set_tally": (C.c_int, [vp, C.POINTER(vp), C.c_int]),
    "hast_fq_next_tallied": (C.c_int, [vp, C.POINTER(FqTallied)]),
    "hast_dz_bound": (C.c_size_t, [C.c_size_t]),
    "hast_dz_compress_device": (C.c_int, [vp, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t), vp]),
    "hast_dz_compress_device_ex": (C.c_int, [vp, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t), C.c_uint, vp]),
    "hast_dz_bound_blocked": (C.c_size_t, [C.c_size_t]),
    "hast_dz_compress_blocked_device": (C.c_int, [vp, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t), vp]),
    "hast_rows_build_device": (C.c_int, [vp, vp, vp, C.c_size_t, C.c_uint64, C.c_uint64, C.c_double, C.c_double, C.c_int, C.POINTER(vp)]),
    "hast_rows_build": (C.c_int, [vp, vp, C.c_size_t, C.c_uint64, C.c_uint64, C.c_double, C.c_double, C.c_int, C.POINTER(vp)]),
    "hast_rows_get_info": (C.c_int, [vp, C.POINTER(RowsInfo)]),
    "hast_rows_read": (C.c_int, [vp, C.c_int, C.c_uint64, C.c_size_t, vp]),
    "hast_rows_order": (C.c_int, [vp, C.POINTER(C.c_uint32)]),
    "hast_rows_classes": (C.c_int, [vp, C.POINTER(C.c_uint8)]),
    "hast_rows_destroy": (None, [vp]),
    "hast_gz_open": (C.c_int, [vp, C.c_char_p, C.POINTER(vp)]),
    "hast_gz_open_ex": (C.c_int, [vp, C.c_char_p, C.c_size_t, C.c_size_t, C.c_double, C.POINTER(vp)]),
    "hast_gz_open_multi": (C.c_int, [C.POINTER(vp), C.c_int, C.c_char_p, C.POINTER(vp)]),
    "hast_gz_open_multi_ex": (C.c_int, [C.POINTER(vp), C.c_int, C.c_char_p, C.c_size_t, C.c_size_t, C.c_double, C.POINTER(vp)]),
    "hast_gz_units": (C.c_int, [vp]),
    "hast_gz_read_device": (C.c_int, [vp, vp, C.c_size_t, C.POINTER(C.c_size_t), vp]),
    "hast_gz_get_stats": (C.c_int, [vp, C.POINTER(GzStats)]),
    "hast_gz_close": (None, [vp]),
    "hast_gz_open_blocked": (C.c_int, [vp, C.c_char_p, C.POINTER(vp)]),
    "hast_gz_open_blocked_ex": (C.c_int, [vp, C.c_char_p, C.c_size_t, C.c_size_t, C.POINTER(vp)]),
    "hast_gz_get_blocked_stats": (C.c_int, [vp, C.POINTER(GzBlockedStats)]),
    "hast_parse_barcode": (None, [C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "hast_get_hap": (C.c_int, [C.c_char_p, C.c_size_t, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_double, C.c_double]),
    "hast_canon_kmer": (C.c_uint64, [C.c_char_p, C.c_int]),
    "hast_chop_read": (C.c_size_t, [C.c_char_p, C.c_size_t, C.c_int, u64p]),
    "hast_kmer_to_str": (None, [C.c_uint64, C.c_int, C.c_char_p]),
    "hast_synth_keys_host": (C.c_int, [C.POINTER(SynthParams), C.c_int, C.c_uint64, C.c_size_t, vp]),
    "hast_synth_reads_host": (C.c_int, [C.POINTER(SynthParams), C.c_uint64, C.c_size_t, vp, vp]),
    "hast_synth_keys_device": (C.c_int, [vp, C.POINTER(SynthParams), C.c_int, C.c_uint64, C.c_size_t, vp, vp]),
    "hast_synth_reads_device": (C.c_int, [vp, C.POINTER(SynthParams), C.c_uint64, C.c_size_t, vp, vp, vp]),
    "hast_synth_table_build": (C.c_int, [vp, C.POINTER(SynthParams)]),
    # stage 00: parent-unique k-mer sets
    "hast_kc_create": (C.c_int, [C.c_int, C.c_int, C.c_size_t, C.POINTER(vp)]),
    "hast_kc_create_ex": (C.c_int, [C.c_int, C.c_int, C.c_size_t, C.c_uint64, C.POINTER(vp)]),
    "hast_kc_destroy": (None, [vp]),
    "hast_kc_stream": (vp, [vp]),
    "hast_kc_set_slice": (C.c_int, [vp, C.c_uint32, C.c_uint32]),
    "hast_kc_count_device": (C.c_int, [vp, C.c_int, vp, C.c_size_t]),
    "hast_kc_count": (C.c_int, [vp, C.c_int, vp, C.c_size_t]),
    "hast_kc_sync": (C.c_int, [vp]),
    "hast_kc_partition_info": (C.c_int, [vp, u64p]),
    "hast_kc_stats": (C.c_int, [vp, u64p]),
    "hast_kc_histo": (C.c_int, [vp, C.c_int, vp]),
    "hast_kc_find_bounds": (None, [vp, C.POINTER(C.c_long)]),
    "hast_kc_select": (C.c_int, [vp, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_size_t)]),
    "hast_kc_selection_clear": (C.c_int, [vp]),
    "hast_kc_selection_adopt": (C.c_int, [vp, vp]),
    "hast_kc_release_table": (C.c_int, [vp]),
    "hast_kc_selection_sort": (C.c_int, [vp, C.c_int, C.POINTER(C.c_size_t)]),
    "hast_kc_selection_text": (C.c_int, [vp, C.c_int, C.c_size_t, C.c_size_t, vp]),
    "hast_kc_selection_keys": (C.c_int, [vp, C.c_int, C.c_size_t, C.c_size_t, vp]),
    "hast_kc_synth_host": (C.c_int, [C.POINTER(KcSynth), C.c_int, C.c_uint64, C.c_size_t, vp]),
    "hast_kc_synth_device": (C.c_int, [vp, C.POINTER(KcSynth), C.c_int, C.c_uint64, C.c_size_t, vp]),
    # stage 00 ingest on the device: four-line FASTQ in HBM -> the counter's base stream
    "hast_sq_create": (C.c_int, [vp, C.c_size_t, C.POINTER(vp)]),
    "hast_sq_frame_device": (C.c_int, [vp, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(SqResult)]),
    "hast_sq_frame_fasta_device": (C.c_int, [vp, vp, C.c_size_t, vp, C.c_size_t, C.c_uint, C.POINTER(SqResult)]),
    "hast_sq_destroy": (None, [vp]),
    "hast_sq_feed_create": (C.c_int, [vp, C.c_size_t, C.POINTER(vp)]),
    "hast_sq_feed_host_block": (C.c_int, [vp, C.POINTER(vp)]),
    "hast_sq_feed_device_block": (C.c_int, [vp, C.POINTER(vp)]),
    "hast_sq_feed_submit": (C.c_int, [vp, C.c_size_t]),
    "hast_sq_feed_next": (C.c_int, [vp, C.c_int, C.POINTER(SqResult)]),
    "hast_sq_feed_take_tail": (C.c_int, [vp, vp, C.POINTER(C.c_size_t)]),
    "hast_sq_feed_destroy": (None, [vp]),
    "hast_sq_feed_set_formats": (C.c_int, [vp, C.c_uint]),
    "hast_sq_feed_format": (C.c_int, [vp]),
    "hast_sq_feed_finish": (C.c_int, [vp, C.c_int, C.POINTER(SqResult)]),
    "hast_rs_create": (C.c_int, [vp, C.c_int, C.c_size_t, C.POINTER(vp)]),
    "hast_rs_host_block": (C.c_int, [vp, C.POINTER(vp)]),
    "hast_rs_device_block": (C.c_int, [vp, C.POINTER(vp), C.POINTER(vp)]),
    "hast_rs_submit": (C.c_int, [vp, C.c_size_t, C.c_int]),
    "hast_rs_next": (C.c_int, [vp, C.POINTER(RsBlock)]),
    "hast_rs_take_tail": (C.c_int, [vp, vp, C.POINTER(C.c_size_t)]),
    "hast_rs_set_bins": (C.c_int, [vp, C.c_int, C.c_uint32, C.c_uint32]),
    "hast_rs_next_binned": (C.c_int, [vp, C.POINTER(RsBlock), C.POINTER(RsBinned)]),
    "hast_rs_rows_device": (C.c_int, [vp, vp, vp, vp, C.c_size_t, C.c_uint32, C.c_uint32, vp, C.c_size_t, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64 * 3)]),
    "hast_rs_set_rows": (C.c_int, [vp, C.c_int, C.c_uint32, C.c_uint32]),
    "hast_rs_next_rows": (C.c_int, [vp, C.POINTER(RsBlock), C.POINTER(RsBinned), C.POINTER(RsRows)]),
    "hast_rs_destroy": (None, [vp]),
    # stage 02: stLFR pairs -> 10x FASTQ (fake_10x.pl)
    "hast_tx_map_load": (C.c_int, [C.c_char_p, C.POINTER(vp), C.POINTER(TxMapInfo)]),
    "hast_tx_map_parse": (C.c_int, [C.c_char_p, C.c_size_t, C.POINTER(vp), C.POINTER(TxMapInfo)]),
    "hast_tx_map_destroy": (None, [vp]),
    "hast_tx_pair_host": (C.c_int, [vp, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_int, C.POINTER(TxState), C.POINTER(vp), C.POINTER(vp),
                                    C.POINTER(TxResult)]),
    "hast_tx_free": (None, [vp]),
    "hast_tx_step_mode": (C.c_int, [C.c_int, C.c_int, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]),
    "hast_tx_create": (C.c_int, [vp, vp, C.c_size_t, C.POINTER(vp)]),
    "hast_tx_pair_device": (C.c_int, [vp, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(TxState), vp, C.c_size_t, vp, C.c_size_t, C.POINTER(TxResult), vp]),
    "hast_tx_destroy": (None, [vp]),
    "hast_tx_pair_staged": (C.c_int, [vp, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.POINTER(TxState), C.c_int, C.POINTER(vp), C.POINTER(vp),
                                      C.POINTER(TxResult), C.POINTER(TxTimes)]),
    "hast_tx_feed_create": (C.c_int, [vp, C.c_size_t, C.c_int, C.POINTER(vp)]),
    "hast_tx_feed_wants": (C.c_int, [vp, C.c_int]),
    "hast_tx_feed_room": (C.c_size_t, [vp]),
    "hast_tx_feed_device_block": (C.c_int, [vp, C.c_int, C.POINTER(vp), C.POINTER(vp)]),
    "hast_tx_feed_host_block": (C.c_int, [vp, C.c_int, C.POINTER(vp)]),
    "hast_tx_feed_submit": (C.c_int, [vp, C.c_int, C.c_size_t]),
    "hast_tx_feed_step": (C.c_int, [vp, C.POINTER(TxState), C.POINTER(TxResult), C.POINTER(C.c_int)]),
    "hast_tx_feed_collect": (C.c_int, [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_uint64 * 2), C.POINTER(C.c_uint64 * 2)]),
    "hast_tx_feed_take_tail": (C.c_int, [vp, C.c_int, vp, C.POINTER(C.c_size_t)]),
    "hast_tx_feed_times": (C.c_int, [vp, C.POINTER(TxTimes), C.POINTER(C.c_double)]),
    "hast_tx_feed_destroy": (None, [vp]),
}


def B_ALG_PER_READ(read_len: int, k: int) -> int:
    """Algorithmic HBM bytes per read: every base once + one 64-B line per window."""
    return read_len + max(0, read_len - k + 1) * 64


class HastError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__("hast: %s: %s" % (STATUS.get(status, status), msg))
        self.status = status


def lib_path():
    return os.environ.get("HAST_LIB") or os.path.join(_HERE, "libhast.so")


def classify_exe():
    return os.path.join(_HERE, "classify")


def classify_read_exe():
    return os.path.join(_HERE, "classify_read")


def unshared_kmers_exe():
    return os.path.join(_HERE, "unshared_kmers")


def fake_10x_exe():
    return os.path.join(_HERE, "fake_10x")


def barcode_freq_exe():
    return os.path.join(_HERE, "barcode_freq")


def build(verbose=False):
    """Compile libhast.so + classify for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    res = subprocess.run(["make", "-C", os.path.join(_HERE, "csrc")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if verbose or res.returncode:
        print(res.stdout.decode())
    if res.returncode:
        raise RuntimeError("building libhast.so failed")


def lib():
    """The loaded library.  No fallback: a missing libhast.so is an error."""
    global _LIB
    if _LIB is None:
        p = lib_path()
        if not os.path.exists(p):
            raise RuntimeError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(or make -C hast_amd/csrc); there is no Python/CPU fallback" % p)
        l = C.CDLL(p)
        for name, (res, args) in ABI_SYMBOLS.items():
            f = getattr(l, name)
            f.restype, f.argtypes = res, args
        _LIB = l
    return _LIB


def _ck(st):
    if st != 0:
        raise HastError(st, lib().hast_last_error().decode())


def _ptr(a):
    if a is None:
        return None
    if isinstance(a, int):
        return C.c_void_p(a)
    if isinstance(a, np.ndarray):
        assert a.flags["C_CONTIGUOUS"]
        return C.c_void_p(a.ctypes.data)
    return a


# ---- host-side pieces --------------------------------------------------------------------------
def parse_barcode(head: bytes) -> bytes:
    s, n = C.c_size_t(), C.c_size_t()
    lib().hast_parse_barcode(head, len(head), C.byref(s), C.byref(n))
    return head[s.value:s.value + n.value]


def get_hap(barcode: bytes, c0, c1, n0, n1, w0=1.0, w1=1.0) -> int:
    return lib().hast_get_hap(barcode, len(barcode), c0, c1, n0, n1, w0, w1)


def canon_kmer(s: bytes) -> int:
    return lib().hast_canon_kmer(s, len(s))


def chop_read(seq: bytes, k: int):
    n = max(0, len(seq) - k + 1)
    out = (C.c_uint64 * max(1, n))()
    got = lib().hast_chop_read(seq, len(seq), k, out)
    return [out[i] for i in range(got)]


def make_params(k, read_len=150, n_keys_per_hap=0, n_barcodes=1, seed_k=0, seed_r=0, seed_b=0, clustered=False, no_plants=False):
    return SynthParams(seed_k, seed_r, seed_b, n_keys_per_hap, n_barcodes, read_len, k, (1 if clustered else 0) | (2 if no_plants else 0))


def synth_keys_host(p: SynthParams, hap, first, n):
    out = np.empty(n, dtype=np.uint64)
    _ck(lib().hast_synth_keys_host(C.byref(p), hap, first, n, _ptr(out)))
    return out


def synth_reads_host(p: SynthParams, first, n):
    bases = np.empty(n * p.read_len, dtype=np.uint8)
    ids = np.empty(n, dtype=np.uint32)
    _ck(lib().hast_synth_reads_host(C.byref(p), first, n, _ptr(bases), _ptr(ids)))
    return bases, ids


# ---- device context ----------------------------------------------------------------------------
class Context:
    """One GPU context (hast_ctx).  Raises HastError(NO_DEVICE) when there is no GPU."""

    def __init__(self, k, device=0, minimizer=None):
        self._h = C.c_void_p()
        self._lib = lib()
        _ck(self._lib.hast_ctx_create(device, k, C.byref(self._h)))
        self.k = k
        self.device = device
        if minimizer is not None:
            _ck(self._lib.hast_ctx_set_minimizer(self._h, minimizer))

    @property
    def minimizer(self):
        return self._lib.hast_ctx_minimizer(self._h)

    def set_filter(self, enable=True, m=0, t=0, kp=0):
        """enable: False/0 = probe the table directly, True/1 = filter (exact entries where they fit), 2 = filter with prints always"""
        _ck(self._lib.hast_ctx_set_filter(self._h, int(enable), m, t, kp))

    def filter_build(self):
        _ck(self._lib.hast_filter_build(self._h))

    def filter_request_ceiling(self):
        """requests/s at which this GPU serves random 128-B blocks of this context's filter (measurement entry)"""
        r = C.c_double()
        _ck(self._lib.hast_filter_request_ceiling(self._h, C.byref(r)))
        return r.value

    def filter_info(self):
        """(enabled, m, t, kp, bytes); m = t = kp = bytes = 0 until the filter has been built for the current table"""
        en, m, t, kp, b = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_uint64()
        _ck(self._lib.hast_filter_info(self._h, C.byref(en), C.byref(m), C.byref(t), C.byref(kp), C.byref(b)))
        return bool(en.value), m.value, t.value, kp.value, b.value

    def filter_mode(self):
        """0 = off, 1 = 16-bit prints, 2 = exact entries (hast_common.h); known once the filter has been built"""
        en = C.c_int()
        _ck(self._lib.hast_filter_info(self._h, C.byref(en), None, None, None, None))
        return en.value

    def filter_dense(self):
        """True: the built filter holds exact entries filed under every m-mer of a string (hast_common.h, dense filing)"""
        d = C.c_int()
        _ck(self._lib.hast_filter_dense(self._h, C.byref(d)))
        return bool(d.value)

    def filter_lookups(self):
        """windows k_classify_f has sent to the exact table on this context (HAST_COUNT_LOOKUPS=1 at creation, an error otherwise)"""
        n = C.c_uint64()
        _ck(self._lib.hast_filter_lookups(self._h, C.byref(n)))
        return n.value

    def close(self):
        if self._h:
            self._lib.hast_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def stream(self):
        return self._lib.hast_ctx_stream(self._h)

    def sync(self, stream=None):
        _ck(self._lib.hast_stream_sync(self._h, stream))

    # raw device memory
    def alloc(self, nbytes) -> int:
        p = C.c_void_p()
        _ck(self._lib.hast_dev_alloc(self._h, nbytes, C.byref(p)))
        return p.value

    def free(self, dptr):
        _ck(self._lib.hast_dev_free(self._h, C.c_void_p(dptr)))

    def to_device(self, arr: np.ndarray) -> int:
        arr = np.ascontiguousarray(arr)
        d = self.alloc(max(arr.nbytes, 1))
        _ck(self._lib.hast_memcpy_h2d(self._h, C.c_void_p(d), _ptr(arr), arr.nbytes))
        return d

    def to_host(self, dptr, shape, dtype) -> np.ndarray:
        out = np.empty(shape, dtype=dtype)
        _ck(self._lib.hast_memcpy_d2h(self._h, _ptr(out), C.c_void_p(dptr), out.nbytes))
        return out

    def memset(self, dptr, byte, nbytes, stream=None):
        _ck(self._lib.hast_memset_d(self._h, C.c_void_p(dptr), byte, nbytes, stream))

    # table
    def table_reserve(self, max_keys, load_factor=0.0):
        _ck(self._lib.hast_table_reserve(self._h, max_keys, load_factor))

    def table_insert_text(self, hap, text: bytes) -> int:
        lines = C.c_uint64()
        _ck(self._lib.hast_table_insert_text(self._h, hap, text, len(text), C.byref(lines)))
        return lines.value

    def set_text_check(self, acgt_only=True):
        _ck(self._lib.hast_ctx_set_text_check(self._h, 1 if acgt_only else 0))

    def table_insert_text_file(self, hap, path) -> int:
        lines = C.c_uint64()
        _ck(self._lib.hast_table_insert_text_file(self._h, hap, os.fsencode(path), C.byref(lines)))
        return lines.value

    def table_insert_keys(self, hap, keys: np.ndarray):
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        _ck(self._lib.hast_table_insert_keys(self._h, hap, _ptr(keys), keys.size))

    def table_insert_keys_device(self, hap, d_keys, n, stream=None):
        _ck(self._lib.hast_table_insert_keys_device(self._h, hap, C.c_void_p(d_keys), n, stream))

    def table_erase(self, keys) -> np.ndarray:
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        hit = np.zeros(keys.size, dtype=np.uint8)
        _ck(self._lib.hast_table_erase(self._h, _ptr(keys), keys.size, _ptr(hit)))
        return hit

    def table_sizes(self):
        a, b = C.c_uint64(), C.c_uint64()
        _ck(self._lib.hast_table_sizes(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def table_lookup(self, keys) -> np.ndarray:
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        tags = np.zeros(keys.size, dtype=np.uint8)
        _ck(self._lib.hast_table_lookup(self._h, _ptr(keys), keys.size, _ptr(tags)))
        return tags

    def table_save(self, path):
        _ck(self._lib.hast_table_save(self._h, os.fsencode(path)))

    def table_load(self, path, load_factor=0.0):
        _ck(self._lib.hast_table_load(self._h, os.fsencode(path), load_factor))

    def table_clone_from(self, src):
        _ck(self._lib.hast_table_clone(self._h, src._h))

    def table_info(self):
        a, b = C.c_uint64(), C.c_uint64()
        _ck(self._lib.hast_table_info(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    # counters
    def counts_resize(self, n):
        _ck(self._lib.hast_counts_resize(self._h, n))

    def counts_bind(self, d_counts, n):
        _ck(self._lib.hast_counts_bind(self._h, C.c_void_p(d_counts), n))

    def counts_zero(self, stream=None):
        _ck(self._lib.hast_counts_zero(self._h, stream))

    def counts_read(self, n):
        """(c0, c1, neg) as uint64 arrays: the device counts in 64-bit words (include/hast.h)."""
        c0 = np.zeros(n, dtype=np.uint64)
        c1 = np.zeros(n, dtype=np.uint64)
        neg = np.zeros(n, dtype=np.uint64)
        _ck(self._lib.hast_counts_read(self._h, _ptr(c0), _ptr(c1), _ptr(neg), n))
        return c0, c1, neg

    def counts_pack(self, d_packed, n, stream=None):
        """counts[n][4] -> d_packed = c0[n] | c1[n] | neg[n] (what a caller's own collective moves)"""
        _ck(self._lib.hast_counts_pack(self._h, C.c_void_p(d_packed), n, stream))

    def counts_unpack(self, d_packed, n, stream=None):
        _ck(self._lib.hast_counts_unpack(self._h, C.c_void_p(d_packed), n, stream))

    def counts_add_votes(self, d_votes, d_barcode_ids, n_reads, max_votes, stream=None):
        _ck(self._lib.hast_counts_add_votes(self._h, C.c_void_p(d_votes), C.c_void_p(d_barcode_ids), n_reads, max_votes, stream))

    def set_option(self, name, value):
        _ck(self._lib.hast_ctx_set_option(self._h, name.encode(), int(value)))

    def options(self):
        buf = C.create_string_buffer(512)
        _ck(self._lib.hast_ctx_options(self._h, buf, len(buf)))
        return buf.value.decode()

    # classify
    def classify_device(self, d_bases, bases_bytes, n_reads, read_len, d_offsets=None, d_barcode_ids=None,
                        d_votes=None, stream=None):
        _ck(self._lib.hast_classify_device(self._h, C.c_void_p(d_bases), bases_bytes,
                                           C.c_void_p(d_offsets) if d_offsets else None, read_len,
                                           C.c_void_p(d_barcode_ids) if d_barcode_ids else None,
                                           C.c_void_p(d_votes) if d_votes else None, n_reads, stream))

    def classify_timing(self, n_slots):
        _ck(self._lib.hast_classify_timing(self._h, n_slots))

    def classify_times(self, max_n=4096):
        a, b, n = (C.c_float * max_n)(), (C.c_float * max_n)(), C.c_int()
        _ck(self._lib.hast_classify_times(self._h, a, b, max_n, C.byref(n)))
        return list(a[:n.value]), list(b[:n.value])

    def classify_batch(self, bases: np.ndarray, offsets: np.ndarray, ids: np.ndarray, max_read_len):
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        _ck(self._lib.hast_classify_batch(self._h, _ptr(bases), _ptr(offsets), _ptr(ids), ids.size, max_read_len))

    def classify_perread(self, bases: np.ndarray, offsets: np.ndarray) -> np.ndarray:
        """per-read (hits0, hits1), stage-03 string semantics, any read length"""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        votes = np.zeros((offsets.size - 1, 2), dtype=np.uint32)
        _ck(self._lib.hast_classify_perread(self._h, _ptr(bases), _ptr(offsets), offsets.size - 1, _ptr(votes)))
        return votes

    def classify_perread_device(self, d_bases, bases_bytes, d_offsets, n_reads, d_votes, stream=None):
        _ck(self._lib.hast_classify_perread_device(self._h, C.c_void_p(d_bases), bases_bytes, C.c_void_p(d_offsets),
                                                   n_reads, C.c_void_p(d_votes), stream))

    # synthetic
    def dz_compress_device(self, d_src, n_bytes, d_dst, cap, literals_only=False, stream=None) -> int:
        """one gzip member for the n_bytes at d_src, written to d_dst (room: cap >= dz_bound(n_bytes)); returns its size"""
        n = C.c_size_t()
        _ck(self._lib.hast_dz_compress_device_ex(self._h, C.c_void_p(d_src), n_bytes, C.c_void_p(d_dst), cap, C.byref(n), 1 if literals_only else 0, stream))
        return n.value

    def dz_compress_blocked_device(self, d_src, n_bytes, d_dst, cap, stream=None) -> int:
        """the n_bytes at d_src as blocked gzip (BGZF members of at most 49 152 bytes of input; 0 bytes: the end-of-file block),
        written to d_dst (room: cap >= dz_bound_blocked(n_bytes)); returns the size"""
        n = C.c_size_t()
        _ck(self._lib.hast_dz_compress_blocked_device(self._h, C.c_void_p(d_src), n_bytes, C.c_void_p(d_dst), cap, C.byref(n), stream))
        return n.value

    def synth_keys_device(self, p, hap, first, n, d_out, stream=None):
        _ck(self._lib.hast_synth_keys_device(self._h, C.byref(p), hap, first, n, C.c_void_p(d_out), stream))

    def synth_reads_device(self, p, first, n, d_bases, d_ids, stream=None):
        _ck(self._lib.hast_synth_reads_device(self._h, C.byref(p), first, n, C.c_void_p(d_bases),
                                              C.c_void_p(d_ids) if d_ids else None, stream))

    def synth_table_build(self, p):
        _ck(self._lib.hast_synth_table_build(self._h, C.byref(p)))


# ---- stage 00: parent-unique k-mer sets ---------------------------------------------------------------------
def dz_bound(n_bytes: int) -> int:
    """the most bytes Context.dz_compress_device can write for n_bytes of input"""
    return lib().hast_dz_bound(n_bytes)


def dz_bound_blocked(n_bytes: int) -> int:
    """the most bytes Context.dz_compress_blocked_device can write for n_bytes of input"""
    return lib().hast_dz_bound_blocked(n_bytes)


def kc_find_bounds(histo: np.ndarray):
    """(MIN_INDEX, MAX_INDEX, LOWER_INDEX, UPPER_INDEX) of find_bounds.awk; host arithmetic only"""
    histo = np.ascontiguousarray(histo, dtype=np.uint64)
    assert histo.size == KC_HISTO_HIGH + 2
    out = (C.c_long * 4)()
    lib().hast_kc_find_bounds(_ptr(histo), out)
    return tuple(out)


def kc_synth_host(p: KcSynth, parent, first, n_reads):
    out = np.empty(n_reads * (p.read_len + 1), dtype=np.uint8)
    _ck(lib().hast_kc_synth_host(C.byref(p), parent, first, n_reads, _ptr(out)))
    return out


class Rows:
    """hast_rows: the output table of `classify`, and with_lists the three barcode lists, made on the GPU from text records and counters
    in device memory (raw pointers: torch tensors' data_ptr(), Context.alloc)."""

    def __init__(self, ctx, d_text16, d_counts, n, n0, n1, w0=1.0, w1=1.0, with_lists=True):
        self._lib = lib()
        self._h = C.c_void_p()
        _ck(self._lib.hast_rows_build_device(ctx._h, C.c_void_p(d_text16), C.c_void_p(d_counts), n, n0, n1, w0, w1, int(with_lists), C.byref(self._h)))
        self.n = n

    def info(self) -> RowsInfo:
        r = RowsInfo()
        _ck(self._lib.hast_rows_get_info(self._h, C.byref(r)))
        return r

    def read(self, which, offset=0, n=None) -> bytes:
        if n is None:
            i = self.info()
            n = (i.list_bytes[which - 1] if which else i.table_bytes) - offset
        out = np.empty(max(n, 1), dtype=np.uint8)
        _ck(self._lib.hast_rows_read(self._h, which, offset, n, _ptr(out)))
        return out[:n].tobytes()

    def order(self) -> np.ndarray:
        out = np.empty(max(self.n, 1), dtype=np.uint32)
        _ck(self._lib.hast_rows_order(self._h, out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out[:self.n]

    def classes(self) -> np.ndarray:
        out = np.empty(max(self.n, 1), dtype=np.uint8)
        _ck(self._lib.hast_rows_classes(self._h, out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out[:self.n]

    def close(self):
        if self._h:
            self._lib.hast_rows_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class GzReader:
    """hast_gz: one .gz file inflated on the GPU (include/hast.h); read() returns the next bytes as a numpy array (test view:
    the product hands the bytes to the FASTQ framer on the device)."""

    def __init__(self, ctx, path, chunk_bytes=0, chunks_per_pass=0, room=0.0, ctxs=None):
        """ctxs: several contexts -> hast_gz_open_multi_ex (the passes of the one stream go to their GPUs in turn); reads land on ctx"""
        self._lib = lib()
        self._ctx = ctx
        h = C.c_void_p()
        if ctxs:
            arr = (C.c_void_p * len(ctxs))(*[c._h for c in ctxs])
            _ck(self._lib.hast_gz_open_multi_ex(arr, len(ctxs), os.fsencode(path), chunk_bytes, chunks_per_pass, room, C.byref(h)))
        else:
            _ck(self._lib.hast_gz_open_ex(ctx._h, os.fsencode(path), chunk_bytes, chunks_per_pass, room, C.byref(h)))
        self._h = h
        self._d = None
        self._cap = 0

    @classmethod
    def blocked(cls, ctx, path, batch_in=0, batch_out=0):
        """hast_gz_open_blocked_ex: a blocked-gzip (BGZF) file inflated per member; batch_in / batch_out: bytes a batch, 0 = default"""
        self = cls.__new__(cls)
        self._lib = lib()
        self._ctx = ctx
        self._d = None
        self._cap = 0
        self._h = None
        h = C.c_void_p()
        _ck(self._lib.hast_gz_open_blocked_ex(ctx._h, os.fsencode(path), batch_in, batch_out, C.byref(h)))
        self._h = h
        return self

    def blocked_stats(self):
        st = GzBlockedStats()
        _ck(self._lib.hast_gz_get_blocked_stats(self._h, C.byref(st)))
        return {n: getattr(st, n) for n, _ in GzBlockedStats._fields_}

    def read_device(self, d_dst, cap, stream=None):
        n = C.c_size_t()
        _ck(self._lib.hast_gz_read_device(self._h, C.c_void_p(d_dst), cap, C.byref(n), stream))
        return n.value

    def read(self, cap):
        if self._cap < cap:
            if self._d:
                self._ctx.free(self._d)
            self._d = self._ctx.alloc(cap + 16)
            self._cap = cap
        n = self.read_device(self._d, cap)
        self._ctx.sync()
        return self._ctx.to_host(self._d, (n,), np.uint8) if n else np.zeros(0, np.uint8)

    def read_all(self, piece=1 << 22):
        parts = []
        while True:
            a = self.read(piece)
            if a.size == 0:
                break
            parts.append(a)
        return np.concatenate(parts).tobytes() if parts else b""

    def units(self):
        return self._lib.hast_gz_units(self._h)

    def stats(self):
        st = GzStats()
        _ck(self._lib.hast_gz_get_stats(self._h, C.byref(st)))
        return {n: getattr(st, n) for n, _ in GzStats._fields_}

    def close(self):
        if self._h:
            self._lib.hast_gz_close(self._h)
            self._h = None
        if self._d:
            self._ctx.free(self._d)
            self._d = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class KmerCounter:
    """One count table of both parents' canonical k-mers in HBM (hast_kc_*)."""

    def __init__(self, k, table_bytes=0, device=0):
        self._lib = lib()
        h = C.c_void_p()
        _ck(self._lib.hast_kc_create(device, k, table_bytes, C.byref(h)))
        self._h = h
        self.k = k

    def close(self):
        if self._h:
            self._lib.hast_kc_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_slice(self, slice_, n_slices):
        _ck(self._lib.hast_kc_set_slice(self._h, slice_, n_slices))

    def count(self, parent, data: np.ndarray):
        data = np.ascontiguousarray(data, dtype=np.uint8)
        _ck(self._lib.hast_kc_count(self._h, parent, _ptr(data), data.size))

    def count_device(self, parent, d_bytes, n_bytes):
        _ck(self._lib.hast_kc_count_device(self._h, parent, C.c_void_p(d_bytes), n_bytes))

    def sync(self):
        _ck(self._lib.hast_kc_sync(self._h))

    def partition_info(self):
        out = np.zeros(5, dtype=np.uint64)
        _ck(self._lib.hast_kc_partition_info(self._h, out.ctypes.data_as(u64p)))
        return dict(partitioned=bool(out[0]), flushes=int(out[1]), records=int(out[2]), spilled_windows=int(out[3]), record_capacity=int(out[4]))

    def stats(self):
        out = np.zeros(6, dtype=np.uint64)
        _ck(self._lib.hast_kc_stats(self._h, out.ctypes.data_as(u64p)))
        return dict(distinct=(int(out[0]), int(out[1])), keys=int(out[2]), capacity=int(out[3]), total=(int(out[4]), int(out[5])))

    def histo(self, parent, into=None):
        h = np.zeros(KC_HISTO_HIGH + 2, dtype=np.uint64) if into is None else into
        _ck(self._lib.hast_kc_histo(self._h, parent, _ptr(h)))
        return h

    def select(self, parent, lower, upper):
        n = C.c_size_t()
        _ck(self._lib.hast_kc_select(self._h, parent, lower, upper, C.byref(n)))
        return n.value

    def selection_clear(self):
        _ck(self._lib.hast_kc_selection_clear(self._h))

    def release_table(self):
        _ck(self._lib.hast_kc_release_table(self._h))

    def selection_sort(self, parent):
        n = C.c_size_t()
        _ck(self._lib.hast_kc_selection_sort(self._h, parent, C.byref(n)))
        return n.value

    def selection_text(self, parent, first, count) -> bytes:
        out = np.empty(count * (self.k + 1), dtype=np.uint8)
        _ck(self._lib.hast_kc_selection_text(self._h, parent, first, count, _ptr(out)))
        return out.tobytes()

    def selection_keys(self, parent, first, count):
        out = np.empty(count, dtype=np.uint64)
        _ck(self._lib.hast_kc_selection_keys(self._h, parent, first, count, _ptr(out)))
        return out

    def synth_device(self, p: KcSynth, parent, first, n_reads, d_out):
        _ck(self._lib.hast_kc_synth_device(self._h, C.byref(p), parent, first, n_reads, C.c_void_p(d_out)))


class SqFramer:
    """Raw four-line FASTQ in HBM -> the counter's base stream in HBM (hast_sq_*), on the stream of a KmerCounter."""

    def __init__(self, kc: KmerCounter, max_in_bytes):
        self._lib = lib()
        h = C.c_void_p()
        _ck(self._lib.hast_sq_create(kc._h, max_in_bytes, C.byref(h)))
        self._h = h

    def frame_device(self, d_in, n_in, d_out, cap_out) -> SqResult:
        res = SqResult()
        _ck(self._lib.hast_sq_frame_device(self._h, C.c_void_p(d_in), n_in, C.c_void_p(d_out), cap_out, C.byref(res)))
        return res

    def frame_fasta_device(self, d_in, n_in, d_out, cap_out, in_flags=0) -> SqResult:
        """a view of raw FASTA (SQ_FA_OPEN: a header came in an earlier view; SQ_FA_LAST: the input ends with it); cap_out >= n_in + 1"""
        res = SqResult()
        _ck(self._lib.hast_sq_frame_fasta_device(self._h, C.c_void_p(d_in), n_in, C.c_void_p(d_out), cap_out, in_flags, C.byref(res)))
        return res

    def close(self):
        if self._h:
            self._lib.hast_sq_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class SqFeed:
    """One input stream of `unshared_kmers --ingest device` (hast_sq_feed_*): raw bytes in, counted in the KmerCounter's table."""

    def __init__(self, kc: KmerCounter, block_bytes, formats=SQ_TAKE_FASTQ):
        self._lib = lib()
        self._kc = kc
        self.block = block_bytes
        h = C.c_void_p()
        _ck(self._lib.hast_sq_feed_create(kc._h, block_bytes, C.byref(h)))
        self._h = h
        if formats != SQ_TAKE_FASTQ:
            self.set_formats(formats)

    def set_formats(self, mask):
        _ck(self._lib.hast_sq_feed_set_formats(self._h, mask))

    @property
    def format(self):
        return self._lib.hast_sq_feed_format(self._h)

    def submit(self, data: bytes, device=None):
        """up to block_bytes through the pinned staging block; device=<a Context on the table's device>: written into the feed's
        device block instead, once the table's stream has run dry (nothing reads the view any more), with a synchronous copy"""
        assert 0 < len(data) <= self.block
        p = C.c_void_p()
        if device is not None:
            _ck(self._lib.hast_sq_feed_device_block(self._h, C.byref(p)))
            self._kc.sync()
            _ck(self._lib.hast_memcpy_h2d(device._h, p, data, len(data)))
        else:
            _ck(self._lib.hast_sq_feed_host_block(self._h, C.byref(p)))
            C.memmove(p, data, len(data))
        _ck(self._lib.hast_sq_feed_submit(self._h, len(data)))

    def next(self, parent) -> SqResult:
        res = SqResult()
        _ck(self._lib.hast_sq_feed_next(self._h, parent, C.byref(res)))
        return res

    def finish(self, parent) -> SqResult:
        res = SqResult()
        _ck(self._lib.hast_sq_feed_finish(self._h, parent, C.byref(res)))
        return res

    def take_tail(self) -> bytes:
        buf = (C.c_uint8 * self.block)()
        n = C.c_size_t()
        _ck(self._lib.hast_sq_feed_take_tail(self._h, buf, C.byref(n)))
        return bytes(buf[:n.value])

    def close(self):
        if self._h:
            self._lib.hast_sq_feed_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class ReadStream:
    """The feed of `classify_read --ingest device` (hast_rs_*): raw FASTA / FASTQ bytes in, per-read names and votes out."""

    def __init__(self, ctx: Context, fmt, block_bytes):
        self._lib = lib()
        self._ctx = ctx
        self.block = block_bytes
        h = C.c_void_p()
        _ck(self._lib.hast_rs_create(ctx._h, fmt, block_bytes, C.byref(h)))
        self._h = h

    def submit(self, data: bytes, last=False, device=False):
        """one block of up to block_bytes; device=True: written into the feed's device block (the stream it names is the context's)"""
        p, stream = C.c_void_p(), C.c_void_p()
        if device:
            _ck(self._lib.hast_rs_device_block(self._h, C.byref(p), C.byref(stream)))
            assert stream.value == self._ctx.stream
            if data:
                _ck(self._lib.hast_memcpy_h2d(self._ctx._h, p, data, len(data)))      # (synchronous: the bytes lie there before the submit)
        else:
            _ck(self._lib.hast_rs_host_block(self._h, C.byref(p)))
            C.memmove(p, data, len(data))
        _ck(self._lib.hast_rs_submit(self._h, len(data), 1 if last else 0))

    def set_bins(self, mode, total0, total1):
        """the read bins (hast_rs_set_bins): 0 off, 1 plain, 2 gzip; total0 / total1: the two set sizes"""
        _ck(self._lib.hast_rs_set_bins(self._h, mode, total0, total1))

    def next_binned(self):
        """next(), and behind it the bins of the same view: (runs [3 x bytes], raw_bytes [3], count [3]); copies of the pinned buffers"""
        bins = RsBinned()
        out = self.next(bins)
        runs = [C.string_at(bins.run[c], bins.run_bytes[c]) if bins.run_bytes[c] else b"" for c in range(3)]
        return out + (runs, [int(x) for x in bins.raw_bytes], [int(x) for x in bins.count])

    def set_rows(self, mode, total0, total1):
        """the rows (hast_rs_set_rows): 0 off, 1 on; total0 / total1: the two set sizes, at least 1 each"""
        _ck(self._lib.hast_rs_set_rows(self._h, mode, total0, total1))

    def next_rows(self, binned=False):
        """next() or next_binned(), and behind it the rows of the same view: (text or None, count [3], on_host).  With the text there
        are no names and votes (names is None then); an on_host view has them and no text"""
        bins, rows = RsBinned(), RsRows()
        out = self.next(bins if binned else None, rows)
        if binned:
            runs = [C.string_at(bins.run[c], bins.run_bytes[c]) if bins.run_bytes[c] else b"" for c in range(3)]
            out = out + (runs, [int(x) for x in bins.raw_bytes], [int(x) for x in bins.count])
        text = None if rows.on_host else (C.string_at(rows.text, rows.bytes) if rows.bytes else b"")
        return out + (text, [int(x) for x in rows.count], bool(rows.on_host))

    def next(self, _bins=None, _rows=None):
        """(flags, consumed, bases, names, votes[records, 2]) of the oldest submitted block; copies of the feed's pinned buffers"""
        b = RsBlock()
        if _rows is not None:
            _ck(self._lib.hast_rs_next_rows(self._h, C.byref(b), None if _bins is None else C.byref(_bins), C.byref(_rows)))
            if b.records and not b.names and not b.votes and not b.name_off:
                return b.flags, b.consumed, b.bases, None, None
        elif _bins is None:
            _ck(self._lib.hast_rs_next(self._h, C.byref(b)))
        else:
            _ck(self._lib.hast_rs_next_binned(self._h, C.byref(b), C.byref(_bins)))
        n = b.records
        if not n:
            return b.flags, b.consumed, b.bases, [], np.zeros((0, 2), dtype=np.uint32)
        off = np.ctypeslib.as_array(b.name_off, (n + 1,))
        raw = C.string_at(b.names, b.name_bytes) if b.name_bytes else b""
        assert int(off[n]) == b.name_bytes
        names = [raw[int(off[i]):int(off[i + 1])] for i in range(n)]
        return b.flags, b.consumed, b.bases, names, np.ctypeslib.as_array(b.votes, (n, 2)).copy()

    def take_tail(self) -> bytes:
        buf = C.create_string_buffer(self.block)
        n = C.c_size_t()
        _ck(self._lib.hast_rs_take_tail(self._h, buf, C.byref(n)))
        return buf.raw[:n.value]

    def close(self):
        if self._h:
            self._lib.hast_rs_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def rs_rows_device(ctx, d_names, d_name_off, d_votes, n, total0, total1, d_out, cap):
    """hast_rs_rows_device over device pointers -> (bytes, count [3]); HastError(UNSUPPORTED).needed = the bytes a too small cap lacks"""
    nbytes, count = C.c_uint64(), (C.c_uint64 * 3)()
    st = lib().hast_rs_rows_device(ctx._h, _ptr(d_names), _ptr(d_name_off), _ptr(d_votes), n, total0, total1, _ptr(d_out), cap, C.byref(nbytes), C.byref(count))
    if st != 0:
        e = HastError(st, lib().hast_last_error().decode())
        e.needed = int(nbytes.value)
        raise e
    return int(nbytes.value), [int(x) for x in count]


# ---- stage 02: stLFR pairs -> 10x FASTQ ----------------------------------------------------------
class TxMap:
    """fake_10x.pl's map file as perl reads it (hast_tx_map_*); host only, no GPU"""

    def __init__(self, text: bytes):
        self._lib = lib()
        self._h = C.c_void_p()
        info = TxMapInfo()
        _ck(self._lib.hast_tx_map_parse(text, len(text), C.byref(self._h), C.byref(info)))
        self.n_keys, self.device_ok, self.reason = info.n_keys, bool(info.device_ok), info.reason.decode()

    def pair_host(self, r1: bytes, r2: bytes, final, state: TxState):
        """the host model over two buffers -> (out1, out2, TxResult); state is updated"""
        o1, o2, res = C.c_void_p(), C.c_void_p(), TxResult()
        _ck(self._lib.hast_tx_pair_host(self._h, r1, len(r1), r2, len(r2), int(final), C.byref(state), C.byref(o1), C.byref(o2), C.byref(res)))
        try:
            return C.string_at(o1, res.out_bytes[0]), C.string_at(o2, res.out_bytes[1]), res
        finally:
            self._lib.hast_tx_free(o1)
            self._lib.hast_tx_free(o2)

    def close(self):
        if self._h:
            self._lib.hast_tx_map_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class TxConverter:
    """The conversion over device memory (hast_tx_create / hast_tx_pair_device): the map as a table in HBM and the scratch of the worst
    step of max_in_bytes a side, on a Context's device and stream.  A map that is not device_ok raises HastError(UNSUPPORTED)."""

    def __init__(self, ctx: Context, tx_map: TxMap, max_in_bytes):
        self._lib = lib()
        self._h = C.c_void_p()
        _ck(self._lib.hast_tx_create(ctx._h, tx_map._h, max_in_bytes, C.byref(self._h)))

    def pair_device(self, d_r1, n1, d_r2, n2, state: TxState, d_out1, cap1, d_out2, cap2, stream=None) -> TxResult:
        """TxMap.pair_host(..., False, state) over d_r1[0, n1) / d_r2[0, n2) into d_out1 / d_out2; state is updated.  An output larger
        than its room raises HastError(UNSUPPORTED) whose .result holds the sizes needed; state is then unchanged."""
        res = TxResult()
        st = self._lib.hast_tx_pair_device(self._h, C.c_void_p(d_r1), n1, C.c_void_p(d_r2), n2, C.byref(state), C.c_void_p(d_out1), cap1, C.c_void_p(d_out2), cap2,
                                           C.byref(res), stream)
        if st != 0:
            err = HastError(st, self._lib.hast_last_error().decode())
            err.result = res
            raise err
        return res

    def pair_staged(self, r1: bytes, r2: bytes, state: TxState, gz, times: TxTimes = None):
        """a step from host bytes to host bytes (hast_tx_pair_staged) -> (out1, out2, TxResult); gz: each run as one gzip member"""
        o1, o2, res = C.c_void_p(), C.c_void_p(), TxResult()
        times = TxTimes() if times is None else times
        _ck(self._lib.hast_tx_pair_staged(self._h, r1, len(r1), r2, len(r2), C.byref(state), int(gz), C.byref(o1), C.byref(o2), C.byref(res), C.byref(times)))
        return C.string_at(o1, res.out_bytes[0]), C.string_at(o2, res.out_bytes[1]), res

    def close(self):
        if self._h:
            self._lib.hast_tx_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


TX_ON_HOST, TX_TAIL_TOO_LONG, TX_ENDS = 1, 4, 8


class TxFeed:
    """The paired, pipelined device route of one fake_10x run over a TxConverter (hast_tx_feed_*): per side, bytes are written in HBM
    (device_block: the address and the stream to fill it on) or handed over from the host (submit_host), step() converts the whole
    pairs and enqueues the runs' deflate (gz_out) on a second stream, collect() returns the oldest step's outputs.  At most two steps
    wait for collect()."""

    def __init__(self, conv: TxConverter, block_bytes, gz_out):
        self._lib = lib()
        self._h = C.c_void_p()
        self.block = block_bytes
        _ck(self._lib.hast_tx_feed_create(conv._h, block_bytes, int(bool(gz_out)), C.byref(self._h)))
        self.room = self._lib.hast_tx_feed_room(self._h)

    def wants(self, side) -> bool:
        return bool(self._lib.hast_tx_feed_wants(self._h, side))

    def device_block(self, side):
        """-> (device address of the side's next block, the stream its bytes must be written on)"""
        d, stream = C.c_void_p(), C.c_void_p()
        _ck(self._lib.hast_tx_feed_device_block(self._h, side, C.byref(d), C.byref(stream)))
        return d.value, stream

    def submit(self, side, n_bytes):
        _ck(self._lib.hast_tx_feed_submit(self._h, side, n_bytes))

    def submit_host(self, side, data: bytes):
        """the side's next block from host bytes (at most block_bytes; fewer: the side's end)"""
        h = C.c_void_p()
        _ck(self._lib.hast_tx_feed_host_block(self._h, side, C.byref(h)))
        C.memmove(h, data, len(data))
        self.submit(side, len(data))

    def step(self, state: TxState):
        """-> (TxResult, flags: TX_ON_HOST | TX_TAIL_TOO_LONG | TX_ENDS); state is updated"""
        res, flags = TxResult(), C.c_int(0)
        _ck(self._lib.hast_tx_feed_step(self._h, C.byref(state), C.byref(res), C.byref(flags)))
        return res, flags.value

    def collect(self):
        """the oldest step not yet collected -> (out1, out2, raw_bytes): copies of what the feed's pinned slots hold"""
        o1, o2, n_out, n_raw = C.c_void_p(), C.c_void_p(), (C.c_uint64 * 2)(), (C.c_uint64 * 2)()
        _ck(self._lib.hast_tx_feed_collect(self._h, C.byref(o1), C.byref(o2), C.byref(n_out), C.byref(n_raw)))
        return C.string_at(o1, n_out[0]) if n_out[0] else b"", C.string_at(o2, n_out[1]) if n_out[1] else b"", (n_raw[0], n_raw[1])

    def take_tail(self, side) -> bytes:
        buf, n = C.create_string_buffer(max(self.room, 1)), C.c_size_t(0)
        _ck(self._lib.hast_tx_feed_take_tail(self._h, side, buf, C.byref(n)))
        return buf.raw[:n.value]

    def times(self):
        """-> (TxTimes, seconds spent waiting in collect)"""
        t, w = TxTimes(), C.c_double(0)
        _ck(self._lib.hast_tx_feed_times(self._h, C.byref(t), C.byref(w)))
        return t, w.value

    def close(self):
        if self._h:
            self._lib.hast_tx_feed_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class Tally:
    """A device dictionary of exactly max_texts ids with a 64-bit counter per id (hast_tally_*): what a FASTQ stream in tally mode
    (hast_fq_set_tally / hast_fq_next_tallied) counts the keys of its header lines into."""

    def __init__(self, ctx: Context, max_texts):
        self._h = C.c_void_p()
        _ck(lib().hast_tally_create(ctx._h, max_texts, C.byref(self._h)))

    def limit(self) -> int:
        return lib().hast_tally_limit(self._h)

    def size(self) -> int:
        n = C.c_size_t()
        _ck(lib().hast_tally_size(self._h, C.byref(n)))
        return n.value

    def read(self):
        """{key: count} of every id handed out"""
        n = self.size()
        text = np.zeros((max(n, 1), 16), np.uint8)
        counts = np.zeros(max(n, 1), np.uint64)
        _ck(lib().hast_tally_read(self._h, 0, n, text.ctypes.data_as(C.POINTER(C.c_uint8)), counts.ctypes.data_as(u64p)))
        return {bytes(text[i, 1:1 + text[i, 0]]): int(counts[i]) for i in range(n)}

    def close(self):
        if self._h:
            lib().hast_tally_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
