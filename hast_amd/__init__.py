"""hast_amd -- Python-side handle on the MI355X-native HAST stage-01 classifier.

The product is native: `libhast.so` (HIP kernels for gfx950 + C ABI, include/hast.h) and the drop-in
`classify` executable, both built in-tree by hast_amd/csrc/Makefile.  This package is only the
ctypes view of that C ABI used by bench.py and the tests; there is no Python or CPU compute path --
every call needs the shared library, and every compute call needs a GPU.
"""
from .binding import (HastError, Context, SynthParams, lib, lib_path, classify_exe, classify_read_exe, build,  # noqa: F401
                      parse_barcode, get_hap, canon_kmer, chop_read, synth_keys_host, synth_reads_host,
                      ABI_SYMBOLS, B_ALG_PER_READ, KmerCounter, SqFramer, SqFeed, SqResult, SQ_NOT_FOUR_LINE, SQ_NO_RECORD, SQ_TAIL_TOO_LONG, SQ_FA_OPEN, SQ_FA_LAST, SQ_TAKE_FASTQ, SQ_TAKE_FASTA, KcSynth, KC_HISTO_HIGH, kc_find_bounds, kc_synth_host,
                      unshared_kmers_exe, GzReader, GzStats, GzBlockedStats, dz_bound, dz_bound_blocked,
                      fake_10x_exe, TxMap, TxState, TxResult, TxMapInfo, TxConverter, TxTimes, TxFeed, TX_ON_HOST, TX_TAIL_TOO_LONG, TX_ENDS,
                      barcode_freq_exe, Tally, FqTallied, Rows, RowsInfo,
                      ReadStream, RsBlock, RsRows, rs_rows_device, RS_FASTA, RS_FASTQ, RS_FORMAT_ERROR, RS_RECORD_TOO_LONG)
