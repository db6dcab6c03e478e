#!/usr/bin/env python3
"""Windows per read that k_classify_f sends to the exact table (phase V), counted on the device (HAST_COUNT_LOOKUPS=1,
hast_filter_lookups), on the bench's own tables and reads: C3's 200M + 200M keys, random and clustered, one launch of R reads.
    python3 tools/gpu/lookups_per_read.py [reads per launch, default 12000000]
Prints one JSON line per kind of keys; the simulation's figures for the same tables are in profiles/exact_load_sim_pos.txt."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
os.environ["HAST_COUNT_LOOKUPS"] = "1"

import numpy as np  # noqa: E402

import bench  # noqa: E402
import hast_amd  # noqa: E402
from hast_amd.binding import make_params  # noqa: E402

K, L, N_KEYS, N_BC = 21, 150, 200_000_000, 10_000_000
R = int(sys.argv[1]) if len(sys.argv) > 1 else 12_000_000
for clustered in (False, True):
    p = make_params(K, L, N_KEYS, N_BC, clustered=clustered)
    with hast_amd.Context(K, 0) as ctx:
        ctx.table_reserve(2 * N_KEYS, 0.2)
        ctx.synth_table_build(p)
        akeys = []
        for ad in (bench.ADAPTOR_F, bench.ADAPTOR_R):
            for kmer in hast_amd.chop_read(ad, K):
                if kmer not in akeys:
                    akeys.append(kmer)
        ctx.table_erase(np.array(akeys, dtype=np.uint64))
        ctx.filter_build()
        ctx.counts_resize(N_BC)
        d_bases, d_ids = ctx.alloc(R * L + 64), ctx.alloc(R * 4)
        ctx.synth_reads_device(p, 0, R, d_bases, d_ids)
        ctx.classify_device(d_bases, R * L, R, L, d_barcode_ids=d_ids)
        ctx.sync()
        n = ctx.filter_lookups()
        c0, c1, neg = ctx.counts_read(N_BC)
        print(json.dumps({"keys": "clustered" if clustered else "random", "reads": R, "dense": ctx.filter_dense(), "lookups": n, "lookups_per_read": n / R,
                          "hits": {"c0": int(c0.sum(dtype=np.uint64)), "c1": int(c1.sum(dtype=np.uint64))}}), flush=True)
