#!/usr/bin/env python3
"""Measurement: the pairwise strain evidence (pantax_hip_strain_pair_evidence) on a bench workload, beside the db-only pair sums
(pantax_hip_db_hap_pairs) on the same selection in the same process -- the yardstick.  Builds the set as bench.py does, uploads db and reads, runs one
coverage pass as a stage call, selects every haplotype of every species and times both node passes through timing_get and by wall time: ms per kernel
variant (by the columns a wave keeps), the ratio of the two calls, algorithmic bytes.  With route "walk" the membership comes from the selected walks
(hap_pairs_route=walk): the mask pass is timed too.
usage: pair_evidence_probe.py [workload (cfg4)] [repeats (3)] [route (node | walk)] [record.json]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import bench
from pantax_amd.engine import Engine

name = sys.argv[1] if len(sys.argv) > 1 else "cfg4"
N = int(sys.argv[2]) if len(sys.argv) > 2 else 3
route = sys.argv[3] if len(sys.argv) > 3 else "node"
record = sys.argv[4] if len(sys.argv) > 4 else None
spec = bench.workload_spec(name)
t0 = time.perf_counter()
ns = bench.native_set(spec, threads=min(16, os.cpu_count() or 1))
rd = ns.reads()
species = ns.graphs()
print("%s: %d species, %d reads, generated in %.1f s" % (name, len(species), rd.n_reads, time.perf_counter() - t0), flush=True)
eng = Engine(0)
eng.upload_db(species)
eng.upload_packed(rd)
eng.rcls_profile(want_species=False)
eng.trio_nodes_info(fetch=False)
eng.get_node_abundances(fetch=False)                              # the coverage result of the stage kind
K = np.array([g.n_paths for g in species], dtype=np.int64)
sel = (np.concatenate([[0], np.cumsum(K)]).astype(np.uint64), np.concatenate([np.arange(k, dtype=np.uint32) for k in K]))
V = int(eng.node_off[-1])
nw = (K + 63) // 64
by_node = route != "walk"
words = np.where((K <= 64) & by_node, 1, nw)                      # mask words per node: the node -> haplotype word of route 1, the compact masks of route 2
tiles = words * (words + 1) // 2                                  # block pairs of every species
nodes = np.array([g.n_nodes for g in species], dtype=np.int64)
m_words = np.where(words > 1, 8 * words, 0)                       # every word once more for m(v) where a species has several
# db-only: one node read per block pair, 4 (length) + 8 a word, two words off the diagonal
b_db = int((nodes * (words * 12 + (tiles - words) * 20 + m_words)).sum())
# coverage form: three planes per block pair, the quantity 4 / 4 / 8 bytes + the words each time; the species sums read 4 + 4 + 8 once more
b_pe = int((nodes * (words * (12 + 12 + 16) + (tiles - words) * (20 + 20 + 24) + m_words + 16)).sum())
print("selected: %d haplotypes over %d species (K %d .. %d), %d nodes, %d pair entries" % (int(K.sum()), eng.S, K.min(), K.max(), V, int((K * K).sum())), flush=True)
if route == "walk":
    eng.set_option("hap_pairs_route", "walk")


def timed(call, prefix):
    out = call(sel[0], sel[1])                                    # warm-up
    eng.timing_enable(True)
    eng.timing_reset()
    walls = []
    for _ in range(N):
        t0 = time.perf_counter()
        out = call(sel[0], sel[1])
        walls.append((time.perf_counter() - t0) * 1e3)
    rows = eng.timing_get()
    eng.timing_enable(False)
    per = lambda k: rows.get(k, (0, 0.0))[1] / max(N, 1)
    variants = {k: per(k) for k in sorted(rows) if k.startswith(prefix)}
    return out, walls, variants, per("read_strain_mask_kernel")


db_out, db_wall, db_var, db_mask = timed(eng.hap_pairs, "hap_pairs_kernel")
pe_out, pe_wall, pe_var, pe_mask = timed(eng.pair_evidence, "pair_evidence_kernel")
eng.set_option("hap_pairs_route", None)
assert np.array_equal(pe_out[0], db_out[0]) and np.array_equal(pe_out[1][:, :2], db_out[1]) and np.array_equal(pe_out[2][:, :, :2], db_out[2])
ms_db, ms_pe = sum(db_var.values()), sum(pe_var.values())
res = {"workload": name, "route": route, "repeats": N, "haplotypes": int(K.sum()), "species": eng.S, "nodes": V, "pair_entries": int((K * K).sum()),
       "db_hap_pairs": {"call_ms_wall": db_wall, "kernel_ms": ms_db, "kernel_ms_by_columns": db_var, "kernel_gb": b_db / 1e9,
                        "of_8TBs": b_db / ms_db / 1e6 / 8000 if ms_db else None, "read_strain_mask_kernel_ms": db_mask if route == "walk" else None},
       "strain_pair_evidence": {"call_ms_wall": pe_wall, "kernel_ms": ms_pe, "kernel_ms_by_columns": pe_var, "kernel_gb": b_pe / 1e9,
                                "of_8TBs": b_pe / ms_pe / 1e6 / 8000 if ms_pe else None, "read_strain_mask_kernel_ms": pe_mask if route == "walk" else None},
       "kernel_ms_ratio": ms_pe / ms_db if ms_db else None, "call_wall_ratio_of_medians": float(np.median(pe_wall) / np.median(db_wall)),
       "columns_0_2_equal_db_hap_pairs": True,
       "covered_sum_over_entries": int(pe_out[1][:, 2].sum()), "bases_total": int(pe_out[2][:, 0, 3].sum())}
print(json.dumps(res), flush=True)
if record:
    with open(record, "w") as f:
        json.dump(res, f, indent=1)
eng.close()
