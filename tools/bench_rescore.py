#!/usr/bin/env python3
"""Exact rescoring of candidate documents (vdb_flat_rescore_groups_device) against the first stage alone, same process, same table.

1M x 960 f32 rows (bench data, seed 1806) with a label column of 8 rows per document; 100 questions of 32 sub-queries (a base vector plus
small perturbations).  The first stage, vdb_flat_knn_fused_groups_device (SUM) at k = fetch_k = 64, yields 64 candidate documents per
question; the second stage rescores them over all their chunks (64 x 8 rows x 32 sub-queries per question) and returns k = 10.  Host clock
around calls that end synchronised, median of --reps with the range; the three timers of the call come from one more run with the profile
on.  No threshold is set on any of these times.  Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COLUMN, PER_DOC = 0, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=960)
    ap.add_argument("--questions", type=int, default=100)
    ap.add_argument("--lists", type=int, default=32)
    ap.add_argument("--candidates", type=int, default=64)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()

    import numpy as np
    import torch

    import lab_1806_vec_db_amd as vdb
    from bench import gist_like_gpu

    dev = torch.device("cuda", 0)
    n, dim, nq, S, ld, k = args.rows, args.dim, args.questions, args.lists, args.candidates, args.k
    ix = vdb.GpuIndex(dim, "l2sqr")
    base = gist_like_gpu(torch, n, dim, 1806, dev)
    ix.add_device(base.data_ptr(), n)
    del base
    ix.set_labels(COLUMN, (np.arange(n) // PER_DOC).astype(np.uint32))
    seeds = gist_like_gpu(torch, nq, dim, 1807, dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1900 + S)
    tq = (seeds[:, None, :] + torch.randn((nq, S, dim), generator=gen, device=dev, dtype=torch.float32) * 0.02).clamp_(0, 0.8)
    tq = tq.reshape(nq * S, dim).contiguous()
    lims = np.arange(0, nq * S + 1, S, dtype=np.uint64)
    c_i = torch.zeros((nq, ld), dtype=torch.int64, device=dev)
    c_d = torch.zeros((nq, ld), dtype=torch.float32, device=dev)
    c_c = torch.zeros((nq,), dtype=torch.int64, device=dev)
    o_i = torch.zeros((nq, k), dtype=torch.int64, device=dev)
    o_d = torch.zeros((nq, k), dtype=torch.float32, device=dev)
    o_c = torch.zeros((nq,), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    def first():
        ix.flat_knn_fused_groups_device(tq.data_ptr(), lims, ld, ld, COLUMN, c_i.data_ptr(), c_d.data_ptr(), c_c.data_ptr(), mode="sum")

    def second():
        ix.rescore_groups_device(tq.data_ptr(), lims, c_i.data_ptr(), c_c.data_ptr(), ld, k, COLUMN, o_i.data_ptr(), o_d.data_ptr(), o_c.data_ptr(), mode="sum")

    def wall(fn):
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return {"ms_median": float(np.median(ts)), "ms_min": float(np.min(ts)), "ms_max": float(np.max(ts)), "reps": args.reps}

    first()
    second()  # (warm: buffers, the LDS opt-in)
    rows0 = ix.get_stat("flat_rescore_rows")
    rec = {"what": "vdb_flat_rescore_groups_device (SUM) over the candidates of vdb_flat_knn_fused_groups_device, per %d questions" % nq,
           "rows": n, "dim": dim, "rows_per_document": PER_DOC, "questions": nq, "sub_queries": S, "candidates": ld, "k": k,
           "fused_groups_alone": wall(first), "rescore": wall(second)}
    rec["candidate_rows_per_question"] = (ix.get_stat("flat_rescore_rows") - rows0) / (args.reps * nq)
    ix.prof_enable(True)
    ix.prof_reset()
    second()
    rec["timers_ms"] = {name: ix.prof_get(name)["ms"] for name in ("rescore_collect", "rescore_pairs", "rescore_finish")}
    ix.prof_enable(False)
    rec["rescore_over_fused_groups"] = rec["rescore"]["ms_median"] / rec["fused_groups_alone"]["ms_median"]
    print(json.dumps(rec))
    ix.close()


if __name__ == "__main__":
    main()
