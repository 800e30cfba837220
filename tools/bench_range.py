#!/usr/bin/env python3
"""Exact Flat range search against the k-NN call it competes with, same process, same queries, legs alternating.

  range leg: vdb_flat_range_device, r_q = the query's K-th exact distance (K = 64 by default)
  k-NN leg : vdb_flat_knn_device at k = K (unchanged by the range search: the parent's number measured in the same run)

Device events around calls that end synchronised; WARMUP + STEPS steps of NQ queries on the default bench data (1M x 960 gist-like
rows, seeds 1806 / 1807).  Writes one JSON record (default profiles/flat_range_1M.json) with the two step times, the tier's share
and the hit / result statistics per query.  The per-kernel table kept beside the record comes from a separate run of the same loop,
`rocprofv3 --kernel-trace --stats -d DIR -o range -- python tools/bench_range.py --steps 3 --warmup 1 --out ''`, summarised by
`python tools/kstats.py DIR`."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=960)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--k", type=int, default=64, help="the radius is the query's k-th exact distance; the k-NN leg runs at this k")
    ap.add_argument("--scale", type=float, default=1.0, help="radius = scale x that distance")
    ap.add_argument("--dist", choices=["l2sqr", "cosine"], default="l2sqr")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--mode", type=int, default=0, help="flat mode of the range leg: 0 auto, 1 scan only, 2 tier forced")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "flat_range_1M.json"), help="'' = print only")
    args = ap.parse_args()

    import numpy as np
    import torch

    import lab_1806_vec_db_amd as vdb
    from bench import gist_like_gpu
    from lab_1806_vec_db_amd import _lib as L

    dev = torch.device("cuda", 0)
    n, dim, nq, k = args.rows, args.dim, args.nq, args.k
    base = gist_like_gpu(torch, n, dim, 1806, dev)
    qs = gist_like_gpu(torch, nq, dim, 1807, dev)
    ix = vdb.GpuIndex(dim, args.dist)
    ix.add_device(base.data_ptr(), n)
    del base
    oi = torch.zeros(nq, k, dtype=torch.int64, device=dev)
    od = torch.zeros(nq, k, device=dev)
    oc = torch.zeros(nq, dtype=torch.int64, device=dev)
    ix.flat_knn_device(qs.data_ptr(), nq, k, oi.data_ptr(), od.data_ptr(), oc.data_ptr())
    torch.cuda.synchronize()
    radius = (od[:, k - 1] * args.scale).contiguous()
    lib, h = ix._lib, ix._h
    stats = ("flat_range_queries", "flat_range_i8_queries", "flat_range_scan_queries", "flat_range_hits", "flat_range_results")

    def range_step():
        res = L.vp()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ix.set_flat_mode(args.mode)
        a.record()
        L.check(lib.vdb_flat_range_device(h, L.vp(qs.data_ptr()), nq, dim, L.vp(radius.data_ptr()), 0, L.vp(0), C.byref(res)))
        b.record()
        b.synchronize()
        ix.set_flat_mode(0)
        lims = np.zeros(nq + 1, dtype=np.uint64)
        L.check(lib.vdb_range_lims(res, lims.ctypes.data_as(L.u64p)))
        L.check(lib.vdb_range_destroy(res))
        return a.elapsed_time(b), np.diff(lims.astype(np.int64))

    def knn_step():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ix.flat_knn_device(qs.data_ptr(), nq, k, oi.data_ptr(), od.data_ptr(), oc.data_ptr())
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    for _ in range(args.warmup):
        range_step()
        knn_step()
    s0 = {s: ix.get_stat(s) for s in stats}
    t_range, t_knn, per_q = [], [], None
    for _ in range(args.steps):
        ms, per_q = range_step()
        t_range.append(ms)
        t_knn.append(knn_step())
    d = {s: ix.get_stat(s) - s0[s] for s in stats}
    tq = max(1, d["flat_range_i8_queries"])
    rec = {
        "what": "exact Flat range search vs vdb_flat_knn_device at the same k, same process, alternating legs, device events",
        "rows": n, "dim": dim, "nq": nq, "dist": args.dist, "k": k, "radius": f"{args.scale} x the query's {k}-th exact distance",
        "steps": args.steps, "warmup": args.warmup, "range_mode": args.mode,
        "range_step_ms_median": float(np.median(t_range)), "range_step_ms_min": float(np.min(t_range)), "range_step_ms_max": float(np.max(t_range)),
        "knn_step_ms_median": float(np.median(t_knn)), "knn_step_ms_min": float(np.min(t_knn)), "knn_step_ms_max": float(np.max(t_knn)),
        "range_over_knn": float(np.median(t_range) / np.median(t_knn)),
        "tier_share": d["flat_range_i8_queries"] / max(1, d["flat_range_queries"]),
        "hits_per_tier_query_mean": d["flat_range_hits"] / tq, "hits_per_tier_query_max": ix.get_stat("flat_range_hits_max"),
        "results_per_query_mean": float(per_q.mean()), "results_per_query_max": int(per_q.max()), "results_per_query_min": int(per_q.min()),
        "hits_over_results": d["flat_range_hits"] / max(1, d["flat_range_results"]),
    }
    print(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
