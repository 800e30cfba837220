#!/usr/bin/env python3
"""Exact Flat range search against the k-NN call it competes with, same process, same queries, legs alternating.

  range leg: vdb_flat_range_device, r_q = the query's K-th exact distance (K = 64 by default)
  k-NN leg : vdb_flat_knn_device at k = K (unchanged by the range search: the parent's number measured in the same run)

Device events around calls that end synchronised; WARMUP + STEPS steps of NQ queries on the default bench data (1M x 960 gist-like
rows, seeds 1806 / 1807).  Writes one JSON record (default profiles/flat_range_1M.json) with the two step times, the tier's share
and the hit / result statistics per query.  The per-kernel table kept beside the record comes from a separate run of the same loop,
`rocprofv3 --kernel-trace --stats -d DIR -o range -- python tools/bench_range.py --steps 3 --warmup 1 --out ''`, summarised by
`python tools/kstats.py DIR`.

  --shards S[,S...]: the row-sharded range search's pieces on ONE GPU (a shard-size run, not a multi-GPU measurement: there is no
  second GPU, so no collective is timed).  The corpus is held a second time as S indexes of N/S rows with id offsets; per step, legs
  alternating: the unsharded range step, every shard's range step in turn, then -- on the shards' results packed the way phase 2 of the
  exchange delivers them ([S][largest shard total] ids / distances, [S][nq + 1] offsets, on the device) -- vdb_range_merge_device (device
  events around the call that ends synchronised, and the kernel alone from the library's own events) and the host utility
  vdb_range_merge on the same lists.  Writes profiles/flat_range_shards.json."""
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
    ap.add_argument("--shards", type=str, default="", help="e.g. 8,4: measure the sharded range search's pieces at these shard counts instead")
    ap.add_argument("--out", type=str, default=None, help="'' = print only (default: profiles/flat_range_1M.json, with --shards profiles/flat_range_shards.json)")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "flat_range_shards.json" if args.shards else "flat_range_1M.json")

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
    if not args.shards:
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

    if args.shards:
        runs = [shard_run(args, torch, np, vdb, L, ix, base, qs, radius, range_step, int(x)) for x in args.shards.split(",")]
        rec = {"what": "pieces of the row-sharded range search on ONE GPU (shard-size run, no collective timed): device merge vs one shard's "
                       "range step vs the host merge vs the unsharded step; same process, alternating legs, device events",
               "rows": n, "dim": dim, "nq": nq, "dist": args.dist, "radius": f"{args.scale} x the query's {k}-th exact distance",
               "steps": args.steps, "warmup": args.warmup, "range_mode": args.mode, "runs": runs}
        print(json.dumps(rec))
        if args.out:
            with open(args.out, "w") as f:
                json.dump(rec, f, indent=1)
                f.write("\n")
        return
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


def shard_run(args, torch, np, vdb, L, ix, base, qs, radius, unsharded_step, S):
    """one shard count: medians over the steps of (a) the device merge, (b) one shard's range step, (c) the host merge, (d) the unsharded step"""
    import time

    from lab_1806_vec_db_amd.shard import shard_bounds

    n, dim, nq = args.rows, args.dim, args.nq
    lib = ix._lib
    shards = []
    for r in range(S):
        r0, r1 = shard_bounds(n, S, r)
        sx = vdb.GpuIndex(dim, args.dist)
        sx.add_device(base[r0:r1].data_ptr(), r1 - r0)
        sx.set_id_offset(r0)
        sx.set_flat_mode(args.mode)
        shards.append(sx)
    merger = vdb.GpuIndex(dim, args.dist)  # (the merge needs an index for its device and its events; this one holds no rows)
    merger.prof_enable(True)

    def shard_step(sx):
        res = L.vp()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        L.check(lib.vdb_flat_range_device(sx._h, L.vp(qs.data_ptr()), nq, dim, L.vp(radius.data_ptr()), 0, L.vp(0), C.byref(res)))
        b.record()
        b.synchronize()
        return a.elapsed_time(b), sx._range_out(res, nq)

    t_merge, t_kernel, t_host, t_shard0, t_shards_sum, t_unsharded = [], [], [], [], [], []
    in_pairs = out_pairs = 0
    for step in range(args.warmup + args.steps):
        ms_u, _ = unsharded_step()
        parts = [shard_step(sx) for sx in shards]
        res = [p[1] for p in parts]
        stride = max(max(int(r[0][nq]) for r in res), 1)
        lims = np.stack([r[0] for r in res])
        ids = np.zeros((S, stride), dtype=np.uint64)
        ds = np.zeros((S, stride), dtype=np.float32)
        for s_, (l, i, d) in enumerate(res):
            ids[s_, :len(i)] = i
            ds[s_, :len(d)] = d
        d_lims = torch.from_numpy(lims.view(np.int64)).cuda()
        d_ids = torch.from_numpy(ids.view(np.int64)).cuda()
        d_ds = torch.from_numpy(ds).cuda()
        torch.cuda.synchronize()
        merger.prof_reset()
        out = L.vp()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        L.check(lib.vdb_range_merge_device(merger._h, L.vp(d_lims.data_ptr()), L.vp(d_ids.data_ptr()), L.vp(d_ds.data_ptr()), S, nq, stride, 0, L.vp(0),
                                           C.byref(out)))
        b.record()
        b.synchronize()
        dl, di, dd = merger._range_out(out, nq)
        ol = np.zeros(nq + 1, dtype=np.uint64)
        oi = np.zeros(int(dl[nq]), dtype=np.uint64)
        od = np.zeros(int(dl[nq]), dtype=np.float32)
        t0 = time.perf_counter()
        L.check(lib.vdb_range_merge(lims.ctypes.data_as(L.u64p), ids.ctypes.data_as(L.u64p), ds.ctypes.data_as(L.f32p), S, nq, stride, 0,
                                    ol.ctypes.data_as(L.u64p), oi.ctypes.data_as(L.u64p), od.ctypes.data_as(L.f32p)))
        t1 = time.perf_counter()
        assert np.array_equal(ol, dl) and np.array_equal(oi, di) and np.array_equal(od.view(np.uint32), dd.view(np.uint32))
        if step < args.warmup:
            continue
        t_unsharded.append(ms_u)
        t_shard0.append(parts[0][0])
        t_shards_sum.append(sum(p[0] for p in parts))
        t_merge.append(a.elapsed_time(b))
        t_kernel.append(merger.prof_get("range_merge")["ms"])
        t_host.append((t1 - t0) * 1e3)
        in_pairs, out_pairs = int(lims[:, nq].sum()), int(dl[nq])
    tier = sum(sx.get_stat("flat_range_i8_queries") for sx in shards) / max(1, sum(sx.get_stat("flat_range_queries") for sx in shards))
    for sx in shards:
        sx.close()
    merger.close()
    med = lambda v: float(np.median(v))  # noqa: E731
    return {"shards": S, "rows_per_shard": -(-n // S),
            "a_merge_device_call_ms_median": med(t_merge), "a_merge_device_call_ms_min": float(np.min(t_merge)),
            "a_merge_kernel_ms_median": med(t_kernel),
            "b_one_shard_range_step_ms_median": med(t_shard0), "b_all_shards_in_turn_ms_median": med(t_shards_sum),
            "c_merge_host_ms_median": med(t_host), "c_merge_host_ms_min": float(np.min(t_host)),
            "d_unsharded_range_step_ms_median": med(t_unsharded),
            "a_over_b": med(t_merge) / med(t_shard0), "a_over_c": med(t_merge) / med(t_host),
            "pairs_in": in_pairs, "pairs_out": out_pairs, "phase2_bytes_per_rank": stride * 12, "shard_tier_share": tier}


if __name__ == "__main__":
    main()
