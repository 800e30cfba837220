#!/usr/bin/env python3
"""One label column grouped by code in a single pass (vdb_mask_create_partition, vdb_index_label_counts) against what the table did
before, same process, same table.

1M x 960 f32 rows (bench data, seed 1806) in a VecDB table as tools/bench_mask_build.py makes it: metadata per row an id, `tenant` (1000
tenants x 1000 rows, row i belongs to tenant i % 1000 -- the 64 rows of a wave carry 64 different tenants, the longest loop
k_mask_partition has) and a two-valued `tier`.  Host clock around calls that end synchronised, median of --reps (40):
  masks         GpuIndex.make_masks_partition against GpuIndex.make_masks_where for the SAME G codes, G in --groups: wall time of the
                call with its masks closed again, and the kernels' own time (vdb_prof_get "mask_partition" / "mask_where", from
                separate profiled calls).  partition_min = the smallest G of the sweep at which the partition call's median wall time
                was below make_masks_where's: the value vecdb.PARTITION_MIN ships with (None when there is none).
  batch_search  VecDB.batch_search, one query per tenant, k = 10, all 1000 tenants, the masks dropped by a batch_add just before, with the
                routing through the partition on (PARTITION_MIN = 1) and off (None); and warm.
  count_by      VecDB.count_by("tenant") against the host loop collections.Counter(m.get("tenant") for matching rows), without a filter
                and under {"tier": "gold"} (the host loop with --host-reps repetitions: each is a pass over 1M dicts).
Every partition mask is compared with the make_masks_where mask of the same code (words and ids), every count with the host loop's,
before anything is timed.  Writes one JSON record (default profiles/mask_partition_1M.json)."""
from __future__ import annotations

import argparse
import collections
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=960)
    ap.add_argument("--tenants", type=int, default=1000)
    ap.add_argument("--groups", type=str, default="1,2,4,8,16,32,64,256,1000")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "mask_partition_1M.json"), help="'' = print only")
    args = ap.parse_args()

    import numpy as np
    import torch

    from bench import gist_like_gpu
    from lab_1806_vec_db_amd import vecdb
    from lab_1806_vec_db_amd.vecdb import VecDB

    dev = torch.device("cuda", 0)
    n, dim, T, k = args.rows, args.dim, args.tenants, args.k
    db = VecDB()
    db.create_table_if_not_exists("t", dim, "l2sqr")
    t = db._tables["t"]
    ix = t.index
    base = gist_like_gpu(torch, n, dim, 1806, dev)
    ix.add_device(base.data_ptr(), n)  # (the rows go in from the device: a host copy of 3.84 GB is no part of what is measured)
    del base
    t.metadata = [{"id": str(i), "tenant": str(i % T), "tier": "gold" if i % 2 else "free"} for i in range(n)]
    qs = gist_like_gpu(torch, T, dim, 1807, dev).cpu().numpy()
    extra = gist_like_gpu(torch, 1, dim, 1809, dev).cpu().numpy()
    t.create_columns([{"tenant": "0", "tier": "gold"}])
    col = t.codec.column_of("tenant")

    def wall(fn, reps=args.reps):
        ts, out = [], None
        for _ in range(reps):
            t0 = time.perf_counter()
            out = fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return {"ms_median": float(np.median(ts)), "ms_min": float(np.min(ts)), "ms_max": float(np.max(ts)), "reps": reps}, out

    rec = {"what": "one label column grouped by code in one pass: vdb_mask_create_partition vs vdb_mask_create_where_many for the same codes, "
                   "VecDB.batch_search after a write with the routing on / off, VecDB.count_by vs the host Counter loop; host clock around "
                   "synchronised calls, same process, same table",
           "rows": n, "dim": dim, "tenants": T, "rows_per_tenant": n // T, "k": k}

    # ---- masks: the same G codes through both calls
    codes_all = [t.codec.terms({"tenant": str(j)})[0][1] for j in range(T)]
    rec["masks"] = {}
    partition_min = None
    for G in [int(g) for g in args.groups.split(",")]:
        G = min(G, T)
        codes = codes_all[:G]
        terms = [[(col, c)] for c in codes]
        part, where = ix.make_masks_partition(col, codes), ix.make_masks_where(terms)
        for a, b in zip(part, where):  # identical before anything is timed
            assert all(np.array_equal(x, y) for x, y in zip(a.rows(), b.rows())) and len(a) == len(b) == n // T
        for mk in part + where:
            mk.close()

        def run_part():
            for mk in ix.make_masks_partition(col, codes):
                mk.close()

        def run_where():
            for mk in ix.make_masks_where(terms):
                mk.close()

        e = {}
        for name, fn, prof in (("partition", run_part, "mask_partition"), ("where_many", run_where, "mask_where")):
            fn()
            e[name], _ = wall(fn)
            ix.prof_enable(True)
            ix.prof_reset()
            fn()
            p = ix.prof_get(prof)
            ix.prof_enable(False)
            e[name].update({"kernels_ms": p["ms"], "kernel_launch_groups": p["launches"], "kernel_gbytes": p["bytes"] / 1e9})
        e["wall_where_over_partition"] = e["where_many"]["ms_median"] / e["partition"]["ms_median"]
        e["kernels_where_over_partition"] = e["where_many"]["kernels_ms"] / e["partition"]["kernels_ms"] if e["partition"]["kernels_ms"] else None
        rec["masks"][str(G)] = e
        if partition_min is None and e["partition"]["ms_median"] < e["where_many"]["ms_median"]:
            partition_min = G
    rec["partition_min"] = partition_min
    top = rec["masks"][str(max(int(g) for g in rec["masks"]))]
    rec["claim_partition_below_where_many_at_largest_group"] = {
        "kernels": top["partition"]["kernels_ms"] < top["where_many"]["kernels_ms"], "call": top["partition"]["ms_median"] < top["where_many"]["ms_median"]}

    # ---- VecDB.batch_search after a write, routing on / off
    pats = [{"tenant": str(j)} for j in range(T)]

    def cold():
        db.batch_add("t", extra, [{"id": "extra", "tenant": "none", "tier": "free"}])
        assert not t.masks
        t0 = time.perf_counter()
        out = db.batch_search("t", qs, k, filters=pats)
        return (time.perf_counter() - t0) * 1e3, out

    rec["batch_search_after_write"] = {}
    answers = {}
    saved = vecdb.PARTITION_MIN
    try:
        for name, pm in (("routing_off", None), ("routing_on", 1)):
            vecdb.PARTITION_MIN = pm
            cold()  # warm-up (mirrors of the search tiers, code objects)
            ts = []
            for _ in range(args.reps):
                ms, answers[name] = cold()
                ts.append(ms)
            rec["batch_search_after_write"][name] = {"ms_median": float(np.median(ts)), "ms_min": float(np.min(ts)), "ms_max": float(np.max(ts)),
                                                     "reps": args.reps, "partition_min": pm}
    finally:
        vecdb.PARTITION_MIN = saved
    assert answers["routing_on"] == answers["routing_off"]
    rec["batch_search_after_write"]["off_over_on"] = (rec["batch_search_after_write"]["routing_off"]["ms_median"] /
                                                      rec["batch_search_after_write"]["routing_on"]["ms_median"])
    rec["batch_search_warm"], _ = wall(lambda: db.batch_search("t", qs, k, filters=pats))

    # ---- count_by against the host loop
    rec["count_by"] = {}
    for name, f, fn in (("no_filter", None, lambda m: True), ("tier_gold", {"tier": "gold"}, lambda m: m.get("tier") == "gold")):
        def host():
            return dict(collections.Counter(m.get("tenant") for m in t.metadata if fn(m)))

        want = host()
        assert db.count_by("t", "tenant", f) == want
        e = {}
        e["device"], _ = wall(lambda: db.count_by("t", "tenant", f))
        e["host_loop"], _ = wall(host, reps=args.host_reps)
        ix.prof_enable(True)
        ix.prof_reset()
        db.count_by("t", "tenant", f)
        p = ix.prof_get("label_counts")
        ix.prof_enable(False)
        e["device"].update({"kernels_ms": p["ms"], "kernel_launch_groups": p["launches"], "values": len(want)})
        e["host_over_device"] = e["host_loop"]["ms_median"] / e["device"]["ms_median"]
        rec["count_by"][name] = e
    rec["stats"] = {s: ix.get_stat(s) for s in ("mask_partition_masks", "mask_where_masks", "label_count_calls")}
    print(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    db.delete_table("t")


if __name__ == "__main__":
    main()
