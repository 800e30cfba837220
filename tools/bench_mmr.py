#!/usr/bin/env python3
"""Diversified Flat k-NN (vdb_flat_knn_mmr: maximal marginal relevance over the fetch_k nearest rows) against its floor and against what a
caller did before, same process, same table.

1M x 960 f32 rows (bench data, seed 1806) in a VecDB table, 1000 queries, k = 10, lambda = 0.5, fetch_k in 20, 40, 64, 128.  Host clock
around calls that end synchronised, median of --reps (20) with the range, everything from this one run; per fetch_k:
  mmr          vdb_flat_knn_mmr_device: the list call at k = fetch_k, then k_mmr_select
  select       k_mmr_select alone, between events (vdb_prof_get "mmr_select" of one more call with the profile on)
  floor        vdb_flat_knn_device at k = fetch_k, unfiltered, the same queries: the list call the mmr call cannot beat
  host         what a caller did before: VecDB.batch_search(k = fetch_k, with_vectors=True) -- fetch_k x dim floats per query to the
               host -- plus a numpy greedy loop over the returned vectors (its distances are numpy's, not the library's bit-exact ones)
The mmr answers of 32 queries are compared with a numpy walk over the list call's rows before anything is timed (ids; the walk's pair
distances are float64, so a query whose scores tie within rounding is reported, not failed).  Writes one JSON record (default
profiles/flat_mmr_1M.json)."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TIERS = ("flat_i8_queries", "flat_i8_redo", "flat_half_queries", "flat_half_redo", "flat_fallback")


def greedy(np, d, vecs, k, lam):
    """the caller's loop: positions selected from one query's hits (distances d, vectors vecs), squared L2 between the vectors"""
    F = len(d)
    near = np.full(F, np.inf)
    taken = np.zeros(F, dtype=bool)
    sel = [0]
    taken[0] = True
    while len(sel) < min(k, F):
        diff = vecs - vecs[sel[-1]]
        near = np.minimum(near, np.einsum("ij,ij->i", diff, diff))
        score = np.where(taken, np.inf, lam * d - (1.0 - lam) * near)
        sel.append(int(np.argmin(score)))
        taken[sel[-1]] = True
    return sel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=960)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--fetch", type=str, default="20,40,64,128")
    ap.add_argument("--lam", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "flat_mmr_1M.json"), help="'' = print only")
    args = ap.parse_args()

    import numpy as np
    import torch

    from bench import gist_like_gpu
    from lab_1806_vec_db_amd.vecdb import VecDB

    dev = torch.device("cuda", 0)
    n, dim, k, nq, lam = args.rows, args.dim, args.k, args.queries, args.lam
    db = VecDB()
    db.create_table_if_not_exists("t", dim, "l2sqr")
    t = db._tables["t"]
    ix = t.index
    base = gist_like_gpu(torch, n, dim, 1806, dev)
    ix.add_device(base.data_ptr(), n)  # (the rows go in from the device: a host copy of 3.84 GB is no part of what is measured)
    del base
    t.metadata = [{"id": str(i)} for i in range(n)]
    tq = gist_like_gpu(torch, nq, dim, 1807, dev)
    qs = tq.cpu().numpy()

    def wall(fn, reps):
        ts, out = [], None
        for _ in range(reps):
            t0 = time.perf_counter()
            out = fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return {"ms_median": float(np.median(ts)), "ms_min": float(np.min(ts)), "ms_max": float(np.max(ts)), "reps": reps}, out

    rec = {"what": "diversified Flat k-NN (maximal marginal relevance over the fetch_k nearest rows) against vdb_flat_knn_device at k = fetch_k "
                   "(the floor), k_mmr_select alone between events, and VecDB.batch_search(k = fetch_k, with_vectors=True) plus a numpy greedy "
                   "loop; host clock around synchronised calls, medians with their ranges, one process, one table",
           "rows": n, "dim": dim, "queries": nq, "k": k, "lambda": lam, "fetch_k": {}}

    for fk in [int(x) for x in args.fetch.split(",")]:
        o_i = torch.zeros((nq, k), dtype=torch.int64, device=dev)
        o_d = torch.zeros((nq, k), dtype=torch.float32, device=dev)
        o_c = torch.zeros((nq,), dtype=torch.int64, device=dev)
        l_i = torch.zeros((nq, fk), dtype=torch.int64, device=dev)
        l_d = torch.zeros((nq, fk), dtype=torch.float32, device=dev)
        l_c = torch.zeros((nq,), dtype=torch.int64, device=dev)
        torch.cuda.synchronize()

        def mmr():
            ix.flat_knn_mmr_device(tq.data_ptr(), nq, k, fk, lam, o_i.data_ptr(), o_d.data_ptr(), o_c.data_ptr())

        def floor():
            ix.flat_knn_device(tq.data_ptr(), nq, fk, l_i.data_ptr(), l_d.data_ptr(), l_c.data_ptr())

        # ---- correctness first: 32 queries against a numpy walk over the list call's rows
        mmr()
        floor()
        chk = min(32, nq)
        got = o_i[:chk].cpu().numpy()
        li, ld = l_i[:chk].cpu().numpy(), l_d[:chk].cpu().numpy()
        vec = ix.get_rows(li.reshape(-1).astype(np.uint64)).reshape(chk, fk, dim).astype(np.float64)
        differ = sum(got[q].tolist() != li[q][greedy(np, ld[q].astype(np.float64), vec[q], k, lam)].tolist() for q in range(chk))
        assert differ <= chk // 8, (fk, differ)  # (float64 pair distances: a near-tie may fall the other way; anything more is a bug)

        e = {"checked_queries": chk, "checked_queries_differing_from_float64_walk": int(differ)}
        s0 = {s: ix.get_stat(s) for s in TIERS}
        e["mmr"], _ = wall(mmr, args.reps)
        e["mmr"]["list_call_tiers_per_call"] = {s: (ix.get_stat(s) - s0[s]) / args.reps for s in TIERS}
        e["floor_flat_knn_device"], _ = wall(floor, args.reps)
        sel_ms = []
        for _ in range(5):
            ix.prof_enable(True)
            ix.prof_reset()
            mmr()
            p = ix.prof_get("mmr_select")
            ix.prof_enable(False)
            sel_ms.append(p["ms"])
        e["select_between_events"] = {"ms_median": float(np.median(sel_ms)), "ms_min": float(np.min(sel_ms)), "ms_max": float(np.max(sel_ms)), "reps": 5,
                                      "launches": p["launches"]}
        e["select_share_of_mmr"] = e["select_between_events"]["ms_median"] / e["mmr"]["ms_median"]
        e["mmr_over_floor"] = e["mmr"]["ms_median"] / e["floor_flat_knn_device"]["ms_median"]

        def host():
            res = db.batch_search("t", qs, fk, with_vectors=True)
            out = []
            for r in res:
                d = np.array([x[1] for x in r])
                v = np.stack([x[2] for x in r])
                out.append([r[p][0]["id"] for p in greedy(np, d, v, k, lam)])
            return out

        e["host_alternative"], _ = wall(host, args.host_reps)
        e["host_over_mmr"] = e["host_alternative"]["ms_median"] / e["mmr"]["ms_median"]
        rec["fetch_k"][str(fk)] = e

    rec["stats"] = {s: ix.get_stat(s) for s in ("flat_mmr_calls", "flat_mmr_queries")}
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    db.delete_table("t")


if __name__ == "__main__":
    main()
