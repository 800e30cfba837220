#!/usr/bin/env python3
"""Fused multi-query Flat search (vdb_flat_knn_fused: the lists of several sub-queries joined by reciprocal rank fusion or by the smallest
distance) against its floor and against what a caller did before, same process, same table.

1M x 960 f32 rows (bench data, seed 1806) in a VecDB table, 1000 fused queries of S = 2, 4, 8 sub-queries each (a base vector plus small
perturbations: paraphrases, lists that overlap in part), k = 10, fetch_k in 20, 40, 64, 128.  Host clock around calls that end
synchronised, median of --reps (10) with the range, everything from this one run; per (S, fetch_k):
  fused        vdb_flat_knn_fused_device (RRF, c = 60): ONE list call over the S x 1000 sub-queries at K' = fetch_k, then k_fuse_lists
  fused_min    the same with VDB_FUSE_MIN
  kernel       k_fuse_lists alone, between events (vdb_prof_get "fuse_lists" of one more call with the profile on)
  floor        vdb_flat_knn_device at k = fetch_k over the same S x 1000 sub-queries: the list call the fused call cannot beat
  host         what a caller did before: VecDB.batch_search(k = fetch_k) over the sub-queries, every hit through dict(metadata) on the
               host, a Python dictionary of RRF scores per question and a sort
The fused answers of 32 questions are compared with tests/fuse_ref.py over the floor call's lists before anything is timed (ids and
score bits).  Writes one JSON record (default profiles/flat_fuse_1M.json)."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

TIERS = ("flat_i8_queries", "flat_i8_redo", "flat_half_queries", "flat_half_redo", "flat_fallback")


def host_rrf(res, lims, k, c=60.0):
    """the caller's loop: per question a dictionary id -> score over its hit lists, sorted"""
    out = []
    for q in range(len(lims) - 1):
        score = {}
        for hits in res[lims[q]:lims[q + 1]]:
            for rank, (meta, _) in enumerate(hits):
                score[meta["id"]] = score.get(meta["id"], 0.0) + 1.0 / (rank + 1 + c)
        out.append(sorted(score, key=lambda i: (-score[i], int(i)))[:k])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=960)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--lists", type=str, default="2,4,8")
    ap.add_argument("--fetch", type=str, default="20,40,64,128")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "flat_fuse_1M.json"), help="'' = print only")
    args = ap.parse_args()

    import numpy as np
    import torch

    import fuse_ref as R
    from bench import gist_like_gpu
    from lab_1806_vec_db_amd.vecdb import VecDB

    dev = torch.device("cuda", 0)
    n, dim, k, nq = args.rows, args.dim, args.k, args.queries
    db = VecDB()
    db.create_table_if_not_exists("t", dim, "l2sqr")
    t = db._tables["t"]
    ix = t.index
    base = gist_like_gpu(torch, n, dim, 1806, dev)
    ix.add_device(base.data_ptr(), n)  # (the rows go in from the device: a host copy of 3.84 GB is no part of what is measured)
    del base
    t.metadata = [{"id": str(i)} for i in range(n)]
    seeds = gist_like_gpu(torch, nq, dim, 1807, dev)

    def wall(fn, reps):
        ts, out = [], None
        for _ in range(reps):
            t0 = time.perf_counter()
            out = fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return {"ms_median": float(np.median(ts)), "ms_min": float(np.min(ts)), "ms_max": float(np.max(ts)), "reps": reps}, out

    rec = {"what": "fused multi-query Flat search (RRF / min-distance over the lists of S sub-queries per question) against vdb_flat_knn_device "
                   "over the same S x nq sub-queries at k = fetch_k (the floor), k_fuse_lists alone between events, and VecDB.batch_search(k = "
                   "fetch_k) plus a Python dictionary fusion; host clock around synchronised calls, medians with their ranges, one process, one "
                   "table",
           "rows": n, "dim": dim, "fused_queries": nq, "k": k, "rrf_c": 60.0, "cases": {}}

    for S in [int(x) for x in args.lists.split(",")]:
        gen = torch.Generator(device=dev)
        gen.manual_seed(1900 + S)
        noise = torch.randn((nq, S, dim), generator=gen, device=dev, dtype=torch.float32) * 0.02
        noise[:, 0] = 0  # the first sub-query is the question itself
        tq = (seeds[:, None, :] + noise).clamp_(0, 0.8).reshape(nq * S, dim).contiguous()
        qs = tq.cpu().numpy()
        lims = np.arange(0, nq * S + 1, S, dtype=np.uint64)
        for fk in [int(x) for x in args.fetch.split(",")]:
            o_i = torch.zeros((nq, k), dtype=torch.int64, device=dev)
            o_d = torch.zeros((nq, k), dtype=torch.float32, device=dev)
            o_c = torch.zeros((nq,), dtype=torch.int64, device=dev)
            l_i = torch.zeros((nq * S, fk), dtype=torch.int64, device=dev)
            l_d = torch.zeros((nq * S, fk), dtype=torch.float32, device=dev)
            l_c = torch.zeros((nq * S,), dtype=torch.int64, device=dev)
            torch.cuda.synchronize()

            def fused(mode="rrf"):
                ix.flat_knn_fused_device(tq.data_ptr(), lims, k, fk, o_i.data_ptr(), o_d.data_ptr(), o_c.data_ptr(), mode=mode)

            def floor():
                ix.flat_knn_device(tq.data_ptr(), nq * S, fk, l_i.data_ptr(), l_d.data_ptr(), l_c.data_ptr())

            # ---- correctness first: 32 questions against the reference over the floor call's lists
            floor()
            li, ld = l_i.cpu().numpy().view(np.uint64), l_d.cpu().numpy()
            chk = min(32, nq)
            union = []
            for mode in ("rrf", "min"):
                fused(mode)
                gi, gd = o_i[:chk].cpu().numpy().view(np.uint64), o_d[:chk].cpu().numpy()
                for q in range(chk):
                    ids, sc = R.fuse([(li[j], ld[j]) for j in range(q * S, (q + 1) * S)], k, mode)
                    assert gi[q].tolist() == ids.tolist() and gd[q].view(np.uint32).tolist() == sc.view(np.uint32).tolist(), (S, fk, mode, q)
                    union.append(len(set(li[q * S:(q + 1) * S].reshape(-1).tolist())))

            e = {"checked_queries": chk, "mean_distinct_rows_per_question": float(np.mean(union))}
            s0 = {s: ix.get_stat(s) for s in TIERS}
            e["fused_rrf"], _ = wall(fused, args.reps)
            e["fused_rrf"]["list_call_tiers_per_call"] = {s: (ix.get_stat(s) - s0[s]) / args.reps for s in TIERS}
            e["fused_min"], _ = wall(lambda: fused("min"), args.reps)
            e["floor_flat_knn_device"], _ = wall(floor, args.reps)
            ker = []
            for _ in range(5):
                ix.prof_enable(True)
                ix.prof_reset()
                fused()
                p = ix.prof_get("fuse_lists")
                ix.prof_enable(False)
                ker.append(p["ms"])
            e["kernel_between_events"] = {"ms_median": float(np.median(ker)), "ms_min": float(np.min(ker)), "ms_max": float(np.max(ker)), "reps": 5,
                                          "launches": p["launches"]}
            e["kernel_share_of_fused"] = e["kernel_between_events"]["ms_median"] / e["fused_rrf"]["ms_median"]
            e["fused_over_floor"] = e["fused_rrf"]["ms_median"] / e["floor_flat_knn_device"]["ms_median"]

            def host():
                return host_rrf(db.batch_search("t", qs, fk), lims.tolist(), k)

            e["host_alternative"], hres = wall(host, args.host_reps)
            e["host_over_fused"] = e["host_alternative"]["ms_median"] / e["fused_rrf"]["ms_median"]
            fused()
            gi = o_i[:chk].cpu().numpy()
            e["host_questions_with_the_same_top_k_set"] = int(sum(set(map(int, hres[q])) == set(gi[q].tolist()) for q in range(chk)))
            rec["cases"]["S=%d,fetch_k=%d" % (S, fk)] = e

    rec["stats"] = {s: ix.get_stat(s) for s in ("flat_fused_calls", "flat_fused_queries", "flat_fused_lists")}
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    db.delete_table("t")


if __name__ == "__main__":
    main()
