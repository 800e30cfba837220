#!/usr/bin/env python3
"""Document-level fused Flat search (vdb_flat_knn_fused_groups: the lists of several sub-queries joined by the value of a label column)
against its floor and against what a caller did before, same process, same table.

1M x 960 f32 rows (bench data, seed 1806) in a VecDB table with a `doc` label column of 10 rows per value, 1000 fused queries of
S = 2, 4, 8, 32 sub-queries each (a base vector plus small perturbations), k = 10, fetch_k in 20, 40, 64, 128.  Host clock around calls
that end synchronised, median of --reps (10) with the range, everything from this one run; per (S, fetch_k):
  groups_rrf / _min / _sum   vdb_flat_knn_fused_groups_device: ONE list call over the S x 1000 sub-queries at K' = fetch_k, then k_fuse_groups
  kernel                     k_fuse_groups alone, between events (vdb_prof_get "fuse_groups" of one more call with the profile on)
  floor                      vdb_flat_knn_fused_device (RRF) on the SAME sub-queries: the row-level fusion, the same list call under it
  host                       what a caller did before: VecDB.batch_search(k = fetch_k) over the sub-queries, every hit through
                             dict(metadata) on the host, a Python dictionary of per-document RRF scores per question and a sort
The answers of 32 questions are compared with tests/fuse_groups_ref.py over the lists of a vdb_flat_knn_device call before anything is
timed (representatives and score bits).  Nothing is gated on the ratios.  Writes one JSON record (default
profiles/flat_fuse_groups_1M.json)."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

COLUMN, PER_DOC = 0, 10
MODES = ("rrf", "min", "sum")


def host_rrf_by_doc(res, lims, k, c=60.0):
    """the caller's loop: per question a dictionary document -> score over its hit lists (a document counts once per list, at its first
    hit, by its rank among the documents of the list), sorted"""
    out = []
    for q in range(len(lims) - 1):
        score = {}
        for hits in res[lims[q]:lims[q + 1]]:
            seen = {}
            for meta, _ in hits:
                seen.setdefault(meta["doc"], len(seen))
            for doc, rank in seen.items():
                score[doc] = score.get(doc, 0.0) + 1.0 / (rank + 1 + c)
        out.append(sorted(score, key=lambda d: (-score[d], int(d)))[:k])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=960)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--lists", type=str, default="2,4,8,32")
    ap.add_argument("--fetch", type=str, default="20,40,64,128")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "flat_fuse_groups_1M.json"), help="'' = print only")
    args = ap.parse_args()

    import numpy as np
    import torch

    import fuse_groups_ref as R
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
    labels = (np.arange(n) // PER_DOC).astype(np.uint32)
    ix.set_labels(COLUMN, labels)
    t.metadata = [{"id": str(i), "doc": str(i // PER_DOC)} for i in range(n)]
    seeds = gist_like_gpu(torch, nq, dim, 1807, dev)
    group_of = R.label_groups(labels)

    def wall(fn, reps):
        ts, out = [], None
        for _ in range(reps):
            t0 = time.perf_counter()
            out = fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return {"ms_median": float(np.median(ts)), "ms_min": float(np.min(ts)), "ms_max": float(np.max(ts)), "reps": reps}, out

    rec = {"what": "document-level fused Flat search (RRF / min / sum over the lists of S sub-queries per question, joined by a label column "
                   "of 10 rows per value) against vdb_flat_knn_fused_device on the same sub-queries (the floor), k_fuse_groups alone between "
                   "events, and VecDB.batch_search(k = fetch_k) plus a Python per-document dictionary fusion; host clock around synchronised "
                   "calls, medians with their ranges, one process, one table",
           "rows": n, "dim": dim, "rows_per_document": PER_DOC, "fused_queries": nq, "k": k, "rrf_c": 60.0, "cases": {}}

    for S in [int(x) for x in args.lists.split(",")]:
        gen = torch.Generator(device=dev)
        gen.manual_seed(1900 + S)
        noise = torch.randn((nq, S, dim), generator=gen, device=dev, dtype=torch.float32) * 0.02
        noise[:, 0] = 0  # the first sub-query is the question itself
        tq = (seeds[:, None, :] + noise).clamp_(0, 0.8).reshape(nq * S, dim).contiguous()
        qs = tq.cpu().numpy()
        lims = np.arange(0, nq * S + 1, S, dtype=np.uint64)
        for fk in [int(x) for x in args.fetch.split(",")]:
            if S * fk > 16384:
                continue
            o_i = torch.zeros((nq, k), dtype=torch.int64, device=dev)
            o_d = torch.zeros((nq, k), dtype=torch.float32, device=dev)
            o_c = torch.zeros((nq,), dtype=torch.int64, device=dev)
            o_e = torch.zeros((nq,), dtype=torch.uint8, device=dev)
            l_i = torch.zeros((nq * S, fk), dtype=torch.int64, device=dev)
            l_d = torch.zeros((nq * S, fk), dtype=torch.float32, device=dev)
            l_c = torch.zeros((nq * S,), dtype=torch.int64, device=dev)
            torch.cuda.synchronize()

            def groups(mode="rrf"):
                ix.flat_knn_fused_groups_device(tq.data_ptr(), lims, k, fk, COLUMN, o_i.data_ptr(), o_d.data_ptr(), o_c.data_ptr(), o_e.data_ptr(),
                                                mode=mode)

            def floor():
                ix.flat_knn_fused_device(tq.data_ptr(), lims, k, fk, o_i.data_ptr(), o_d.data_ptr(), o_c.data_ptr(), mode="rrf")

            # ---- correctness first: 32 questions against the reference over the lists of a plain search
            ix.flat_knn_device(tq.data_ptr(), nq * S, fk, l_i.data_ptr(), l_d.data_ptr(), l_c.data_ptr())
            li, ld = l_i.cpu().numpy().view(np.uint64), l_d.cpu().numpy()
            chk = min(32, nq)
            docs = []
            for mode in MODES:
                groups(mode)
                gi, gd, ge = o_i[:chk].cpu().numpy().view(np.uint64), o_d[:chk].cpu().numpy(), o_e[:chk].cpu().numpy()
                for q in range(chk):
                    ids, sc, ex = R.fuse_groups([(li[j], ld[j]) for j in range(q * S, (q + 1) * S)], group_of, k, mode, trunc_len=fk)
                    assert gi[q].tolist() == ids.tolist() and gd[q].view(np.uint32).tolist() == sc.view(np.uint32).tolist(), (S, fk, mode, q)
                    assert ge[q] == ex, (S, fk, mode, q)
                    docs.append(len({int(r) // PER_DOC for r in li[q * S:(q + 1) * S].reshape(-1).tolist()}))

            e = {"checked_queries": chk, "mean_distinct_documents_per_question": float(np.mean(docs))}
            for mode in MODES:
                e["groups_" + mode], _ = wall(lambda: groups(mode), args.reps)
            e["floor_flat_knn_fused_device"], _ = wall(floor, args.reps)
            ker = []
            for _ in range(5):
                ix.prof_enable(True)
                ix.prof_reset()
                groups()
                p = ix.prof_get("fuse_groups")
                ix.prof_enable(False)
                ker.append(p["ms"])
            e["kernel_between_events"] = {"ms_median": float(np.median(ker)), "ms_min": float(np.min(ker)), "ms_max": float(np.max(ker)), "reps": 5,
                                          "launches": p["launches"]}
            e["kernel_share_of_call"] = e["kernel_between_events"]["ms_median"] / e["groups_rrf"]["ms_median"]
            e["groups_over_floor"] = {m: e["groups_" + m]["ms_median"] / e["floor_flat_knn_fused_device"]["ms_median"] for m in MODES}

            def host():
                return host_rrf_by_doc(db.batch_search("t", qs, fk), lims.tolist(), k)

            if args.host_reps > 0:
                e["host_alternative"], hres = wall(host, args.host_reps)
                e["host_over_groups"] = e["host_alternative"]["ms_median"] / e["groups_rrf"]["ms_median"]
                groups()
                gi = o_i[:chk].cpu().numpy()
                e["host_questions_with_the_same_top_k_documents"] = int(sum(set(map(int, hres[q])) == {int(r) // PER_DOC for r in gi[q].tolist()}
                                                                            for q in range(chk)))
            rec["cases"]["S=%d,fetch_k=%d" % (S, fk)] = e
            print("S=%d fetch_k=%d: groups %.2f ms, floor %.2f ms, kernel %.3f ms" % (S, fk, e["groups_rrf"]["ms_median"],
                                                                                    e["floor_flat_knn_fused_device"]["ms_median"],
                                                                                    e["kernel_between_events"]["ms_median"]), file=sys.stderr, flush=True)

    rec["stats"] = {s: ix.get_stat(s) for s in ("flat_fused_groups_calls", "flat_fused_groups_queries", "flat_fused_groups_lists")}
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    db.delete_table("t")


if __name__ == "__main__":
    main()
