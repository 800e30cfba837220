#!/usr/bin/env python3
"""Outlier scores (vdb_flat_outliers_device: the k-NN self-join of the table's own rows + k_lof_lrd / k_lof_score) at k = 20 on the
--rows x --dim (default 1M x 960) gist-like corpus the other tools build, under L2Sqr and under Cosine, with its parts:
  walk     vdb_flat_knn_graph_device alone (one search call at k + 1 per 16384 rows + k_knn_self_pack)
  stages   vdb_lof_lists_device alone over that graph (id check, k-distances, k_lof_lrd, k_lof_score)
  floor    what the walk should cost: vdb_flat_knn_device over the same rows as queries at k + 1, in the same chunks
and, on a --prefix-row prefix (default 20 000) as a table of its own, the same answer obtained the way it had to be before: flat_knn_like
over single positives at k = 20 in batches of 1000, ids and distances to the host, LOF in numpy -- against outliers() on that prefix, whose
scores it must match.  Medians of --calls (default 5) synchronised calls after one warm-up call each, host clock, one process.  Not
measured: masks, other k, other chunk sizes.  Nothing is gated on these numbers.  Writes --out as JSON."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
K, CHUNK = 20, 16384  # DUP_CHUNK_DEFAULT of csrc/dup_plan.hpp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=960)
    ap.add_argument("--prefix", type=int, default=20_000)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "flat_outliers_1M.json"), help="'' = print only")
    args = ap.parse_args()

    import numpy as np
    import torch

    import lab_1806_vec_db_amd as vdb
    from bench import gist_like_gpu

    dev = torch.device("cuda", 0)
    n, dim = args.rows, args.dim
    base = gist_like_gpu(torch, n, dim, 1806, dev)

    def median_ms(fn, name=""):
        fn()  # warm-up: builds what the first call builds
        out = []
        for _ in range(args.calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()  # (returns synchronised)
            out.append((time.perf_counter() - t0) * 1e3)
        print(name, [round(x, 1) for x in out], file=sys.stderr, flush=True)
        return {"median_ms": statistics.median(out), "min_ms": min(out), "max_ms": max(out), "calls": len(out)}

    rec = {"what": "outlier scores at k = 20 (vdb_flat_outliers_device) and their parts; medians of synchronised calls after a warm-up, host clock",
           "rows": n, "dim": dim, "k": K, "chunk": CHUNK, "graph_bytes": 8 * n * K}
    ids = torch.zeros((n, K), dtype=torch.int64, device=dev)
    nd = torch.zeros((n, K), dtype=torch.float32, device=dev)
    cnt = torch.zeros((n,), dtype=torch.int64, device=dev)
    sc = [torch.zeros((n,), dtype=torch.float32, device=dev) for _ in range(3)]
    l_idx = torch.zeros((CHUNK, K + 1), dtype=torch.int64, device=dev)
    l_d = torch.zeros((CHUNK, K + 1), dtype=torch.float32, device=dev)
    l_c = torch.zeros((CHUNK,), dtype=torch.int64, device=dev)
    for metric in ("l2sqr", "cosine"):
        ix = vdb.GpuIndex(dim, metric, device=0)
        ix.add_device(base.data_ptr(), n)

        def floor():
            for a in range(0, n, CHUNK):
                ix.flat_knn_device(base.data_ptr() + a * dim * 4, min(CHUNK, n - a), K + 1, l_idx.data_ptr(), l_d.data_ptr(), l_c.data_ptr())

        r = {"outliers": median_ms(lambda: ix.outliers_device(K, *(s.data_ptr() for s in sc))),
             "walk": median_ms(lambda: ix.knn_graph_device(K, ids.data_ptr(), nd.data_ptr(), cnt.data_ptr())),
             "floor_knn_at_k_plus_1": median_ms(floor)}
        nbr32, cnt32 = ids.to(torch.int32), cnt.to(torch.int32)  # (id_offset 0: the ids are the local rows)
        lof_walk = sc[2].clone()
        r["stages"] = median_ms(lambda: ix.lof_lists_device(nbr32.data_ptr(), nd.data_ptr(), cnt32.data_ptr(), n, K, *(s.data_ptr() for s in sc)))
        r["stages_match_outliers_bits"] = bool(torch.equal(lof_walk.view(torch.int32), sc[2].view(torch.int32)))
        r["stages_share"] = r["stages"]["median_ms"] / r["outliers"]["median_ms"]
        r["walk_to_floor"] = r["walk"]["median_ms"] / r["floor_knn_at_k_plus_1"]["median_ms"]
        rec[metric] = r
        del nbr32, cnt32
        ix.close()

    # the same answer the way it had to be obtained before, on a prefix as a table of its own
    p = min(args.prefix, n)
    px = vdb.GpuIndex(dim, "l2sqr", device=0)
    px.add_device(base.data_ptr(), p)

    def before():
        nb, dd = np.zeros((p, K), dtype=np.int64), np.zeros((p, K), dtype=np.float32)
        for a in range(0, p, 1000):
            i, d, _ = px.flat_knn_like([[r] for r in range(a, min(a + 1000, p))], K)
            nb[a:a + len(i)], dd[a:a + len(i)] = i, d
        kd = dd[:, K - 1]
        lrd = 1.0 / (np.maximum(kd[nb], dd).astype(np.float64).mean(axis=1) + 1e-10)
        return lrd[nb].mean(axis=1) / lrd

    lof_before = before()
    lof_now = px.outliers(K)[2]
    rec["prefix"] = {"rows": p, "before_knn_like_plus_numpy": median_ms(before), "outliers": median_ms(lambda: px.outliers(K)),
                     "max_rel_diff": float(np.max(np.abs(lof_now - lof_before) / lof_before))}
    rec["prefix"]["speedup"] = rec["prefix"]["before_knn_like_plus_numpy"]["median_ms"] / rec["prefix"]["outliers"]["median_ms"]
    rec["not_measured"] = ["masks", "other k", "other chunk sizes", "the full table the old way"]
    px.close()
    print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
