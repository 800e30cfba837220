#!/usr/bin/env python3
"""Exact filtered Flat k-NN against the unfiltered call it shares its corpus pass with, same process, same queries, legs alternating.

  filtered leg: vdb_flat_knn_filtered_device at k = K under a random mask of m allowed rows
  k-NN leg    : vdb_flat_knn_device at k = K (unchanged by the filtered search: the parent's number measured in the same run)

Device events around calls that end synchronised; WARMUP + STEPS steps of NQ queries on the default bench data (1M x 960 gist-like
rows, seeds 1806 / 1807).  Cases: random masks at m / n = 0.5, 0.1, 0.01 (the 8-bit tier with the masked row constants) and masks of
m = 1024 and 8192 rows (the direct path: gathered strict-order scan), each with its hand-on count (queries the tier gave to the
direct path).  Then the sweep behind the default of "flat_filtered_direct_max": m in powers of two, the tier forced (mode 2, threshold
0) and the direct path forced (mode 1), both curves in the same record.  Writes one JSON record (default
profiles/flat_filtered_1M.json)."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FSTATS = ("flat_filtered_queries", "flat_filtered_direct_queries", "flat_filtered_i8_queries", "flat_filtered_fallback_queries")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=960)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--dist", choices=["l2sqr", "cosine"], default="l2sqr")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sweep-steps", type=int, default=5)
    ap.add_argument("--sweep-max", type=int, default=65536, help="largest m of the direct-vs-tier sweep (powers of two from 256)")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "flat_filtered_1M.json"), help="'' = print only")
    args = ap.parse_args()

    import numpy as np
    import torch

    import lab_1806_vec_db_amd as vdb
    from bench import gist_like_gpu

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
    rng = np.random.default_rng(1808)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def knn_step():
        return timed(lambda: ix.flat_knn_device(qs.data_ptr(), nq, k, oi.data_ptr(), od.data_ptr(), oc.data_ptr()))

    def filtered_step(mk):
        return timed(lambda: ix.flat_knn_filtered_device(qs.data_ptr(), nq, k, mk, oi.data_ptr(), od.data_ptr(), oc.data_ptr()))

    def legs(mk, steps, warmup, with_knn=True):
        for _ in range(warmup):
            filtered_step(mk)
            if with_knn:
                knn_step()
        s0 = {s: ix.get_stat(s) for s in FSTATS}
        tf, tk = [], []
        for _ in range(steps):
            tf.append(filtered_step(mk))
            if with_knn:
                tk.append(knn_step())
        d = {s: ix.get_stat(s) - s0[s] for s in FSTATS}
        return tf, tk, d

    cases = []
    for name, m in (("m/n=0.5", n // 2), ("m/n=0.1", n // 10), ("m/n=0.01", n // 100), ("m=8192", 8192), ("m=1024", 1024)):
        m = min(m, n)
        mk = ix.make_mask(rng.choice(n, m, replace=False))
        tf, tk, d = legs(mk, args.steps, args.warmup)
        mk.close()
        cases.append({
            "mask": name, "m": m, "path": "tier" if d["flat_filtered_i8_queries"] else "direct",
            "filtered_step_ms_median": float(np.median(tf)), "filtered_step_ms_min": float(np.min(tf)), "filtered_step_ms_max": float(np.max(tf)),
            "knn_step_ms_median": float(np.median(tk)), "knn_step_ms_min": float(np.min(tk)), "knn_step_ms_max": float(np.max(tk)),
            "filtered_over_knn": float(np.median(tf) / np.median(tk)),
            "handed_on_per_step": d["flat_filtered_fallback_queries"] / args.steps,
            "tier_queries_per_step": d["flat_filtered_i8_queries"] / args.steps,
        })
        print(json.dumps(cases[-1]), flush=True)

    sweep = []
    m = 256
    while m <= min(args.sweep_max, n):
        mk = ix.make_mask(rng.choice(n, m, replace=False))
        row = {"m": m}
        for leg, mode, dmax in (("tier", 2, 0), ("direct", 1, 8192)):
            ix.set_flat_mode(mode)
            ix.set_param("flat_filtered_direct_max", dmax)
            tf, _, d = legs(mk, args.sweep_steps, 2, with_knn=False)
            row[f"{leg}_step_ms_median"] = float(np.median(tf))
            row[f"{leg}_step_ms_min"] = float(np.min(tf))
            if leg == "tier":
                row["tier_handed_on_per_step"] = d["flat_filtered_fallback_queries"] / args.sweep_steps
                row["tier_ran"] = d["flat_filtered_i8_queries"] > 0
        ix.set_flat_mode(0)
        ix.set_param("flat_filtered_direct_max", 8192)
        mk.close()
        sweep.append(row)
        print(json.dumps(row), flush=True)
        m *= 2
    not_slower = [r["m"] for r in sweep if r["direct_step_ms_median"] <= r["tier_step_ms_median"]]
    rec = {
        "what": "exact filtered Flat k-NN (vdb_flat_knn_filtered_device) vs vdb_flat_knn_device at the same k, same process, alternating legs, "
                "device events; then direct path vs forced tier over m",
        "rows": n, "dim": dim, "nq": nq, "dist": args.dist, "k": k, "steps": args.steps, "warmup": args.warmup, "sweep_steps": args.sweep_steps,
        "cases": cases, "sweep": sweep,
        "largest_m_direct_not_slower": max(not_slower) if not_slower else None,
    }
    print(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
