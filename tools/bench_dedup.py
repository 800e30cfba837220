#!/usr/bin/env python3
"""Near-duplicate grouping (vdb_flat_dup_groups_device: a range self-join over the table's own rows + connected components) against
its floor and against the host route it replaces, same process, same table.

--rows x 960 f32 rows (bench data, seed 1806) with planted near-copies: --seeds rows are copied over other rows, every copy perturbed by
0.001 per element (squared distance 960e-6), a third of them as chains (copy k + 1 made from copy k).  radius = 2.5 x that distance.
Host clock around calls that end synchronised; everything from this one run:
  probe        one vdb_flat_range_device call per chunk size (1024, 4096, 16384) over the table's first rows as queries: ms per query
               and which tier answered (flat_range_i8_queries against flat_range_scan_queries) -- are stored rows kept by the 8-bit tier?
  call         vdb_flat_dup_groups_device over the whole table at the shipped chunk, checked against the planted truth
  floor        the loop of vdb_flat_range_device calls over the same chunks of the same rows (results copied to the host and dropped)
  kernels      k_comp_hook / k_comp_flatten between events (vdb_prof_get "dup_hook" / "dup_flatten" of one more call with the profile on)
  sweep        the call at flat_dup_chunk = 1024, 4096, 16384, in --reps interleaved rounds with the call and the floor (medians, ranges)
  host         range_search from Python over get_rows chunks + a numpy union-find, on --host-chunks chunks, EXTRAPOLATED to the table
A full pass over the table costs rows / 1000 x (ms per 1000 queries); --budget-s bounds what is run: when the probe says the passes
wanted do not fit, the sweep and then the floor are measured on the first --prefix-chunks chunks only and the record says so.
Writes one JSON record (default profiles/flat_dup_1M.json)."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RANGE = ("flat_range_queries", "flat_range_i8_queries", "flat_range_scan_queries", "flat_range_results")
SWEEP = (1024, 4096, 16384)
SHIPPED = 16384  # DUP_CHUNK_DEFAULT of csrc/dup_plan.hpp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=960)
    ap.add_argument("--seeds", type=int, default=1000)
    ap.add_argument("--budget-s", type=float, default=600.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--prefix-chunks", type=int, default=4)
    ap.add_argument("--host-chunks", type=int, default=2)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "flat_dup_1M.json"), help="'' = print only")
    args = ap.parse_args()

    import numpy as np
    import torch

    import lab_1806_vec_db_amd as vdb
    from bench import gist_like_gpu

    dev = torch.device("cuda", 0)
    n, dim = args.rows, args.dim
    t_start = time.perf_counter()
    base = gist_like_gpu(torch, n, dim, 1806, dev)
    # planted copies: seed rows and their copies at distinct random places
    rng = np.random.default_rng(1809)
    place = rng.permutation(n)
    truth = np.arange(n, dtype=np.int64)
    at = args.seeds
    eps = 0.001
    for s_at in range(args.seeds):
        members = [int(place[s_at])]
        for _ in range(int(rng.integers(1, 6))):
            c = int(place[at])
            at += 1
            src = members[-1] if s_at % 3 == 0 else members[0]  # a chain: from the copy before; a star: from the seed
            base[c] = base[src] + eps
            members.append(c)
        truth[members] = min(members)
    d_pair = dim * eps * eps
    radius = 2.5 * d_pair  # a chain's rows two apart lie at 4 x d_pair: outside, joined by linkage only
    ix = vdb.GpuIndex(dim, "l2sqr", device=0)
    ix.add_device(base.data_ptr(), n)
    t_r = torch.full((max(SWEEP),), radius, dtype=torch.float32, device=dev)
    out = torch.zeros((n,), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    def wall(fn):
        t0 = time.perf_counter()
        r = fn()
        return (time.perf_counter() - t0) * 1e3, r

    def stats():
        return {s: ix.get_stat(s) for s in RANGE}

    def floor(chunk, n_chunks=None):
        total = -(-n // chunk)
        for c in range(total if n_chunks is None else min(n_chunks, total)):
            a = c * chunk
            nb = min(chunk, n - a)
            ix.range_search_device(base.data_ptr() + a * dim * 4, nb, t_r.data_ptr())

    rec = {"what": "near-duplicate grouping (vdb_flat_dup_groups_device) against the loop of vdb_flat_range_device calls over the same chunks "
                   "of the table's own rows (the floor), the component kernels between events, the chunk sweep and the host route "
                   "(range_search over get_rows chunks + numpy union-find); host clock around synchronised calls, one process, one table, one run",
           "rows": n, "dim": dim, "seeds": args.seeds, "planted_rows": int((truth != np.arange(n)).sum()) + args.seeds, "radius": radius,
           "planted_pair_distance": d_pair, "shipped_chunk": SHIPPED}

    # ---- probe: one range call per chunk size over the first rows (the first call also builds the 8-bit mirror: not timed)
    ix.range_search_device(base.data_ptr(), 64, t_r.data_ptr())
    rec["probe"] = {}
    for chunk in SWEEP:
        nb = min(chunk, n)
        s0 = stats()
        ms, _ = wall(lambda: ix.range_search_device(base.data_ptr(), nb, t_r.data_ptr()))
        s1 = stats()
        rec["probe"][str(chunk)] = {"queries": nb, "ms": ms, "ms_per_1000_queries": ms / nb * 1000,
                                    "i8_queries": s1["flat_range_i8_queries"] - s0["flat_range_i8_queries"],
                                    "scan_queries": s1["flat_range_scan_queries"] - s0["flat_range_scan_queries"]}
    per_q = min(p["ms_per_1000_queries"] for p in rec["probe"].values()) / 1000
    est_pass_s = per_q * n / 1000
    rec["estimated_full_pass_s"] = est_pass_s
    left = lambda: args.budget_s - (time.perf_counter() - t_start)  # noqa: E731

    # ---- the call, once, at the shipped chunk -- when one pass fits at all
    def call():
        return ix.dup_groups_device(radius, out.data_ptr())

    if est_pass_s < 0.6 * left():
        s0 = stats()
        ms, st = wall(call)
        s1 = stats()
        got = out.cpu().numpy()
        rec["call"] = {"ms": ms, "stats": st, "matches_planted_truth": bool(np.array_equal(got, truth)),
                       "range_i8_queries": s1["flat_range_i8_queries"] - s0["flat_range_i8_queries"],
                       "range_scan_queries": s1["flat_range_scan_queries"] - s0["flat_range_scan_queries"],
                       "chunks": -(-n // SHIPPED)}
        assert rec["call"]["matches_planted_truth"], "the groups differ from the planted truth"
    else:
        rec["call"] = {"skipped": "one pass over the table is estimated at %.0f s, beyond the budget" % est_pass_s}

    # ---- floor, kernels, sweep: over the whole table when the passes fit, else over a prefix of chunks of the floor loop
    passes_wanted = 1 + 1 + len(SWEEP)
    full = "ms" in rec["call"] and est_pass_s * passes_wanted < 0.8 * left()
    rec["floor_and_sweep_over"] = "the whole table" if full else "the first %d chunks of each size (floor loop only; the call has no prefix form)" % args.prefix_chunks
    if full:
        # interleaved rounds: the call and the floor at the shipped chunk, then the call at every chunk size of the sweep
        reps = max(1, min(args.reps, int(0.8 * left() / (est_pass_s * (2 + len(SWEEP))))))
        t_call, t_floor, t_sweep = [rec["call"]["ms"]], [], {c: [] for c in SWEEP}
        for r in range(reps):
            if r:
                t_call.append(wall(call)[0])
            t_floor.append(wall(lambda: floor(SHIPPED))[0])
            for chunk in SWEEP:
                ix.set_param("flat_dup_chunk", chunk)
                t_sweep[chunk].append(wall(call)[0])
            ix.set_param("flat_dup_chunk", SHIPPED)
        summ = lambda ts: {"ms_median": float(np.median(ts)), "ms_min": float(np.min(ts)), "ms_max": float(np.max(ts)), "reps": len(ts)}  # noqa: E731
        rec["call"].update(summ(t_call))
        rec["floor"] = summ(t_floor)
        rec["floor"]["call_over_floor"] = rec["call"]["ms_median"] / rec["floor"]["ms_median"]
        rec["sweep"] = {str(c): summ(t_sweep[c]) for c in SWEEP}
        rec["best_chunk"] = int(min(rec["sweep"], key=lambda c: rec["sweep"][c]["ms_median"]))
        ix.prof_enable(True)
        ix.prof_reset()
        ms_p, _ = wall(call)
        hook, flat = ix.prof_get("dup_hook"), ix.prof_get("dup_flatten")
        ix.prof_enable(False)
        rec["kernels_between_events"] = {"dup_hook_ms": hook["ms"], "dup_hook_launches": hook["launches"], "dup_flatten_ms": flat["ms"],
                                         "profiled_call_ms": ms_p, "share_of_call": (hook["ms"] + flat["ms"]) / ms_p}
    else:
        rec["sweep_floor_prefix"] = {}
        for chunk in SWEEP:
            ms_c, _ = wall(lambda: floor(chunk, args.prefix_chunks))
            q = min(n, chunk * args.prefix_chunks)
            rec["sweep_floor_prefix"][str(chunk)] = {"queries": q, "ms": ms_c, "ms_per_1000_queries": ms_c / q * 1000,
                                                     "EXTRAPOLATED_full_pass_s": ms_c / q * n / 1000}
        if "ms" in rec["call"]:
            ix.prof_enable(True)
            ix.prof_reset()
            if est_pass_s < 0.8 * left():
                ms_p, _ = wall(call)
                hook, flat = ix.prof_get("dup_hook"), ix.prof_get("dup_flatten")
                rec["kernels_between_events"] = {"dup_hook_ms": hook["ms"], "dup_hook_launches": hook["launches"], "dup_flatten_ms": flat["ms"],
                                                 "profiled_call_ms": ms_p, "share_of_call": (hook["ms"] + flat["ms"]) / ms_p}
            ix.prof_enable(False)

    # ---- the host route on a few chunks: get_rows + range_search + numpy union-find over the pairs, extrapolated
    def host(n_chunks, chunk=SHIPPED):
        parent = np.arange(n, dtype=np.int64)

        def find(x):
            while parent[x] != x:
                parent[x] = parent[parent[x]]
                x = parent[x]
            return x

        for c in range(n_chunks):
            a = c * chunk
            rows = np.arange(a, min(n, a + chunk), dtype=np.uint64)
            lims, ids, _ = ix.range_search(ix.get_rows(rows), np.float32(radius))
            src = np.repeat(rows, np.diff(lims).astype(np.int64))
            keep = src != ids
            for u, v in zip(src[keep].tolist(), ids[keep].tolist()):
                ru, rv = find(u), find(v)
                if ru != rv:
                    parent[max(ru, rv)] = min(ru, rv)

    hc = min(args.host_chunks, -(-n // SHIPPED))
    ms_h, _ = wall(lambda: host(hc))
    rec["host_route"] = {"chunks_timed": hc, "ms": ms_h, "EXTRAPOLATED_full_table_ms": ms_h / hc * -(-n // SHIPPED)}
    if "ms" in rec["call"]:
        rec["host_route"]["EXTRAPOLATED_over_call"] = rec["host_route"]["EXTRAPOLATED_full_table_ms"] / rec["call"].get("ms_median", rec["call"]["ms"])
    rec["counters"] = {s: ix.get_stat(s) for s in ("flat_dup_calls", "flat_dup_chunks", "flat_dup_pairs") + RANGE}
    rec["wall_s"] = time.perf_counter() - t_start
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    ix.close()


if __name__ == "__main__":
    main()
