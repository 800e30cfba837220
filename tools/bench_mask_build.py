#!/usr/bin/env python3
"""What it costs to GET a row mask: the host loop over the metadata + vdb_mask_create (the path every mask took before label columns
existed, and still the path of a pattern the columns cannot express) against vdb_mask_create_where / _many over label columns on the
device, same process, same table.

1M x 960 f32 rows (bench data, seed 1806) in a VecDB table; metadata per row: an id, `tenant` (1000 tenants x 1000 rows, row i belongs to
tenant i % 1000) and a two-valued `tier`.  Timed, host clock around calls that end synchronised (every mask call does), median of --reps:
  host_loop / make_mask     the host path for ONE pattern, its two parts separately (_Table.host_match, then GpuIndex.make_mask)
  where_1 / where_2         GpuIndex.make_mask_where for one single-term and one two-term pattern
  where_many                GpuIndex.make_masks_where for all 1000 tenants: wall time, and the three mask kernels' own time
                            (vdb_prof_get "mask_where", from a separate profiled call)
  first_use                 the one-off encode of a key's column (one pass over the metadata + set_labels), per key
  batch_search_cold         VecDB.batch_search, one query per tenant, k = 10, all 1000 tenants, masks dropped by a preceding batch_add: this
                            code; and the host path (a table whose codec may hold no columns: the loop + make_mask per pattern, statement
                            for statement what the parent commit runs) for --host-tenants tenants, since 1000 of them take minutes
Every device-built mask is compared with the host path's mask of the same pattern (words and ids) before anything is timed.
Writes one JSON record (default profiles/mask_build_1M.json)."""
from __future__ import annotations

import argparse
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
    ap.add_argument("--host-tenants", type=int, default=8, help="tenants of the host-path batch_search (each costs a pass over the metadata)")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "mask_build_1M.json"), help="'' = print only")
    args = ap.parse_args()

    import numpy as np
    import torch

    from bench import gist_like_gpu
    from lab_1806_vec_db_amd.labels import LabelCodec
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

    def wall(fn, reps=args.reps):
        ts, out = [], None
        for _ in range(reps):
            t0 = time.perf_counter()
            out = fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return {"ms_median": float(np.median(ts)), "ms_min": float(np.min(ts)), "ms_max": float(np.max(ts)), "reps": reps}, out

    rec = {"what": "cost of building row masks: host loop + vdb_mask_create vs vdb_mask_create_where(_many) over label columns; host clock around "
                   "synchronised calls, same process, same table",
           "rows": n, "dim": dim, "tenants": T, "rows_per_tenant": n // T, "k": k}

    # ---- the host path for one pattern, its two parts
    p1, p2 = {"tenant": "7"}, {"tenant": "7", "tier": "gold"}
    rec["host_loop"], allow1 = wall(lambda: t.host_match(p1), reps=3)
    rec["make_mask"], hm1 = wall(lambda: ix.make_mask(allow1))
    hm2 = ix.make_mask(t.host_match(p2))
    rec["host_path_one_pattern_ms"] = rec["host_loop"]["ms_median"] + rec["make_mask"]["ms_median"]

    # ---- first use of a key: the column's one-off encode
    rec["first_use"] = {}
    for key, pat in (("tenant", p1), ("tier", p2)):
        t0 = time.perf_counter()
        t.create_columns([pat])
        rec["first_use"][key] = {"ms": (time.perf_counter() - t0) * 1e3, "distinct_values": len(t.codec.codes[t.codec.column_of(key)])}
    assert t.codec.keys() == ["tenant", "tier"] and ix.get_stat("label_columns") == 2

    # ---- device-built masks: identical to the host path's before anything is timed
    terms1, terms2 = t.codec.terms(p1), t.codec.terms(p2)
    for terms, hm in ((terms1, hm1), (terms2, hm2)):
        dm = ix.make_mask_where(terms)
        assert all(np.array_equal(a, b) for a, b in zip(dm.rows(), hm.rows())) and len(dm) == len(hm)
        dm.close()
    hm1.close(), hm2.close()

    def single(terms):
        ix.make_mask_where(terms).close()

    single(terms1), single(terms2)  # warm-up
    rec["where_1"], _ = wall(lambda: single(terms1), reps=4 * args.reps)
    rec["where_2"], _ = wall(lambda: single(terms2), reps=4 * args.reps)
    all_terms = [t.codec.terms({"tenant": str(j)}) for j in range(T)]

    def many():
        for mk in ix.make_masks_where(all_terms):
            mk.close()

    many()
    rec["where_many"], _ = wall(many)
    ix.prof_enable(True)
    ix.prof_reset()
    many()
    p = ix.prof_get("mask_where")
    ix.prof_enable(False)
    rec["where_many"]["masks"] = T
    rec["where_many"]["kernels_ms"] = p["ms"]
    rec["where_many"]["kernel_launch_groups"] = p["launches"]
    rec["where_many"]["kernel_gbytes"] = p["bytes"] / 1e9
    rec["where_many"]["kernel_gbps"] = p["bytes"] / (p["ms"] * 1e-3) / 1e9 if p["ms"] else None
    rec["where_many"]["ms_per_mask"] = rec["where_many"]["ms_median"] / T
    rec["host_path_over_where_1"] = rec["host_path_one_pattern_ms"] / rec["where_1"]["ms_median"]
    rec["host_path_over_where_many_per_mask"] = rec["host_path_one_pattern_ms"] / rec["where_many"]["ms_per_mask"]

    # ---- VecDB.batch_search, cold: masks dropped by a batch_add just before
    pats = [{"tenant": str(j)} for j in range(T)]

    def cold(patterns, queries, host_path=False):
        db.batch_add("t", extra, [{"id": "extra", "tenant": "none", "tier": "free"}])
        assert not t.masks
        saved = t.codec
        if host_path:  # no key has or may get a column: every pattern takes the loop + make_mask
            t.codec = LabelCodec(max_columns=0)
        try:
            t0 = time.perf_counter()
            out = db.batch_search("t", queries, k, filters=patterns)
            return (time.perf_counter() - t0) * 1e3, out
        finally:
            t.codec = saved

    cold(pats, qs)  # warm-up (mirrors of the search tiers, code objects)
    ms, got = cold(pats, qs)
    rec["batch_search_cold"] = {"tenants": T, "ms": ms}
    warm0 = time.perf_counter()
    db.batch_search("t", qs, k, filters=pats)
    rec["batch_search_cold"]["warm_ms"] = (time.perf_counter() - warm0) * 1e3
    H = min(args.host_tenants, T)
    ms_h, got_h = cold(pats[:H], qs[:H], host_path=True)
    assert got_h == got[:H]  # same answers from both paths
    rec["batch_search_cold_host_path"] = {"tenants": H, "ms": ms_h, "ms_per_tenant": ms_h / H,
                                          "extrapolated_ms_for_all_tenants": ms_h / H * T,
                                          "note": f"measured for {H} tenants only; the figure for {T} is extrapolated, not measured"}
    rec["mask_where_masks"] = ix.get_stat("mask_where_masks")
    print(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    db.delete_table("t")


if __name__ == "__main__":
    main()
