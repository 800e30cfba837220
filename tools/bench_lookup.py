#!/usr/bin/env python3
"""The key lookup over one label column (vdb_index_label_lookup) and what VecDB builds on it, against the routes the table had before,
same process, same table.  One run, host clock around calls that end synchronised, medians of --reps (20); nothing here is gated.

1M x 960 f32 rows (bench data, seed 1806) in a VecDB table as tools/bench_mask_partition.py makes it: metadata per row a unique `id`
and a `tenant` (1000 tenants x 1000 rows, row i belongs to tenant i % 1000); both keys have label columns.
  A  label_lookup of 1 000 / 100 000 / 1 000 000 ids (shuffled): the direct route against the sorted route (label_lookup_table_bytes = 0),
     both against label_counts on the same codes, and against make_masks_where for the 1 000 case.  keep_direct = the direct route's
     median at 100 000 codes is below the sorted route's by more than the min-max spread of the two.
  B  _Table.match_rows over G uncached one-key id patterns, G = 2 .. 4096, with the lookup routing on (LOOKUP_MIN = 1) against off
     (None).  lookup_min = the smallest G from which on the routing won at every size of the sweep, never below 64: the value
     vecdb.LOOKUP_MIN ships with (None when there is none).
  C  VecDB.batch_upsert of 10 % of the table, half present and half new (--upsert-reps runs, fresh ids each), against the floor --
     update_rows + batch_add called directly on a twin index with the rows known in advance -- and against the route it replaces,
     batch_update with the routing off, TIMED ON 100 IDS AND EXTRAPOLATED linearly to the present half (stated as such in the record).
Every answer is compared with numpy or with the other route before anything is timed.  Writes one JSON record (default
profiles/label_lookup_1M.json)."""
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
    ap.add_argument("--sizes", type=str, default="1000,100000,1000000")
    ap.add_argument("--groups", type=str, default="2,4,8,16,32,64,128,256,512,1024,2048,4096")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--upsert-reps", type=int, default=3)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "label_lookup_1M.json"), help="'' = print only")
    args = ap.parse_args()

    import numpy as np
    import torch

    from bench import gist_like_gpu
    from lab_1806_vec_db_amd import GpuIndex, vecdb
    from lab_1806_vec_db_amd import _lib as L
    from lab_1806_vec_db_amd.vecdb import VecDB

    dev = torch.device("cuda", 0)
    n, dim, T = args.rows, args.dim, args.tenants
    rng = np.random.default_rng(1806)
    db = VecDB()
    db.create_table_if_not_exists("t", dim, "l2sqr")
    t = db._tables["t"]
    ix = t.index
    base = gist_like_gpu(torch, n, dim, 1806, dev)
    ix.add_device(base.data_ptr(), n)  # (the rows go in from the device: a host copy of 3.84 GB is no part of what is measured)
    t.metadata = [{"id": str(i), "tenant": str(i % T)} for i in range(n)]
    t.create_columns([{"id": "0", "tenant": "0"}])
    col = t.codec.column_of("id")
    id_col = ix.get_labels(col)

    def wall(fn, reps=args.reps):
        ts, out = [], None
        for _ in range(reps):
            t0 = time.perf_counter()
            out = fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return {"ms_median": float(np.median(ts)), "ms_min": float(np.min(ts)), "ms_max": float(np.max(ts)), "reps": reps}, out

    def note(msg):  # progress on stderr: the run takes minutes and prints its record only at the end
        print(f"[bench_lookup] {msg}", file=sys.stderr, flush=True)

    note("table ready")
    rec = {"what": "vdb_index_label_lookup (direct / sorted route) vs vdb_index_label_counts and vdb_mask_create_where_many on the same codes; "
                   "_Table.match_rows with the lookup routing on / off; VecDB.batch_upsert vs update_rows + batch_add with known rows and vs "
                   "batch_update extrapolated from 100 ids; host clock around synchronised calls, same process, same table, one run",
           "rows": n, "dim": dim, "tenants": T}

    # ---- A: the primitive
    rec["label_lookup"] = {}
    for m in [min(int(s), n) for s in args.sizes.split(",")]:
        codes = np.ascontiguousarray(id_col[rng.permutation(n)[:m]], dtype=np.uint32)
        want_first = np.empty(n, dtype=np.uint64)
        want_first[id_col] = np.arange(n, dtype=np.uint64)  # (a unique column: code -> its one row)
        counts64 = np.zeros(m, dtype=np.uint64)
        e = {}
        for name, cap in (("direct", 64 << 20), ("sorted", 0)):
            ix.set_param("label_lookup_table_bytes", cap)
            e[name + "_plan"] = dict(zip(("route", "base", "span", "chunks"), GpuIndex.label_lookup_plan(col, codes, cap)))
            first, counts = ix.label_lookup(col, codes)
            assert np.array_equal(first, want_first[codes]) and (counts == 1).all()
            e[name], _ = wall(lambda: ix.label_lookup(col, codes))
        ix.set_param("label_lookup_table_bytes", 64 << 20)

        def run_counts():
            L.check(ix._lib.vdb_index_label_counts(ix._h, col, None, codes.ctypes.data_as(L.u32p), m, counts64.ctypes.data_as(L.u64p)))

        run_counts()
        assert (counts64 == 1).all()
        e["label_counts"], _ = wall(run_counts)
        if m <= 1000:
            terms = [[(col, int(c))] for c in codes]

            def run_where():
                for mk in ix.make_masks_where(terms):
                    mk.close()

            run_where()
            e["make_masks_where"], _ = wall(run_where)
        e["sorted_over_direct"] = e["sorted"]["ms_median"] / e["direct"]["ms_median"]
        rec["label_lookup"][str(m)] = e
        note(f"A: {m} codes done")
    at = rec["label_lookup"].get("100000")
    if at is not None:
        spread = (at["direct"]["ms_max"] - at["direct"]["ms_min"]) + (at["sorted"]["ms_max"] - at["sorted"]["ms_min"])  # of the two, added
        rec["keep_direct"] = {"direct_ms": at["direct"]["ms_median"], "sorted_ms": at["sorted"]["ms_median"], "min_max_spread_ms": spread,
                              "keep": at["sorted"]["ms_median"] - at["direct"]["ms_median"] > spread}

    # ---- B: match_rows, the routing on against off
    rec["match_rows"] = {}
    saved = vecdb.LOOKUP_MIN
    wins = {}
    try:
        for G in [int(g) for g in args.groups.split(",")]:
            pats = [{"id": str(int(i))} for i in rng.permutation(n)[:G]]
            e, answers = {}, {}
            for name, lm in (("routing_off", None), ("routing_on", 1)):
                vecdb.LOOKUP_MIN = lm
                answers[name] = [r.tolist() for r in t.match_rows(pats)]
                e[name], _ = wall(lambda: t.match_rows(pats))
            assert answers["routing_on"] == answers["routing_off"] == [[int(p["id"])] for p in pats]
            e["off_over_on"] = e["routing_off"]["ms_median"] / e["routing_on"]["ms_median"]
            wins[G] = e["routing_on"]["ms_median"] < e["routing_off"]["ms_median"]
            rec["match_rows"][str(G)] = e
            note(f"B: group of {G} done")
    finally:
        vecdb.LOOKUP_MIN = saved
    lookup_min = None
    for G in sorted(wins, reverse=True):
        if not wins[G]:
            break
        lookup_min = G
    rec["lookup_min"] = None if lookup_min is None else max(lookup_min, 64)
    rec["lookup_min_shipped"] = saved

    # ---- C: batch_upsert of 10 % of the table against the floor and against the route it replaces
    half = n // 20
    twin = GpuIndex(dim, "l2sqr")
    twin.add_device(base.data_ptr(), n)
    del base
    fresh = gist_like_gpu(torch, 2 * half, dim, 1811, dev).cpu().numpy()
    ups, floors = [], []
    for rep in range(args.upsert_reps):
        present = rng.permutation(n)[:half]
        metas = [{"id": str(int(i)), "tenant": str(int(i) % T)} for i in present] + [{"id": f"new{rep}_{j}", "tenant": str(j % T)} for j in range(half)]
        t0 = time.perf_counter()
        got = db.batch_upsert("t", "id", fresh, metas)
        ups.append((time.perf_counter() - t0) * 1e3)
        assert got == (half, half)
        t0 = time.perf_counter()
        twin.update_rows(present.astype(np.uint64), fresh[:half])
        twin.batch_add(fresh[half:])
        floors.append((time.perf_counter() - t0) * 1e3)
        note(f"C: upsert {rep} done")
    assert len(ix) == len(twin) == n + args.upsert_reps * half
    probe = np.concatenate([present[:50], np.arange(len(ix) - 50, len(ix))]).astype(np.uint64)
    assert np.array_equal(ix.get_rows(probe), twin.get_rows(probe))
    vecdb.LOOKUP_MIN = None
    try:
        pats = [{"id": str(int(i))} for i in rng.permutation(n)[:100]]
        old, _ = wall(lambda: db.batch_update("t", pats, fresh[:100]))
    finally:
        vecdb.LOOKUP_MIN = saved
    rec["batch_upsert"] = {
        "entries": 2 * half, "present": half, "new": half, "reps": args.upsert_reps,
        "upsert_ms": {"median": float(np.median(ups)), "min": float(np.min(ups)), "max": float(np.max(ups))},
        "floor_update_rows_plus_batch_add_ms": {"median": float(np.median(floors)), "min": float(np.min(floors)), "max": float(np.max(floors))},
        "batch_update_100_ids_routing_off": old,
        "replaced_route_extrapolated_ms": old["ms_median"] * half / 100,
        "extrapolation": "batch_update of 100 ids with LOOKUP_MIN = None, scaled linearly to the present half; the batch_add of the new half is not in it",
    }
    rec["stats"] = {s: ix.get_stat(s) for s in ("label_lookup_calls", "label_lookup_codes", "label_lookup_direct", "label_lookup_passes",
                                                "label_count_calls", "mask_where_masks")}
    print(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    twin.close()
    db.delete_table("t")


if __name__ == "__main__":
    main()
