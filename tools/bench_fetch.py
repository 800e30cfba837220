#!/usr/bin/env python3
"""Bulk row fetch (vdb_index_get_rows / _mask / _device) against the only route the library offered before it -- one vdb_index_row call
per row -- and against the floor of the host form: one plain hipMemcpy of the same byte count from a contiguous device buffer into the
same kind of (pageable, already touched) host memory.

Default bench data (1M x 960 gist-like rows, seed 1806).  Cases: random 0.1 %, 1 % and 10 % of the rows (shuffled order), a 1000-row
mask (get_rows_mask), and all rows ascending (the DIRECT route: one copy, no kernel).  Per case:

  get_rows   : wall time of ONE call (it returns synchronised), median / min / max over the repetitions
  row loop   : vdb_index_row over the same rows, timed IN FULL up to --loop-max rows (10 000) and EXTRAPOLATED linearly beyond, labelled
  memcpy     : hipMemcpy(device -> host) of m x dim x 4 bytes

Then: fetch_chunk_bytes swept over 1 .. 256 MiB on the 10 % case (and on 1 %); the device form over all rows in shuffled order next to
vdb_stream_probe_rows at the same row size in the same run; VecDB.extract_data at --extract-rows rows next to the per-row loop it ran
before (`[(index[i].tolist(), metadata[i]) ...]`, the parent commit's body, evaluated here in the same process).

No test asserts any of these times.  Writes one JSON record (default profiles/fetch_rows_1M.json)."""
from __future__ import annotations

import argparse
import ctypes as C
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop-max", type=int, default=10_000)
    ap.add_argument("--extract-rows", type=int, default=100_000)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "fetch_rows_1M.json"), help="'' = print only")
    args = ap.parse_args()

    import numpy as np
    import torch

    import lab_1806_vec_db_amd as vdb
    from bench import gist_like_gpu
    from lab_1806_vec_db_amd import _lib as L

    dev = torch.device("cuda", 0)
    n, dim = args.rows, args.dim
    row_bytes = dim * 4
    base = gist_like_gpu(torch, n, dim, 1806, dev)
    ix = vdb.GpuIndex(dim, "l2sqr")
    ix.add_device(base.data_ptr(), n)
    default_chunk = vdb.index.FETCH_CHUNK_BYTES_DEFAULT
    rng = np.random.default_rng(1811)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemcpy.restype = C.c_int
    lib = ix._lib

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def summary(ts):
        return {"ms_median": float(np.median(ts)), "ms_min": float(np.min(ts)), "ms_max": float(np.max(ts)), "reps": len(ts)}

    def plain_copy(out, nbytes):
        assert hip.hipMemcpy(out.ctypes.data, base.data_ptr(), nbytes, 2) == 0  # hipMemcpyDeviceToHost

    def row_loop(rows, out):
        f32p = L.f32p
        fn, h = lib.vdb_index_row, ix._h
        for j, r in enumerate(rows):
            fn(h, int(r), out[j].ctypes.data_as(f32p))

    def case(name, rows, call, m):
        out = np.empty((m, dim), dtype=np.float32)
        out.fill(0)  # (touched: no page faults inside the timed calls)
        got = summary([wall(lambda: call(out)) for _ in range(args.reps)])
        assert np.array_equal(out[:: max(1, m // 50)], base[torch.from_numpy(np.asarray(rows[:: max(1, m // 50)], dtype=np.int64)).to(dev)].cpu().numpy())
        floor = summary([wall(lambda: plain_copy(out, m * row_bytes)) for _ in range(args.reps)])
        lm = min(m, args.loop_max)
        loop_ms = float(np.median([wall(lambda: row_loop(rows[:lm], out)) for _ in range(3)]))
        rec = {"case": name, "rows": m, "bytes": m * row_bytes, "get_rows": got, "plain_hipMemcpy": floor,
               "row_loop": {"rows_timed": lm, "ms_timed": loop_ms, "ms_for_all_rows": loop_ms * m / lm,
                            "how": "timed in full" if lm == m else f"EXTRAPOLATED linearly from the first {lm} rows"},
               "GBps_get_rows": m * row_bytes / got["ms_median"] / 1e6, "GBps_plain_hipMemcpy": m * row_bytes / floor["ms_median"] / 1e6}
        rec["row_loop_over_get_rows"] = rec["row_loop"]["ms_for_all_rows"] / got["ms_median"]
        rec["get_rows_over_plain_copy"] = got["ms_median"] / floor["ms_median"]
        print(json.dumps(rec), flush=True)
        return rec

    sets = {f"random {100 * f:g} %": rng.permutation(n)[: int(n * f)] for f in (0.001, 0.01, 0.1)}

    # ---- the chunk size first: the cases below run with the winner ---------------------------------------------------------------------
    sweep = []
    for mb in (1, 2, 4, 8, 16, 32, 64, 128, 256):
        ix.set_param("fetch_chunk_bytes", mb << 20)
        rec = {"chunk_MiB": mb}
        for name in ("random 10 %", "random 1 %"):
            rows = sets[name]
            out = np.empty((len(rows), dim), dtype=np.float32)
            out.fill(0)
            ix.get_rows(rows, out=out)
            rec[name] = summary([wall(lambda: ix.get_rows(rows, out=out)) for _ in range(args.reps)])
        sweep.append(rec)
        print(json.dumps(rec), flush=True)
    best = min(sweep, key=lambda r: r["random 10 %"]["ms_median"])["chunk_MiB"]
    ix.close()
    ix = vdb.GpuIndex(dim, "l2sqr")  # a fresh index: the cases run with the SHIPPED default, whatever the sweep said
    ix.add_device(base.data_ptr(), n)
    lib = ix._lib

    cases = []
    for name, rows in sets.items():
        cases.append(case(name, rows, lambda out, rows=rows: ix.get_rows(rows, out=out), len(rows)))
    allow = np.sort(rng.permutation(n)[:1000])
    mk = ix.make_mask(allow)
    cases.append(case("mask of 1000 rows (get_rows_mask)", allow, lambda out: ix.get_rows_mask(mk, out=out), 1000))
    mk.close()
    every = np.arange(n)
    cases.append(case("all rows ascending (DIRECT)", every, lambda out: ix.get_rows(every, out=out), n))
    stats = {s: ix.get_stat(s) for s in ("fetch_calls", "fetch_rows", "fetch_chunks", "fetch_direct")}

    # ---- the device form's gather against the stream probe -------------------------------------------------------------------------------
    perm = torch.from_numpy(rng.permutation(n).astype(np.int64)).to(dev)
    d_out = torch.zeros((n, dim), dtype=torch.float32, device=dev)
    ix.get_rows_device(perm.data_ptr(), n, d_out.data_ptr())
    assert torch.equal(d_out[::1000], base[perm[::1000]])
    dts = [wall(lambda: ix.get_rows_device(perm.data_ptr(), n, d_out.data_ptr())) for _ in range(args.reps)]
    probe = vdb.index.stream_probe_rows(0, n * row_bytes, 5, row_bytes)
    device = {"what": "get_rows_device over all rows in shuffled order: wall time of the CALL (id check, one flag read-back, one gather launch, "
                      "two stream syncs); GB/s counts the bytes read plus the bytes written; probe = vdb_stream_probe_rows (reads only) at the "
                      "same row size and byte count in the same run",
              "rows": n, "row_bytes": row_bytes, **summary(dts), "GBps_read_plus_write": 2 * n * row_bytes / float(np.median(dts)) / 1e6,
              "GBps_read_only": n * row_bytes / float(np.median(dts)) / 1e6, "stream_probe_rows_GBps": probe}
    print(json.dumps(device), flush=True)
    del d_out, perm
    ix.close()

    # ---- VecDB.extract_data -------------------------------------------------------------------------------------------------------------
    from lab_1806_vec_db_amd.vecdb import VecDB

    ne = min(args.extract_rows, n)
    db = VecDB()
    db.create_table_if_not_exists("t", dim, "l2sqr")
    t = db._tables["t"]
    t.index.add_device(base.data_ptr(), ne)
    t.metadata = [{"id": str(i)} for i in range(ne)]
    after = [wall(lambda: db.extract_data("t")) for _ in range(3)]
    before = [wall(lambda: [(t.index[i].tolist(), dict(t.metadata[i])) for i in range(len(t.index))]) for _ in range(3)]
    extract = {"what": "VecDB.extract_data; 'per_row_loop' is the body the method had before this change (one vdb_index_row call per row), "
                       "evaluated in the same process; both include .tolist() of every row",
               "rows": ne, "extract_data": summary(after), "per_row_loop": summary(before),
               "loop_over_call": float(np.median(before)) / float(np.median(after))}
    print(json.dumps(extract), flush=True)
    db.delete_table("t")

    out = {
        "what": "vdb_index_get_rows* (one call) vs a loop of vdb_index_row calls over the same rows and vs one plain hipMemcpy of the same "
                "bytes into pageable host memory; wall times of calls that return synchronised; medians and ranges over the repetitions of "
                "ONE run; the cases ran with the shipped fetch_chunk_bytes",
        "rows": n, "dim": dim, "row_bytes": row_bytes, "cases": cases, "chunk_sweep": sweep, "chunk_sweep_winner_MiB": best,
        "shipped_fetch_chunk_bytes": default_chunk, "device_form": device, "extract_data": extract, "stats_after_the_cases": stats,
    }
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
