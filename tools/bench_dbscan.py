#!/usr/bin/env python3
"""Density clustering (vdb_flat_dbscan_device: the range self-join over the table's own rows + core test, core components, border rows)
against its floor, vdb_flat_dup_groups_device at the same radius in the same run: that call runs the same range join over the same
chunks and a lane-per-pair hook behind it.  The expectation is a ratio near 1, because the join dominates.

Shape: --rows x --dim (default 1M x 960) gist-like rows, of which --blobs x --blob-rows are planted dense blobs (a seed row plus
Gaussian copies of it, sigma 0.001 per coordinate: pairs inside a blob lie at about 2 dim sigma^2, the radius is twice that); every other
row is scattered.  At min_samples = blob-rows / 2 every blob row is core, so the answer is checked against the planted truth: one cluster
per blob, named by its lowest row, everything else noise.

One call each with the profile off, wall time around synchronised calls after one untimed warm-up range call (it builds the 8-bit
mirror); then one further call each with the profile on for the kernels between events (prof_get "dbscan_link" = k_dbscan_core +
k_dbscan_link, "dbscan_labels") and their share of the timed call.  Not measured: Cosine, masks, u8 rows, very dense neighbourhoods
(lists of thousands of rows), other chunk sizes.  Nothing is gated on these numbers.  Writes --out as JSON."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RANGE = ("flat_range_queries", "flat_range_i8_queries", "flat_range_scan_queries", "flat_range_results")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=960)
    ap.add_argument("--blobs", type=int, default=1000)
    ap.add_argument("--blob-rows", type=int, default=16)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "flat_dbscan_1M.json"), help="'' = print only")
    args = ap.parse_args()

    import numpy as np
    import torch

    import lab_1806_vec_db_amd as vdb
    from bench import gist_like_gpu

    dev = torch.device("cuda", 0)
    n, dim, sigma = args.rows, args.dim, 0.001
    base = gist_like_gpu(torch, n, dim, 1806, dev)
    place = np.random.default_rng(1811).permutation(n)[: args.blobs * args.blob_rows].reshape(args.blobs, args.blob_rows)
    gen = torch.Generator(device=dev).manual_seed(1812)
    for members in place:  # row 0 of a blob is its seed
        t = torch.from_numpy(members[1:]).to(dev)
        base[t] = base[int(members[0])] + sigma * torch.randn((len(members) - 1, dim), generator=gen, device=dev)
    truth = np.full(n, 2 ** 64 - 2, dtype=np.uint64)
    truth[place] = place.min(axis=1, keepdims=True).astype(np.uint64)
    radius, min_samples = 4.0 * dim * sigma * sigma, args.blob_rows // 2
    ix = vdb.GpuIndex(dim, "l2sqr", device=0)
    ix.add_device(base.data_ptr(), n)
    label = torch.zeros((n,), dtype=torch.int64, device=dev)
    kind = torch.zeros((n,), dtype=torch.uint8, device=dev)
    t_r = torch.full((64,), radius, dtype=torch.float32, device=dev)
    ix.range_search_device(base.data_ptr(), 64, t_r.data_ptr())  # warm-up
    torch.cuda.synchronize()

    def timed(fn):
        s0 = {s: ix.get_stat(s) for s in RANGE}
        t0 = time.perf_counter()
        st = fn()
        ms = (time.perf_counter() - t0) * 1e3
        return ms, st, {s: ix.get_stat(s) - s0[s] for s in RANGE}

    def kernel_ms(fn, names):  # a further call with the profile on: its event records stay out of the wall times above
        ix.prof_enable(True)
        ix.prof_reset()
        fn()
        out = {k: ix.prof_get(k)["ms"] for k in names}
        ix.prof_enable(False)
        return out

    dup = lambda: ix.dup_groups_device(radius, label.data_ptr())  # noqa: E731
    dbs = lambda: ix.dbscan_device(radius, min_samples, label.data_ptr(), kind.data_ptr())  # noqa: E731
    floor_ms, floor_st, floor_range = timed(dup)
    ms, st, rng_st = timed(dbs)
    hook = kernel_ms(dup, ("dup_hook", "dup_flatten"))
    prof = kernel_ms(dbs, ("dbscan_link", "dbscan_labels"))
    ok = bool(np.array_equal(label.cpu().numpy().view(np.uint64), truth))
    rec = {"what": "density clustering (vdb_flat_dbscan_device) against vdb_flat_dup_groups_device at the same radius in the same run (the "
                   "floor: the same range self-join); host clock around synchronised calls, one process, one table, one call each",
           "rows": n, "dim": dim, "blobs": args.blobs, "blob_rows": args.blob_rows, "sigma": sigma, "radius": radius,
           "min_samples": min_samples, "chunk": 16384,  # DUP_CHUNK_DEFAULT of csrc/dup_plan.hpp
           "dbscan": {"ms": ms, "stats": st, "range": rng_st, "kernels_ms": prof, "kernels_share": sum(prof.values()) / ms,
                      "matches_planted_truth": ok},
           "floor_dup_groups": {"ms": floor_ms, "stats": floor_st, "range": floor_range, "kernels_ms": hook},
           "ratio_to_floor": ms / floor_ms,
           "not_measured": ["Cosine", "masks", "u8 rows", "very dense neighbourhoods", "other chunk sizes", "repeat runs"]}
    print(json.dumps(rec), flush=True)
    assert ok, "the labels differ from the planted truth"
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    ix.close()


if __name__ == "__main__":
    main()
