"""Flat k-NN over a u8 table: the native 8-bit pass ("flat_u8" = 2, k_gemm_u8.hip) against the routing without it ("flat_u8" = 1: the fp16 /
split-bf16 mirrors) in ONE process on ONE box, steps alternating between the two.  1M x 128 and 1M x 960 rows, both metrics, k = 10, 1000
integer queries.  Per setting: the median step time (host clock around the synchronous call), resident HBM bytes per row, and for the
new pass the filter kernel's time between device events (a run of its own with the library's event timing on) and flat_u8_redo.  Answers of
the two settings are compared bit for bit.  Needs a GPU; writes profiles/flat_u8_1M.json.

    python tools/bench_u8.py [--rows 1000000] [--steps 20] [--warmup 3] [--out profiles/flat_u8_1M.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lab_1806_vec_db_amd as vdb  # noqa: E402


def run_shape(n, dim, dist, steps, warmup, nq=1000, k=10):
    rng = np.random.default_rng(dim)
    qs = rng.integers(0, 256, (nq, dim), dtype=np.uint8)
    ix = {}
    for name, mode in (("native", 2), ("parent", 1)):
        ix[name] = vdb.GpuIndex(dim, dist, scalar="u8")
        ix[name].set_param("flat_u8", mode)
        for r0 in range(0, n, 250000):  # same rows in both: the generator is re-seeded per chunk
            ix[name].batch_add_u8(np.random.default_rng([dim, r0]).integers(0, 256, (min(250000, n - r0), dim), dtype=np.uint8))
    ans = {name: x.flat_knn_u8(qs, k) for name, x in ix.items()}
    same = all(np.array_equal(a, b) for a, b in zip(ans["native"], ans["parent"]))
    times = {name: [] for name in ix}
    for step in range(warmup + steps):
        for name, x in ix.items():  # alternating: both settings see the same neighbours on the box
            t0 = time.perf_counter()
            x.flat_knn_u8(qs, k)
            if step >= warmup:
                times[name].append((time.perf_counter() - t0) * 1e3)
    ix["native"].prof_enable(True)
    ix["native"].prof_reset()
    for _ in range(steps):
        ix["native"].flat_knn_u8(qs, k)
    filt = ix["native"].prof_get("flat_u8")
    med = {name: statistics.median(t) for name, t in times.items()}
    out = {"rows": n, "dim": dim, "dist": dist, "nq": nq, "k": k, "steps": steps, "same_answers": bool(same),
           "native_ms_median": med["native"], "parent_ms_median": med["parent"], "parent_over_native": med["parent"] / med["native"],
           "native_ms_min_max": [min(times["native"]), max(times["native"])], "parent_ms_min_max": [min(times["parent"]), max(times["parent"])],
           "filter_kernel_ms_per_step": filt["ms"] / max(1, filt["launches"]), "filter_bytes_per_step": filt["bytes"] / max(1, filt["launches"]),
           "native_hbm_bytes_per_row": ix["native"].get_stat("hbm_bytes_per_row"), "parent_hbm_bytes_per_row": ix["parent"].get_stat("hbm_bytes_per_row"),
           "flat_u8_queries": ix["native"].get_stat("flat_u8_queries"), "flat_u8_redo": ix["native"].get_stat("flat_u8_redo")}
    for x in ix.values():
        x.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="profiles/flat_u8_1M.json")
    a = ap.parse_args()
    res = []
    for dim in (128, 960):
        for dist in ("l2sqr", "cosine"):
            res.append(run_shape(a.rows, dim, dist, a.steps, a.warmup))
            print(json.dumps(res[-1]), flush=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/bench_u8.py", "results": res}, f, indent=1)


if __name__ == "__main__":
    main()
