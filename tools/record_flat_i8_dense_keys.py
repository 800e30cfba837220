"""Records tests/golden/flat_i8_dense_key_sha256.json: the sha256 of the 8-bit pass's dense keys (flat_shortlist_keys(qs, 2)) for every
case of tests/test_flat_i8_unit_valu_gpu.py.  Run it on an MI355X with the library whose bits are the reference -- the commit BEFORE a
change of k_gemm8.hip that must not move a key bit, built into a directory of its own:

    VDBHIP_LIB=/path/to/parent/libvdbhip.so python3 tools/record_flat_i8_dense_keys.py [--check | --out FILE]

--check writes nothing and compares with the committed file instead (exit status 1 on a difference); --out writes FILE instead of it.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import lab_1806_vec_db_amd as vdb  # noqa: E402
import test_flat_i8_unit_valu_gpu as T  # noqa: E402


def main():
    hashes = {}
    for dim, kcs in T.DENSE_DIMS:
        for metric in T.METRICS:
            hashes.update(T.dense_key_hashes(vdb, dim, metric, kcs))
            print(dim, metric, "done", flush=True)
    if "--check" in sys.argv[1:]:
        with open(T.HASH_FILE) as f:
            want = json.load(f)["sha256"]
        bad = sorted(k for k in set(want) | set(hashes) if want.get(k) != hashes.get(k))
        print("differing cases:", bad if bad else "none")
        sys.exit(1 if bad else 0)
    doc = {"what": "sha256 of flat_shortlist_keys(qs, 2)[0].view(uint32) per case dim_metric_kc_res_epi; inputs: dense_inputs() of "
                   "tests/test_flat_i8_unit_valu_gpu.py (%d rows, %d queries)" % (T.N_ROWS, T.N_QUERIES),
           "sha256": dict(sorted(hashes.items()))}
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv[1:] else T.HASH_FILE
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", out, len(hashes), "cases")


if __name__ == "__main__":
    main()
