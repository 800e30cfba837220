"""CPU: vdb_pca_plan / vdb_pca_segment (host only; csrc/pca_plan.hpp) against layouts worked out by hand, the segments' cover of [0, m), and
every refusal that is a property of the arguments."""
import ctypes as C

import pytest

import lab_1806_vec_db_amd as vdb
from lab_1806_vec_db_amd import _lib as L

FILL = 2**63 + 5
# (n, dim, u8, masked, m, center, project, n_comp, w_dim) -> (dim_pad, blocks = b (b + 1) / 2, R, seg_rows, scratch = 8 (4096 R blocks + 1025 dim_pad))
# R: slices = ceil(m / 16), want = ceil(1024 / blocks), per = max(ceil(slices / want), 4), seg_rows = 16 per, R = ceil(slices / per)
CASES = (
    ((2, 1, 0, 0, 2, 1, 0, 0, 0), (64, 1, 1, 64, 8 * (4096 + 1025 * 64))),
    ((65, 70, 0, 0, 65, 1, 0, 0, 0), (128, 3, 2, 64, 8 * (2 * 3 * 4096 + 1025 * 128))),
    ((5000, 130, 0, 1, 1000, 0, 0, 0, 0), (192, 6, 16, 64, 8 * (16 * 6 * 4096 + 1025 * 192))),
    ((1000000, 960, 0, 0, 1000000, 1, 0, 0, 0), (960, 120, 9, 16 * 6945, 8 * (9 * 120 * 4096 + 1025 * 960))),
    ((100000, 2048, 0, 0, 100000, 1, 0, 0, 0), (2048, 528, 2, 50000, 8 * (2 * 528 * 4096 + 1025 * 2048))),
    ((9, 70, 0, 1, 0, 1, 1, 70, 70), (128, 3, 1, 64, 8 * (3 * 4096 + 1025 * 128))),  # a projection of no rows onto dim components is accepted
    ((100, 8, 1, 0, 100, 1, 0, 0, 0), "f32 rows"), ((100, 8, 1, 0, 100, 1, 1, 2, 8), "f32 rows"),
    ((100, 8, 0, 1, 1, 1, 0, 0, 0), "at least 2 rows"), ((100, 8, 0, 1, 0, 0, 0, 0, 0), "at least 1 rows"),
    ((100, 2049, 0, 0, 100, 1, 0, 0, 0), "1 .. 2048"), ((100, 2049, 0, 0, 100, 1, 1, 3, 2049), "1 .. 2048"),
    ((100, 8, 0, 0, 99, 1, 0, 0, 0), "allowed rows"), ((100, 8, 0, 1, 101, 1, 0, 0, 0), "allowed rows"),
    ((100, 8, 0, 0, 100, 1, 1, 0, 8), "n_comp = 0"), ((100, 8, 0, 0, 100, 1, 1, 9, 8), "9 components of 8"),
    ((100, 2000, 0, 0, 100, 1, 1, 1025, 2000), "more than 1024"), ((100, 8, 0, 0, 100, 1, 1, 2, 9), "dimension mismatch"))


@pytest.mark.parametrize("args,want", CASES, ids=[str(w) for _, w in CASES])
def test_plan_and_refusals(args, want):
    out = [C.c_uint64(FILL) for _ in range(5)]
    st = L.load().vdb_pca_plan(*args, *(C.byref(o) for o in out))
    if isinstance(want, str):  # a refusal leaves the outputs alone
        assert st == 1 and all(o.value == FILL for o in out) and want in L.load().vdb_last_error().decode()
        return
    assert st == 0 and tuple(o.value for o in out) == want
    n, dim, u8, masked, m, center, project, n_comp, w_dim = args
    assert vdb.GpuIndex.pca_plan(n, dim, m if masked else None, bool(u8), bool(center), n_comp if project else None, w_dim if project else None) == want
    if not project:  # the R segments cover [0, m) exactly once, in order, none empty
        at = 0
        for s in range(want[2]):
            first, ln = vdb.GpuIndex.pca_segment(m, dim, s)
            assert first == at and 1 <= ln <= want[3]
            at += ln
        assert at == m
        with pytest.raises(vdb.VdbError, match="s must be below"):
            vdb.GpuIndex.pca_segment(m, dim, want[2])
