"""GPU: the keys of the native 8-bit pass of a u8 table (k_gemm_u8.hip) are LOWER BOUNDS of the reference's distances -- the f32 fold of
the widened elements (oracle.dist_u8) -- for every (row, query) pair, and for L2Sqr they ARE the distances while dim * 255^2 < 2^24
(docs/DESIGN_flat.md 4.1af).  Dense keys through flat_shortlist_keys, tier 3.  48: a partial k-block; 272: the first multiple of 16
whose all-0 against all-255 sum passes 2^24; 960: fifteen k-blocks, sums near 2^26."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DIMS = [16, 48, 64, 128, 272, 960]


@pytest.mark.parametrize("dist,kind", [("l2sqr", 0), ("cosine", 1)])
@pytest.mark.parametrize("dim", DIMS)
def test_dense_keys_are_lower_bounds(dim, dist, kind):
    import lab_1806_vec_db_amd as vdb
    from oracle import oracle as O

    rng = np.random.default_rng(dim)
    rows = rng.integers(0, 256, (101, dim), dtype=np.uint8)  # 101: two full units and a partial one
    qs = rng.integers(0, 256, (8, dim), dtype=np.uint8)
    alt = np.tile(np.array([0, 255], dtype=np.uint8), dim // 2)
    rows[3], rows[50], rows[99], rows[100] = 0, 255, alt, qs[5]
    qs[0], qs[1], qs[2] = 0, 255, alt
    ix = vdb.GpuIndex(dim, dist, scalar="u8")
    ix.set_param("flat_u8", 2)  # (before the rows: forced, the add builds no fp16 mirror)
    ix.batch_add_u8(rows)
    keys = ix.flat_shortlist_keys(qs.astype(np.float32), 3)[0]
    assert keys.shape == (8, 101) and not np.isnan(keys).any()
    ref = np.array([[np.float32(O.dist_u8(kind, r, q)) for r in rows] for q in qs], dtype=np.float32)
    print(dim, dist, "largest reference - key:", float((ref - keys).max()))
    assert (keys <= ref).all(), np.argwhere(keys > ref)[:4]
    if kind == 0 and dim * 255 * 255 < 2 ** 24:
        assert np.array_equal(keys, ref)
    assert ix.get_stat("flat_u8_valid") == 1 and ix.get_stat("flat_half_valid") == 0 and ix.get_stat("flat_bf16_mirror") == 0
