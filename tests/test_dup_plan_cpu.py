"""CPU: vdb_dup_plan (host utility, no GPU; csrc/dup_plan.hpp) against a Python restatement.

The near-duplicate grouping walks its m allowed rows (all n rows without a mask) as queries, `chunk` per range call: ceil(m / chunk)
calls, the last of m - (calls - 1) x chunk queries.  The queries are gathered into a buffer of min(chunk, m) x dim f32 under a mask or on
a u8 index and used in place otherwise; besides that buffer the call holds 8 B per row of the table (parent, sizes), the chunk's radii
(4 B each) and limits (8 B each, one more than queries) and 64 B of counters.  Checked: chunk boundaries, m = 0 and 1, every route,
every refusal (a NaN radius, a chunk of 0 or past 2^20, more allowed rows than rows, 2^32 rows), which leaves the outputs untouched;
+-inf and negative radii and any limit are accepted."""
import ctypes as C
import math

import pytest

FILL = 2**63 + 5


@pytest.fixture(scope="module")
def lib():
    from lab_1806_vec_db_amd import _lib as L

    return L.load()


def _call(so, n, dim, u8, masked, m, radius, limit, chunk):
    chunks, last, gather, scratch = C.c_uint64(FILL), C.c_uint64(FILL), C.c_int(77), C.c_uint64(FILL)
    st = so.vdb_dup_plan(n, dim, int(u8), int(masked), m, radius, limit, chunk, C.byref(chunks), C.byref(last), C.byref(gather), C.byref(scratch))
    return st, (chunks.value, last.value, gather.value, scratch.value)


def _want(n, dim, u8, masked, m, chunk):
    calls = -(-m // chunk)
    last = m - (calls - 1) * chunk if m else 0
    gather = bool(masked or u8)
    ql = min(chunk, m)
    scratch = 8 * n + 4 * ql + 8 * (ql + 1) + 64 + (ql * dim * 4 if gather else 0)
    return calls, last, int(gather), scratch


@pytest.mark.parametrize("u8", (False, True))
@pytest.mark.parametrize("masked", (False, True))
def test_layout_against_the_restatement(lib, u8, masked):
    for n in (0, 1, 2, 63, 64, 65, 300, 4096, 4097, 20000, 1_000_000, 2**32 - 1):
        for chunk in (1, 2, 64, 4096, 16384, 2**20):
            for m in sorted({0, min(1, n), n // 2, max(n - 1, 0), n}) if masked else (n,):
                st, got = _call(lib, n, 960, u8, masked, m, 0.5, 0, chunk)
                assert st == 0 and got == _want(n, 960, u8, masked, m, chunk), (n, chunk, m, got)
    # five chunks with a ragged last one
    assert _call(lib, 300, 5, u8, masked, 300, 0.0, 8, 64)[1][:2] == (5, 44)


def test_radii_and_limits_that_are_accepted(lib):
    for r in (0.0, -1.0, math.inf, -math.inf, 1e-45, 3.4e38):
        for limit in (0, 1, 8, 2**40):
            st, got = _call(lib, 1000, 8, False, False, 1000, r, limit, 4096)
            assert st == 0 and got == _want(1000, 8, False, False, 1000, 4096)


def test_refusals_leave_the_outputs_alone(lib):
    from lab_1806_vec_db_amd import _lib as L

    untouched = (FILL, FILL, 77, FILL)
    bad = [
        (1000, 8, False, False, 1000, math.nan, 0, 4096, "NaN"),
        (1000, 8, False, False, 1000, 0.5, 0, 0, "flat_dup_chunk"),
        (1000, 8, False, False, 1000, 0.5, 0, 2**20 + 1, "flat_dup_chunk"),
        (1000, 8, False, True, 1001, 0.5, 0, 4096, "allowed rows"),
        (1000, 8, False, False, 999, 0.5, 0, 4096, "allowed rows"),
        (2**32, 8, False, False, 2**32, 0.5, 0, 4096, "2^32"),
    ]
    for *args, word in bad:
        st, got = _call(lib, *args)
        assert st == 1 and got == untouched, args
        assert word in lib.vdb_last_error().decode(), (word, lib.vdb_last_error())
    # NULL outputs are allowed
    assert lib.vdb_dup_plan(10, 4, 0, 0, 10, 0.5, 0, 4, None, None, None, None) == 0
    assert L.load() is lib


def test_python_wrapper(lib):
    import lab_1806_vec_db_amd as vdb

    assert vdb.GpuIndex.dup_plan(300, 5, 0.1, chunk=64) == (5, 44, False, _want(300, 5, False, False, 300, 64)[3])
    assert vdb.GpuIndex.dup_plan(300, 5, 0.1, m_allowed=100, chunk=64) == (2, 36, True, _want(300, 5, False, True, 100, 64)[3])
    assert vdb.GpuIndex.dup_plan(300, 5, 0.1, elem_u8=True)[2] is True
    with pytest.raises(vdb.VdbError):
        vdb.GpuIndex.dup_plan(300, 5, float("nan"))
