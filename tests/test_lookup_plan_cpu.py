"""CPU: vdb_label_lookup_plan (host utility, no GPU) against a Python restatement.

A key lookup over n_codes distinct codes is carried out on the DIRECT route (a table slot_of[code - base] of span u32, one read of the
column) when n_codes > 1024 and 4 B x span <= table_bytes, where base / span run over the codes other than LABEL_NONE, and on the
SORTED route otherwise, in ceil(n_codes / 1024) reads.  Checked: 0, 1, 1024 and 1025 codes; a span at the cap and one entry above it;
LABEL_NONE alone and among others; codes 0 and 0xFFFFFFFE together; every refusal, which leaves the outputs untouched."""
import ctypes as C

import numpy as np
import pytest

SORTED, DIRECT = 0, 1
NONE = 0xFFFFFFFF
CHUNK = 1024
MIB64 = 64 << 20
FILL = 2**63 + 5


@pytest.fixture(scope="module")
def lib():
    from lab_1806_vec_db_amd import _lib as L

    return L, L.load()


def _call(lib, column, codes, table_bytes, n_codes=None):
    L, so = lib
    c = None if codes is None else np.ascontiguousarray(codes, dtype=np.uint32)
    n = (0 if c is None else c.size) if n_codes is None else n_codes
    route, base, span, chunks = C.c_int(77), C.c_uint32(77), C.c_uint64(FILL), C.c_uint64(FILL)
    st = so.vdb_label_lookup_plan(column, None if c is None or c.size == 0 else c.ctypes.data_as(L.u32p), n, table_bytes, C.byref(route), C.byref(base),
                                  C.byref(span), C.byref(chunks))
    return st, (route.value, base.value, span.value, chunks.value)


def _want(codes, table_bytes):
    real = [int(c) for c in codes if int(c) != NONE]
    base = min(real) if real else 0
    span = max(real) - base + 1 if real else 0
    n = len(codes)
    direct = n > CHUNK and span >= 1 and 4 * span <= table_bytes
    return (DIRECT if direct else SORTED), base, span, (0 if n == 0 else 1 if direct else -(-n // CHUNK))


def _ok(lib, codes, table_bytes=MIB64):
    st, got = _call(lib, 3, codes, table_bytes)
    assert st == 0, lib[1].vdb_last_error()
    assert got == _want(codes, table_bytes), (len(codes), table_bytes)
    assert lib[1].vdb_label_lookup_plan(3, np.ascontiguousarray(codes, dtype=np.uint32).ctypes.data_as(lib[0].u32p) if len(codes) else None, len(codes), table_bytes,
                                        None, None, None, None) == 0  # nothing asked for
    return got


def test_sizes(lib):
    rng = np.random.default_rng(1)
    assert _ok(lib, []) == (SORTED, 0, 0, 0)
    assert _ok(lib, [7]) == (SORTED, 7, 1, 1)
    assert _ok(lib, rng.permutation(CHUNK) + 5) == (SORTED, 5, CHUNK, 1)
    assert _ok(lib, rng.permutation(CHUNK + 1) + 5) == (DIRECT, 5, CHUNK + 1, 1)
    assert _ok(lib, rng.permutation(CHUNK + 1) + 5, 0) == (SORTED, 5, CHUNK + 1, 2)  # table_bytes = 0: never direct
    assert _ok(lib, rng.permutation(3000)) == (DIRECT, 0, 3000, 1)
    assert _ok(lib, rng.permutation(3000), 0) == (SORTED, 0, 3000, 3)
    sparse = rng.choice(2**31, size=2049, replace=False)
    assert _ok(lib, sparse)[0] == SORTED and _ok(lib, sparse)[3] == 3  # a span far over the cap


def test_span_at_the_cap(lib):
    n = 1500
    for cap in (4 * 5000, 4 * 5000 + 3):
        at = np.concatenate([np.arange(n - 1), [4999]]) + 100  # span = 5000: 4 B x span == 4 x 5000
        assert _ok(lib, at, cap) == (DIRECT, 100, 5000, 1)
        over = np.concatenate([np.arange(n - 1), [5000]]) + 100  # one entry above it
        assert _ok(lib, over, cap) == (SORTED, 100, 5001, 2)
    assert _ok(lib, np.arange(n), 4 * n - 1) == (SORTED, 0, n, 2)
    assert _ok(lib, np.arange(n), 4 * n) == (DIRECT, 0, n, 1)


def test_label_none_is_not_counted_into_the_span(lib):
    assert _ok(lib, [NONE]) == (SORTED, 0, 0, 1)
    assert _ok(lib, [9, NONE, 4]) == (SORTED, 4, 6, 1)
    many = np.concatenate([np.arange(10, 1500), [NONE]]).astype(np.uint64)
    np.random.default_rng(2).shuffle(many)
    assert _ok(lib, many) == (DIRECT, 10, 1490, 1)
    assert _ok(lib, many, 4 * 1490 - 1) == (SORTED, 10, 1490, 2)


def test_span_past_32_bits_of_bytes_is_sorted(lib):
    assert _ok(lib, [0, 0xFFFFFFFE]) == (SORTED, 0, 0xFFFFFFFF, 1)
    wide = np.concatenate([np.arange(1, 1100), [0, 0xFFFFFFFE]])  # 4 B x span = 2^34 - 4: over 64 MiB, and over 32 bits
    assert _ok(lib, wide) == (SORTED, 0, 0xFFFFFFFF, 2)
    assert _ok(lib, wide, 2**32 - 1) == (SORTED, 0, 0xFFFFFFFF, 2)  # (a product taken in 32 bits would wrap to a small one)
    assert _ok(lib, wide, 2**34) == (DIRECT, 0, 0xFFFFFFFF, 1)
    assert _ok(lib, np.concatenate([wide, [NONE]])) == (SORTED, 0, 0xFFFFFFFF, 2)


def test_refusals_leave_the_outputs_untouched(lib):
    untouched = (77, 77, FILL, FILL)
    dup_far = np.arange(2000)
    dup_far[1999] = 3  # a duplicate in a dense list
    dup_sparse = [5, 2**31, 9, 2**31]  # ... and in a sparse one
    for column, codes, n_codes in ((16, [1, 2], None), (2**32 - 1, [], None), (0, [4, 4], None), (0, [NONE, 1, NONE], None), (0, dup_far, None),
                                   (0, dup_sparse, None), (0, None, 3), (0, [1], 1 << 28)):
        st, got = _call(lib, column, codes, MIB64, n_codes)
        assert st == 1 and got == untouched, (column, n_codes)
        assert lib[1].vdb_last_error()
    st, _ = _call(lib, 0, [4, 4], MIB64)
    assert b"4" in lib[1].vdb_last_error() and b"twice" in lib[1].vdb_last_error()
    st, got = _call(lib, 15, None, MIB64, 0)  # no codes: no pointer is needed
    assert st == 0 and got == (SORTED, 0, 0, 0)
