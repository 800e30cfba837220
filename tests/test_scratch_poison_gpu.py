"""GPU: every entry point under set_param("debug_scratch_poison", word) returns what it returns without it.

Almost every GPU test builds a fresh index, hence a fresh workspace whose buffers come straight from hipMalloc -- very often all zeros, the
one condition under which a counter nobody zeroed, a padding query's threshold nobody wrote, a key slot past the current n or a ragged
tile read before it is written stay invisible.  The aid fills every new DevBuf allocation, and every scratch buffer of the pooled workspace
before each call, with a word; tests/scratch_cases.py holds the case table, the baselines and their CPU references.

Per row: the baseline (an index that made no other call, two identical runs, the CPU reference), then the call on this module's shared
index under each pattern in turn -- 0x00000001 (a small count / id / offset, a denormal), 0xFFFFFFFF (LABEL_NONE / PAIR_NONE, a NaN),
0x7F800000 (+inf as a key) -- bit for bit the baseline, NaN distances by position, and the same counter deltas: a stale threshold that only
sends more queries to the redo path changes no answer, but it changes a counter.

The shared indexes are made by the first row that needs them and closed by this module's finaliser (tests/test_call_history_gpu.py closes
its own), so here they have made no call before the first poisoned one: their lazily built mirrors, masked row constants and workspace
buffers are allocated -- and filled -- under a pattern, as are the mirrors the edits rows grow and re-tile on their disposable index."""
import pytest

import scratch_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vdb():
    import lab_1806_vec_db_amd as vdb
    yield vdb
    sc.close_shared()


@pytest.mark.parametrize("name", [c.name for c in sc.CASES])
def test_poisoned_scratch_changes_nothing(vdb, name):
    case = sc.BY_NAME[name]
    sc.baseline(vdb, case)
    env = sc.shared_env(vdb, case.kind)
    setter = env.ix if env.ix is not None else sc.shared_env(vdb, "small").ix  # (the parameter is process-wide)
    try:
        for word in sc.PATTERNS:
            setter.set_param("debug_scratch_poison", word)
            sc.check(vdb, case, what=f"under pattern {word:#010x}")
    finally:
        setter.set_param("debug_scratch_poison", 0)


def test_the_parameter_takes_a_32_bit_word_only(vdb):
    from lab_1806_vec_db_amd._lib import VdbError
    ix = sc.shared_env(vdb, "small").ix
    for bad in (-1, 1 << 32):
        with pytest.raises(VdbError, match="32-bit pattern"):
            ix.set_param("debug_scratch_poison", bad)
    sc.check(vdb, sc.BY_NAME["knn-small-nq1-k1"], what="after a refused set_param")  # (and it is still off)
