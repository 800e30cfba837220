"""CPU: vdb_rescore_groups_plan (csrc/rescore_plan.hpp, no GPU needed) -- every refusal code of the exact rescoring of candidate documents
in the order the header states, and the layout (tiles of 64 candidate rows, questions per sub-chunk under a scratch budget, scratch bytes)
for hand-written cases."""
import pytest

from lab_1806_vec_db_amd import GpuIndex

OK = [0, 2, 5]  # two questions: 2 and 3 sub-queries
U64 = (1 << 64) - 1


@pytest.mark.parametrize("code,kw", [
    (0, {}), (0, dict(mode="min")), (0, dict(k=8)), (0, dict(ld=4096, k=4096)), (0, dict(lims=[0, 32])), (0, dict(column=15)),
    (0, dict(cand_count=[8, 0])), (0, dict(lims=[0])),
    (1, dict(mode="rrf")), (1, dict(mode=3)), (1, dict(mode="nonsense", column=99)),           # a bad mode comes first
    (2, dict(column=16)), (2, dict(column=0xFFFFFFFF, lims=[1, 2])),
    (3, dict(lims=[])), (4, dict(lims=[1, 2])), (5, dict(lims=[0, 3, 2, 4])), (6, dict(lims=[0, 2, 2, 5])),
    (7, dict(lims=[0, 33])), (7, dict(lims=[0, 5, U64])),
    (8, dict(ld=4097, k=4097)), (9, dict(k=9)), (9, dict(k=1, ld=0)),
    (10, dict(cand_count=[8, 9])), (9, dict(k=9, cand_count=[9, 9])),                          # k > ld is reported before a count
])
def test_refusal_codes(code, kw):
    a = dict(lims=OK, k=4, ld=8, mode="sum", column=0)
    a.update(kw)
    assert GpuIndex.rescore_groups_plan(**a) == (code, None, None, None)


@pytest.mark.parametrize("kw,expect", [
    # question 0: 1 row, 1 group, S = 2 -> 64 x 8 + 1 x 2 x 8 = 528 B; question 1: 130 rows, 3 groups, S = 3 -> 192 x 8 + 3 x 3 x 8 = 1608 B
    (dict(rows=[1, 130], slots=[1, 3]), (4, 2, 2136)),
    (dict(rows=[1, 130], slots=[1, 3], budget=3216), (4, 2, 2136)),
    (dict(rows=[1, 130], slots=[1, 3], budget=3215), (4, 1, 1608)),
    (dict(rows=[1, 130], slots=[1, 3], budget=1), (4, 1, 1608)),                 # at least one question per sub-chunk
    (dict(rows=[64, 65], slots=[1, 1]), (3, 2, 64 * 8 + 16 + 128 * 8 + 24)),     # a group that ends at / passes a tile boundary
    (dict(rows=[0, 0], slots=[0, 0]), (0, 2, 0)),                                # no candidates: no tile, no scratch
    (dict(rows=[1, 130], cand_count=[2, 4]), (4, 2, 512 + 32 + 1536 + 96)),      # no slots: the counts stand for them ...
    (dict(rows=[1, 130]), (4, 2, 512 + 8 * 2 * 8 + 1536 + 8 * 3 * 8)),           # ... or ld
    # three questions of 520, 520, 5128 B: the largest bounds the sub-chunk, the largest sub-chunk the scratch
    (dict(lims=[0, 1, 2, 3], rows=[64, 64, 640], slots=[1, 1, 1], budget=2 * 5128), (12, 2, 5128)),
    (dict(lims=[0, 1, 2, 3], rows=[64, 64, 640], slots=[1, 1, 1], budget=3 * 5128), (12, 3, 6168)),
])
def test_layout(kw, expect):
    assert GpuIndex.rescore_groups_plan(**{"lims": OK, "k": 4, "ld": 8, **kw}) == (0,) + expect
