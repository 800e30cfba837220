"""GPU: the exact late-interaction rescoring (GpuIndex.rescore_groups / rescore_groups_device; csrc/k_rescore.hip, csrc/flat_rescore.hip,
csrc/rescore_plan.hpp) past the one shape of tests/test_flat_rescore_gpu.py (575 rows, ld = 16, four questions, S in 1, 4, 5, 32, dims
1, 3, 4, 33, 130).  The pair distances are the CPU oracle's (oracle.flat_knn_batch at k = n), the rule is tests/rescore_ref.py, and the
criterion is equality of bits -- counts, ids and scores (NaN scores compare as one NaN), "sum" and "min", the host form, the device form,
the device form twice, and flat_rescore_calls / _questions / _rows moving by exactly (1, questions, rows evaluated).

What each test reaches that the older file does not (the six gaps; the scratch-poison and call-history rows of rescoring are in
tests/scratch_cases.py):

  test_every_sub_query_count    k_rescore_pairs.  na = ceil((S - wave) / 4) picks the fold variant per wave; S = 1 .. 32 in ONE call gives
                                every na of every wave: rs_fold<4> at S = 9 .. 16 with accumulators past S folding a zero panel row,
                                rs_fold<8> at S = 17 .. 31 with 1 to 3 dead accumulators, waves of one workgroup on different variants
                                (S = 13: 4, 3, 3, 3).  dim 32 and 64: the last slice is a full one and the tail loop does not run; 33: a
                                full slice and a tail of 1; 960: thirty slices.  Masks per sub-query leave (group, s) pairs without a row
                                at every S.
  test_long_candidate_lists     k_rescore_slots and k_rescore_finish at ld = 4096.  Rounds 2 .. 16 of the slot walk (slot numbers carried
                                in `base`, counts 255 / 256 / 257 around the first round's end), the 96 KiB dynamic LDS table above the
                                default limit, first occurrences in shuffled order so that slot numbers differ from list positions; the
                                bitonic network with several compare-exchange pairs per thread (np > 512): ns = 4096 exactly (no padding
                                key), ns = 2049 (padded to 4096), k = ld = 4096.
  test_probe_chains             the LDS dedupe table and the call-wide (question, code) table, both probed from the hash of the code
                                alone: 40 codes on one slot of each, codes on the last two slots of each (the chain wraps to slot 0), one
                                code wanted by all 300 questions (a chain of 300 in the call-wide table), the codes 0, 0x80000000 and
                                0xFFFFFFFE, and rows whose code no question wants.
  test_three_sub_chunks         the sub-chunk loop of flat_rescore.hip: c0 != 0 in k_rescore_prepare / k_rescore_match<true> /
                                k_rescore_finish, ent_off / tab_off counted from each sub-chunk's start, item0, the q0 .. q1 window of
                                the match kernel.  LIST_BUDGET is 256 MiB and nothing lowers it; the rule worst question x sub_chunk
                                <= budget is reached through the shape (see the test).
  test_order_key_edges          +inf as a real minimum next to a group without an allowed row, +inf + NaN in the fold, the 1e-10 clamp
                                of a zero row and a zero sub-query under cosine, negative cosine distances (they order before +0).

Seconds on an MI355X, host clock per test with its CPU reference, one run: test_every_sub_query_count 0.16 to 0.19 per dim,
test_long_candidate_lists 0.40, test_probe_chains 0.53, test_three_sub_chunks 0.63, test_order_key_edges 0.02 (the first GPU test of a
process pays the start-up of the device on top, 1.3 s here); 3.6 s for the file.  The yardstick, one parametrisation of
test_flat_rescore_gpu.py::test_both_forms_against_the_reference in the same run: 0.03 to 0.05."""
import numpy as np
import pytest

import rescore_ref

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
STATS = ("flat_rescore_calls", "flat_rescore_questions", "flat_rescore_rows")
METRICS = (("l2sqr", 0), ("cosine", 1))


def _dense(base, qs, kind):
    """dm[sub-query][row]: the oracle's distances, every row of every sub-query"""
    from oracle import oracle as O

    n = len(base)
    oi, od, oc = O.flat_knn_batch(base, qs, n, kind, nthreads=16)
    assert (oc == n).all()
    dm = np.zeros((len(qs), n), np.float32)
    np.put_along_axis(dm, oi.astype(np.int64), od, axis=1)
    return dm


def _index(base, dist, labels, column=0):
    import lab_1806_vec_db_amd as vdb

    ix = vdb.GpuIndex(base.shape[1], dist)
    ix.batch_add(base)
    if labels is not None:
        ix.set_labels(column, labels)
    return ix


def _canon(b):
    return np.where((b & 0x7FFFFFFF) > 0x7F800000, np.uint32(0x7FC00000), b)  # (NaN scores compare as one NaN)


def _same(got, exp, what):
    assert np.array_equal(got[2], exp[2]), (what, np.flatnonzero(got[2] != exp[2])[:8])
    assert got[0].dtype == np.uint64 and np.array_equal(got[0], exp[0]), (what, np.argwhere(got[0] != exp[0])[:8])
    bits = _canon(np.ascontiguousarray(got[1]).view(np.uint32))
    assert got[1].dtype == np.float32 and np.array_equal(bits, _canon(exp[1])), (what, np.argwhere(bits != _canon(exp[1]))[:8])


def _cut(exp, k):
    """the reference answer at a smaller k: the order does not depend on k"""
    return np.ascontiguousarray(exp[0][:, :k]), np.ascontiguousarray(exp[1][:, :k]), np.minimum(exp[2], np.uint64(k)), exp[3]


def _device(ix, qs, lims, cand, cnt, k, column, mode, **kw):
    import torch

    nq, ld = len(lims) - 1, cand.shape[1]
    tq = torch.from_numpy(np.ascontiguousarray(qs)).cuda()
    tci, tcc = torch.from_numpy(np.ascontiguousarray(cand).view(np.int64)).cuda(), torch.from_numpy(cnt.view(np.int64)).cuda()
    ti = torch.full((nq, k), -7, dtype=torch.int64, device="cuda")
    td = torch.full((nq, k), -7.0, dtype=torch.float32, device="cuda")
    tc = torch.full((nq,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    try:
        ix.rescore_groups_device(tq.data_ptr(), lims, tci.data_ptr(), tcc.data_ptr(), ld, k, column, ti.data_ptr(), td.data_ptr(), tc.data_ptr(),
                                 mode=mode, **kw)
    finally:
        torch.cuda.synchronize()
    return ti.cpu().numpy().view(np.uint64), td.cpu().numpy(), tc.cpu().numpy().view(np.uint64)


def _all_forms(ix, qs, lims, cand, cnt, k, column, mode, exp, what, device=True, **kw):
    """the host form == exp with the counters moved by exactly (1, questions, rows evaluated); the device form == the host form, twice"""
    s0 = {s: ix.get_stat(s) for s in STATS}
    host = ix.rescore_groups(qs, lims, cand, cnt, k, column, mode, **kw)
    _same(host, exp, what)
    assert {s: ix.get_stat(s) - v for s, v in s0.items()} == dict(zip(STATS, (1, len(lims) - 1, exp[3]))), what
    if device:
        dev = _device(ix, qs, lims, cand, cnt, k, column, mode, **kw)
        again = _device(ix, qs, lims, cand, cnt, k, column, mode, **kw)
        for a, b, c in zip(host, dev, again):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(b.view(np.uint32), c.view(np.uint32)), what
    return host


# ---- a. every sub-query count ------------------------------------------------------------------------------------------------------------
def _labels_a():
    lab = np.concatenate([np.full(c, v) for v, c in ((10, 1), (11, 63), (12, 64), (13, 65), (14, 150), (NONE, 21))]
                         + [100 + np.arange(60) // 6]).astype(np.uint32)
    return lab[np.random.default_rng(17).permutation(len(lab))]


@pytest.mark.parametrize("dim", (32, 64, 33, 960))
def test_every_sub_query_count(dim):
    """k_rescore_pairs: 32 questions of S = 1, 2, .., 32 sub-queries (528) in one call, over 424 rows whose groups hold 1, 63, 64, 65 and
    150 rows (a group ends at, starts at and spans a tile), ten of 6 and 21 unlabelled rows.  Every question's candidates are a shuffle of
    one row of each large group, a second row of the 63 (a duplicate group), three unlabelled rows and five small groups, so each
    question has 6 tiles and every wave of them takes the variant its S gives it.  In the masked call the first sub-query of EVERY
    question hides the whole group of 64 (S = 1: no allowed row at all, the candidate represents it) and every third sub-query hides
    every third row."""
    lab = _labels_a()
    n, rng = len(lab), np.random.default_rng(500 + dim)
    rows_of = {int(v): np.flatnonzero(lab == v) for v in np.unique(lab)}
    base = rng.random((n, dim)).astype(np.float32)
    lims = np.concatenate([[0], np.cumsum(np.arange(1, 33))]).astype(np.uint64)
    qs = rng.random((int(lims[-1]), dim)).astype(np.float32)
    qs[7] = base[rows_of[13][2]]  # a sub-query equal to a stored row
    pool = np.array([rows_of[10][0], rows_of[11][0], rows_of[11][40], rows_of[12][5], rows_of[13][64], rows_of[14][149], rows_of[NONE][0],
                     rows_of[NONE][7], rows_of[NONE][20], rows_of[100][3], rows_of[101][0], rows_of[103][5], rows_of[105][1], rows_of[109][2]])
    cand = np.zeros((32, 16), dtype=np.uint64)
    for q in range(32):
        cand[q, :len(pool)] = rng.permutation(pool)
    cnt = np.full(32, len(pool), dtype=np.uint64)
    hide, third = np.ones(n, dtype=np.bool_), np.arange(n) % 3 != 0
    hide[rows_of[12]] = False
    allows = [hide, np.ones(n, dtype=np.bool_), third]
    mo = (1 + np.arange(int(lims[-1])) % 2).astype(np.uint32)
    mo[lims[:-1].astype(np.int64)] = 0
    groups = rescore_ref.Groups(lab)
    for dist, kind in METRICS:
        dm = _dense(base, qs, kind)
        ix = _index(base, dist, lab)
        try:
            ix.prof_enable(True)
            masks = [ix.make_mask(a) for a in allows]
            for mode in ("sum", "min"):
                exp = rescore_ref.expect(dm, groups, lims, cand, cnt, 16, mode)
                assert (exp[2] == 13).all()
                _all_forms(ix, qs, lims, cand, cnt, 16, 0, mode, exp, f"dim {dim} {dist} {mode}")
                exp = rescore_ref.expect(dm, groups, lims, cand, cnt, 16, mode, allows=allows, mask_of=mo)
                if mode == "sum":  # the group of 64 has a sub-query without an allowed row in every question
                    assert np.isinf(exp[1].view(np.float32)).any(axis=1).all()
                _all_forms(ix, qs, lims, cand, cnt, 16, 0, mode, exp, f"dim {dim} {dist} {mode} masks", masks=masks, mask_of=mo)
            assert ix.prof_get("rescore_pairs")["launches"] >= 12, "the pairs kernel answered"
        finally:
            ix.close()


# ---- b. long candidate lists ---------------------------------------------------------------------------------------------------------------
def test_long_candidate_lists():
    """k_rescore_slots / k_rescore_finish at ld = 4096 (a 2^13-entry, 96 KiB LDS table).  6500 rows x dim 8: 1200 groups of 1, 2, 3 rows
    (2400 rows) and 4100 unlabelled rows, shuffled.  Nine questions of S = 2 in one call:
      0 .. 6  0, 1, 255, 256, 257, 2048 and 4096 candidates drawn WITH replacement from all rows: one round of 256 threads exactly, one
              more candidate, 8 and 16 rounds; the same row and the same group come back at random positions, so the slots assigned in
              round 2 and later are not the list positions;
      7       4096 candidates in which 2047 groups occur twice and 2 once: the 1200 labelled groups (a group of 2 or 3 as two DIFFERENT
              rows, a group of 1 as the same row twice) and 849 unlabelled rows (the same row twice), shuffled: ns = 2049, the sort pads
              to 4096;
      8       4096 distinct unlabelled rows: ns = 4096, no padding key.
    k = 4096 = ld, and k = 3 in a second call."""
    rng = np.random.default_rng(4096)
    sizes = 1 + np.arange(1200) % 3
    lab = np.concatenate([np.repeat(np.arange(1200) + 7, sizes), np.full(4100, NONE)]).astype(np.uint32)
    lab = lab[rng.permutation(len(lab))]
    n, ld = len(lab), 4096
    assert n == 6500
    unl = np.flatnonzero(lab == NONE)
    base = rng.random((n, 8)).astype(np.float32)
    base[unl[:40]] = base[unl[0]]  # identical rows: equal scores, ordered by the representative
    lims = (2 * np.arange(10)).astype(np.uint64)
    qs = rng.random((18, 8)).astype(np.float32)
    cand, cnt = np.zeros((9, ld), dtype=np.uint64), np.array([0, 1, 255, 256, 257, 2048, 4096, 4096, 4096], dtype=np.uint64)
    for q in range(7):
        cand[q, :int(cnt[q])] = rng.integers(0, n, int(cnt[q]))
    twice = np.concatenate([[np.flatnonzero(lab == code)[[0, -1]] for code in range(7, 1207)]]).ravel()  # 1200 groups, 2400 candidates
    cand[7] = np.concatenate([twice, np.repeat(unl[100:947], 2), unl[947:949]])[rng.permutation(ld)]   # + 847 rows twice + 2 once
    cand[8] = rng.permutation(unl)[:ld]
    groups = rescore_ref.Groups(lab)
    for dist, kind in METRICS:
        dm = _dense(base, qs, kind)
        ix = _index(base, dist, lab)
        try:
            for mode in ("sum", "min"):
                exp = rescore_ref.expect(dm, groups, lims, cand, cnt, ld, mode)
                assert exp[2][7] == 2049 and exp[2][8] == 4096 and exp[2][3] < 256 and exp[2][6] < 4096 and exp[2][:2].tolist() == [0, 1]
                _all_forms(ix, qs, lims, cand, cnt, ld, 0, mode, exp, f"{dist} {mode} k=4096")
                _all_forms(ix, qs, lims, cand, cnt, 3, 0, mode, _cut(exp, 3), f"{dist} {mode} k=3", device=False)
        finally:
            ix.close()


# ---- c. the probe chains -------------------------------------------------------------------------------------------------------------------
def _table_lg(x):
    """rescore_table_lg of csrc/rescore_plan.hpp: 2^lg entries, load at most 1/2 (the LDS table: x = min(ld, 4096); the call-wide table:
    x = the sum of the call's candidate counts)"""
    lg = 6
    while (1 << lg) < 2 * x:
        lg += 1
    return lg


def _slot(code, lg):
    """rs_hash of csrc/k_rescore.hip: the first slot a code probes in a table of 2^lg entries"""
    return ((np.asarray(code, dtype=np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - lg)


def test_probe_chains():
    """300 questions x 48 candidates, ld = 64: the LDS table has 2^7 slots, the call-wide one 2^15 (14 400 counted candidates).  Codes:
      P        the popular one, 200 rows (four tiles), on slot 2^15 - 2 of the call-wide table: every question wants it, so its chain
               is 300 long and wraps to slot 0;
      L[40]    on ONE slot of the LDS table, G[40] on ONE slot of the call-wide table (not P's), one or two rows each: every question
               wants its own random 14 of L and 10 of G;
      WL, WG   three codes each on the last and the last-but-one slot of the LDS / the call-wide table, wanted together by every third
               question: their chains wrap;
      0, 0x80000000, 0xFFFFFFFE  (the last is the largest code there is: 0xFFFFFFFF is "no label");
      U[60]    on the slots of G, of P and of WG, wanted by NO question: the match pass walks the chains and must take none of their rows.
    The rest of a question's 48 are unlabelled rows and repeats."""
    rng = np.random.default_rng(77)
    nq, per, ld = 300, 48, 64
    llg, glg = _table_lg(ld), _table_lg(nq * per)
    assert (llg, glg) == (7, 15)
    scan = np.arange(1, 1 << 23, dtype=np.uint64)
    ls, gs = _slot(scan, llg), _slot(scan, glg)
    on_g = lambda slot, m: scan[gs == slot][:m]  # noqa: E731
    P = on_g((1 << glg) - 2, 1)
    G = on_g(12345, 40)
    L = scan[(ls == 77) & (gs != 12345)][:40]
    WL = np.concatenate([scan[ls == (1 << llg) - 1][:3], scan[ls == (1 << llg) - 2][:3]])
    WG = np.concatenate([on_g((1 << glg) - 1, 3), on_g((1 << glg) - 2, 4)[1:]])
    SP = np.array([0, 0x80000000, 0xFFFFFFFE], dtype=np.uint64)
    U = np.concatenate([on_g(12345, 60)[40:], on_g((1 << glg) - 2, 24)[4:], on_g((1 << glg) - 1, 23)[3:]])
    assert len(G) == 40 and len(L) == 40 and len(U) == 60 and len(WG) == 6 and len(WL) == 6
    assert (_slot(L, llg) == 77).all() and (_slot(G, glg) == 12345).all() and _slot(P, glg)[0] == (1 << glg) - 2
    assert sorted(_slot(WL, llg).tolist()) == [126] * 3 + [127] * 3 and sorted(_slot(WG, glg).tolist()) == [32766] * 3 + [32767] * 3
    wanted = np.concatenate([P, L, G, WL, WG, SP])
    assert len(set(wanted.tolist()) | set(U.tolist())) == len(wanted) + len(U), "every code once"
    lab = np.concatenate([np.repeat(P, 200), np.repeat(L, 1 + np.arange(40) % 2), np.repeat(G, 1 + np.arange(40) % 2), np.repeat(WL, 2),
                          np.repeat(WG, 2), np.repeat(SP, 3), np.repeat(U, 2), np.full(120, NONE)]).astype(np.uint32)
    lab = lab[rng.permutation(len(lab))]
    n = len(lab)
    row_of = {int(c): np.flatnonzero(lab == c) for c in np.unique(lab)}
    unl = row_of[NONE]
    base = rng.standard_normal((n, 4)).astype(np.float32)
    S = 1 + np.arange(nq) % 2
    lims = np.concatenate([[0], np.cumsum(S)]).astype(np.uint64)
    qs = rng.standard_normal((int(lims[-1]), 4)).astype(np.float32)
    cand = np.zeros((nq, ld), dtype=np.uint64)
    pick = lambda codes: [int(rng.choice(row_of[int(c)])) for c in codes]  # noqa: E731  (any row of the group stands for it)
    for q in range(nq):
        mine = pick(P) + pick(rng.permutation(L)[:14]) + pick(rng.permutation(G)[:10])
        if q % 3 == 0:
            mine += pick(WL) + pick(WG)
        if q % 5 == 0:
            mine += pick(SP)
        mine += rng.choice(unl, 6, replace=False).tolist()
        mine += rng.choice(mine, per - len(mine)).tolist()  # repeats
        cand[q, :per] = rng.permutation(mine)
    cnt = np.full(nq, per, dtype=np.uint64)
    groups = rescore_ref.Groups(lab)
    for dist, kind in METRICS:
        dm = _dense(base, qs, kind)
        ix = _index(base, dist, lab, column=5)
        try:
            for mode in ("sum", "min"):
                exp = rescore_ref.expect(dm, groups, lims, cand, cnt, ld, mode)
                assert exp[3] < nq * (200 + 2 * (per - 1)), "no row of an unwanted code is counted"
                _all_forms(ix, qs, lims, cand, cnt, ld, 5, mode, exp, f"{dist} {mode}")
        finally:
            ix.close()


# ---- d. sub-chunks -------------------------------------------------------------------------------------------------------------------------
def test_three_sub_chunks():
    """The sub-chunk loop of flat_rescore.hip.  4096 rows x dim 4: ONE group of 4000 rows, 24 groups of 3 and 24 unlabelled rows.  A
    question that wants the large group costs 63 tiles x 64 entries x 8 B + slots x S x 8 B, about 32 KiB, so the 256 MiB budget holds
    about 8270 of them, and 16 650 questions are two full sub-chunks and a short remainder (GpuIndex.rescore_groups_plan, asked with the
    reference's own rows and slots, says how many; nothing here spells the number out).  The questions are heterogeneous so that ent_off,
    tab_off and item0 are not multiples of one number: S cycles over 1, 2, 3; every seventh question wants small groups and an unlabelled
    row only (one tile); a few have no candidates; the largest (the large group and six others, S = 3) is not the first.  Six candidate
    patterns x six sub-query sets drawn from 8 vectors: the reference computes each pair once and the expected arrays are assembled by
    indexing.  Then the questions at each sub-chunk's first and last index, called alone, and the remainder as a call of its own, return
    the bits they have in the batch.

    This is the shape kept: 0.63 s on the MI355X for the three calls in all forms, far below the ten seconds allowed, so the alternative
    (a group of 20 000 rows, about 1675 questions per sub-chunk) was not measured."""
    import lab_1806_vec_db_amd as vdb

    rng = np.random.default_rng(16650)
    n, dim, ld, nq = 4096, 4, 8, 16650
    lab = np.concatenate([np.full(4000, 9), 100 + np.arange(72) // 3, np.full(24, NONE)]).astype(np.uint32)
    lab = lab[rng.permutation(n)]
    big, unl = np.flatnonzero(lab == 9), np.flatnonzero(lab == NONE)
    small = [np.flatnonzero(lab == 100 + g) for g in range(24)]
    base = rng.standard_normal((n, dim)).astype(np.float32)
    vecs = rng.standard_normal((8, dim)).astype(np.float32)
    sets = [(0,), (1, 2), (3, 4, 5), (6,), (7, 0), (2, 5, 7)]  # index = (q % 3) + 3 * (q // 3 % 2): S cycles 1, 2, 3
    pats = [[big[5]], [small[0][1], big[0], big[3999], unl[0]], [unl[1], small[1][0], small[2][2], big[77], small[1][2], unl[2], small[3][0], small[4][1]],
            [small[5][0], unl[3], small[6][1]], [], [big[1000], unl[4], unl[5]]]
    # pattern 2: the large group and six others (8 candidates, 7 groups) -- with S = 3 the largest question; pattern 3: one tile; 4: none
    pat_of = np.where(np.arange(nq) % 7 == 3, 3, np.where(np.arange(nq) % 1999 == 5, 4, np.array([0, 1, 2, 5])[np.arange(nq) % 4]))
    set_of = np.arange(nq) % 3 + 3 * (np.arange(nq) // 3 % 2)
    assert not (pat_of[0] == 2 and set_of[0] % 3 == 2) and ((pat_of == 2) & (set_of % 3 == 2)).any() and (pat_of == 4).sum() >= 3
    S = np.array([len(sets[t]) for t in set_of])
    lims = np.concatenate([[0], np.cumsum(S)]).astype(np.uint64)
    qs = vecs[np.concatenate([sets[t] for t in set_of])]
    cand, cnt = np.zeros((nq, ld), dtype=np.uint64), np.array([len(pats[p]) for p in pat_of], dtype=np.uint64)
    for p, rows in enumerate(pats):
        cand[pat_of == p, :len(rows)] = np.array(rows, dtype=np.uint64)
    groups = rescore_ref.Groups(lab)

    def expected(kind, mode):
        dm = _dense(base, vecs, kind)
        ans = {(p, t): rescore_ref.question(dm[list(sets[t])], groups, pats[p], ld, mode) for p in range(len(pats)) for t in range(len(sets))}
        idx, bits, count, rows = np.zeros((nq, ld), np.uint64), np.zeros((nq, ld), np.uint32), np.zeros(nq, np.uint64), np.zeros(nq, np.uint64)
        for (p, t), (ids, scores, r) in ans.items():
            at = (pat_of == p) & (set_of == t)
            idx[at, :len(ids)], bits[at, :len(ids)], count[at], rows[at] = ids, scores.view(np.uint32), len(ids), r
        return idx, bits, count, rows

    sub = None
    for dist, kind, modes in (("l2sqr", 0, ("sum", "min")), ("cosine", 1, ("sum",))):
        ix = _index(base, dist, lab)
        try:
            for mode in modes:
                idx, bits, count, rows = expected(kind, mode)
                code, tiles, sub, scratch = vdb.GpuIndex.rescore_groups_plan(lims, ld, ld, mode, rows=rows, slots=count)  # (k = ld: count = slots)
                assert code == 0 and tiles == int(((rows + 63) // 64).sum())
                chunks = [min(sub, nq - c0) for c0 in range(0, nq, sub)]
                assert len(chunks) >= 3 and chunks[-1] < chunks[0] and scratch <= 256 << 20, (sub, chunks)
                exp = (idx, bits, count, int(rows.sum()))
                host = _all_forms(ix, qs, lims, cand, cnt, ld, 0, mode, exp, f"{dist} {mode}")

                def alone(a, b):
                    la, lb = int(lims[a]), int(lims[b])
                    got = ix.rescore_groups(qs[la:lb], lims[a:b + 1] - lims[a], cand[a:b], cnt[a:b], ld, 0, mode)
                    for x, y in zip(got, host):
                        assert np.array_equal(x.view(np.uint32), y[a:b].view(np.uint32)), (dist, mode, a, b)
                for c0 in range(0, nq, sub):
                    last = min(nq, c0 + sub) - 1
                    alone(c0, c0 + 1)
                    alone(last, last + 1)
                alone((len(chunks) - 1) * sub, nq)  # the remainder as a call of its own
        finally:
            ix.close()


# ---- e. the edges of the order key -----------------------------------------------------------------------------------------------------------
def test_order_key_edges():
    """L2Sqr over coordinates of 3e38: squared differences overflow to +inf, so +inf is a REAL minimum (group 1: every row of it is +inf
    away from sub-query 0) next to a group that has no allowed row (group 2 under the mask): both score +inf under SUM and under MIN and
    the representatives decide -- the nearest row of the one, the candidate of the other.  A sub-query with a NaN coordinate puts
    +inf + NaN, and NaN + +inf, into the fold.  Cosine: a zero row and a zero sub-query (the 1e-10 clamp: distance 1 to everything),
    and sub-queries that are copies of stored rows, among which the oracle's table holds NEGATIVE distances (dot / (|a| |b|) rounds above
    1) and exact zeros: the negative keys order before +0."""
    B = np.float32(3e38)
    base = np.array([[B, B, 0], [B, 0, B], [-B, -B, 0], [-B, 0, 0], [1, 2, 3], [0, 0, 0], [B, B, B], [3, 2, 1], [-1, 0, 1], [np.nan, 0, 0]], dtype=np.float32)
    lab = np.array([1, 1, 2, 2, 3, 3, 1, NONE, NONE, 4], dtype=np.uint32)
    qs = np.array([[-B, -B, 0], [1, 1, 1], [np.nan, 1, 1], [-B, -B, 0], [B, B, B], [0, 0, 0], [np.nan, 0, 0], [-B, -B, 0]], dtype=np.float32)
    lims = np.array([0, 1, 3, 5, 6, 8], dtype=np.uint64)  # (far) | (plain, NaN) | (far, far the other way) | (zero) | (NaN, far)
    cand = np.tile(np.array([1, 3, 4, 7, 0, 9, 8, 2], dtype=np.uint64), (5, 1))
    cnt = np.array([8, 8, 8, 8, 8], dtype=np.uint64)
    n = len(base)
    allows = [np.ones(n, dtype=np.bool_), np.array([1, 1, 0, 0, 1, 1, 1, 1, 1, 1], dtype=np.bool_)]  # mask 1 hides group 2
    mo = np.array([1, 0, 0, 1, 0, 0, 0, 1], dtype=np.uint32)
    dm = _dense(base, qs, 0)
    assert np.isposinf(dm[0, [0, 1, 6]]).all() and np.isnan(dm[2]).all() and np.isposinf(dm).any() and np.isfinite(dm).any()
    ix = _index(base, "l2sqr", lab)
    try:
        masks = [ix.make_mask(a) for a in allows]
        for mode in ("sum", "min"):
            for k in (8, 2):
                exp = rescore_ref.expect(dm, lab, lims, cand, cnt, k, mode, allows=allows, mask_of=mo)
                _all_forms(ix, qs, lims, cand, cnt, k, 0, mode, exp, f"l2sqr {mode} k={k} masks", masks=masks, mask_of=mo)
                _all_forms(ix, qs, lims, cand, cnt, k, 0, mode, rescore_ref.expect(dm, lab, lims, cand, cnt, k, mode), f"l2sqr {mode} k={k}")
            # question 0: group 1's real +inf (its lowest row, 0, represents it) and group 2 without a row (its candidate, 3, does)
            exp = rescore_ref.expect(dm, lab, lims, cand, cnt, 8, mode, allows=allows, mask_of=mo)
            both = {int(i): int(b) for i, b in zip(exp[0][0, :6], exp[1][0, :6])}
            assert both[0] == 0x7F800000 and both[3] == 0x7F800000 and list(exp[0][0]).index(0) < list(exp[0][0]).index(3)
            if mode == "sum":
                assert exp[2][1] == 6 and (exp[1][[1, 4], :6] == 0x7FC00000).all()  # finite + NaN, +inf + NaN, NaN + +inf
    finally:
        ix.close()

    from oracle import oracle as O

    rng = np.random.default_rng(2)
    base = rng.standard_normal((96, 8)).astype(np.float32)
    base[40] = 0.0
    lab = np.where(np.arange(96) % 9 == 0, NONE, np.arange(96) // 4).astype(np.uint32)
    self_d = np.array([O.flat_knn_batch(base[r:r + 1], base[r:r + 1], 1, 1)[1][0, 0] for r in range(96)], dtype=np.float32)
    neg, zero = np.flatnonzero(self_d < 0), np.flatnonzero((self_d == 0) & (np.arange(96) != 40))
    assert len(neg) >= 2 and len(zero) >= 2, "the oracle's cosine has negative and exactly zero self-distances among 96 rows"
    a, b = int(neg[0]), int(next(z for z in zero if lab[z] != lab[neg[0]] or lab[z] == NONE))
    qs = np.concatenate([base[[a, b]], base[[b]], np.zeros((1, 8), np.float32), base[[40, a]], base[neg[:2]]]).astype(np.float32)
    lims = np.array([0, 2, 3, 4, 6, 8], dtype=np.uint64)  # (neg, zero) | (zero) | (zero VECTOR) | (the zero row, neg) | (neg, neg)
    cand = np.tile(np.array([b, a, 40, 41, 9, neg[1], zero[1], 95], dtype=np.uint64), (5, 1))
    cnt = np.full(5, 8, dtype=np.uint64)
    dm = _dense(base, qs, 1)
    assert (dm < 0).any() and dm[0, a] < 0 and dm[0, a].view(np.uint32) >> 31 == 1 and dm[1, b].view(np.uint32) == 0
    assert (dm[3] == 1).all() and (dm[:, 40] == 1).all(), "the clamp: a zero vector is at distance 1 from everything"
    ix = _index(base, "cosine", lab)
    try:
        for mode in ("sum", "min"):
            for k in (8, 1):
                _all_forms(ix, qs, lims, cand, cnt, k, 0, mode, rescore_ref.expect(dm, lab, lims, cand, cnt, k, mode), f"cosine {mode} k={k}")
        exp = rescore_ref.expect(dm, lab, lims, cand, cnt, 8, "min")
        assert exp[1][0, 0] >> 31 == 1 and exp[1][0, 1] == 0 and exp[0][0, 0] == a and exp[0][0, 1] == b, "a negative score, then +0"
    finally:
        ix.close()
