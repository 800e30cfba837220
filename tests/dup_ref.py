"""The reference of the near-duplicate grouping (vdb_flat_dup_groups, vdb_link_pairs_device): a union-find over CSR edge lists with the
LOWEST row of a component as its representative and the call's limit rule, a brute-force restatement by label propagation to check it
against (tests/test_dup_ref_cpu.py), and the planted-copy tables the GPU tests group.

The rule (include/vdbhip.h): query q's list is ids[lims[q]:lims[q + 1]], the rows near row src[q] in the (distance, index) order; with a
limit L > 0 only its first L entries count, and a list that reaches L entries is a truncated one.  Every listed j != src[q] is an
undirected edge.  The groups are the connected components (single linkage); group[i] = the lowest row of i's component + id_offset,
ROW_NONE for a row that is not allowed."""
import numpy as np

ROW_NONE = 2 ** 64 - 1


def _cut(src, lims, ids, limit):
    """the (u, v) pairs of the lists after the limit, self pairs included, and the number of lists that reached the limit"""
    pairs, truncated = [], 0
    for q in range(len(src)):
        lst = [int(x) for x in ids[int(lims[q]):int(lims[q + 1])]]
        if limit:
            lst = lst[:limit]
            truncated += len(lst) == limit
        pairs.extend((int(src[q]), v) for v in lst)
    return pairs, truncated


def _answer(n, root_of, allowed, pairs, truncated, id_offset):
    ok = np.ones(n, dtype=bool) if allowed is None else np.asarray(allowed, dtype=bool)
    group = np.full(n, ROW_NONE, dtype=np.uint64)
    sizes = {}
    for i in range(n):
        if ok[i]:
            r = root_of(i)
            group[i] = r + id_offset
            sizes[r] = sizes.get(r, 0) + 1
    big = [s for s in sizes.values() if s >= 2]
    stats = {"groups": len(big), "rows": sum(big), "pairs": sum(1 for u, v in pairs if u != v), "truncated": truncated}
    return group, stats


def dup_ref(n, src, lims, ids, allowed=None, limit=0, id_offset=0):
    """(group uint64 [n], stats dict) by union-find: src / ids hold LOCAL rows"""
    pairs, truncated = _cut(src, lims, ids, limit)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for u, v in pairs:
        a, b = find(u), find(v)
        if a != b:
            parent[max(a, b)] = min(a, b)
    return _answer(n, find, allowed, pairs, truncated, id_offset)


def dup_brute(n, src, lims, ids, allowed=None, limit=0, id_offset=0):
    """the same by repeated label propagation: every row starts with its own number, every pair takes the smaller label of its ends,
    until nothing changes"""
    pairs, truncated = _cut(src, lims, ids, limit)
    label = list(range(n))
    changed = True
    while changed:
        changed = False
        for u, v in pairs:
            m = min(label[u], label[v])
            if label[u] != m or label[v] != m:
                label[u] = label[v] = m
                changed = True
    return _answer(n, lambda i: label[i], allowed, pairs, truncated, id_offset)


def csr(lists):
    """(lims uint64 [nq + 1], ids uint64) of a list of lists"""
    lims = np.zeros(len(lists) + 1, dtype=np.uint64)
    lims[1:] = np.cumsum([len(x) for x in lists], dtype=np.uint64)
    ids = np.array([v for x in lists for v in x], dtype=np.uint64)
    return lims, ids


# ---- planted copies ---------------------------------------------------------------------------------------------------------------------
# Inside a gist-like table, `seeds` seed rows get 1 .. 5 copies each, written over other rows at random places:
#   star   every copy is the seed plus a small perturbation; ALL pairs of a star's rows are planted pairs.
#   chain  copy k is the seed with coordinate 0 moved by k steps of `step` along the axis: CONSECUTIVE rows are planted pairs, at squared
#          distance step^2 exactly; rows two apart lie at 4 step^2 exactly (f32: the coordinates are multiples of 1/16 below 1; u8: small
#          integers), and they are NOT planted pairs -- a chain is one group only through its middle rows.
# radius = 2 step^2: a planted pair is inside it by a factor of 2 (D <= radius / 2: consecutive chain rows exactly at it), every other pair
# outside it by a factor of 2 (D >= 2 radius: chain rows two apart exactly at it).  Both margins are verified in float64 by
# tests/test_dup_ref_cpu.py for the seeds the GPU tests use, so no case sits on the radius itself by accident.
PLANTED_SEEDS = {"f32": 2024, "u8": 2025}  # the tables the GPU tests use: planted_table(20000, 128, kind, PLANTED_SEEDS[kind])


def planted_table(n, dim, kind="f32", seed=2024, seeds=200):
    """(table, radius, truth, pairs, chains): table f32 [n][dim] (kind "u8": uint8), truth[i] = the lowest row of i's planted group (i for
    a row alone), pairs = the planted pairs as an array [p][2], chains = per chain the rows in chain order"""
    from conftest import gist_like

    rng = np.random.default_rng(seed)
    x = gist_like(n, dim=dim, seed=seed)
    if kind == "u8":
        x = np.clip(np.round(x * 300.0), 0, 250).astype(np.uint8)
        step = 2
    else:
        step = 1.0 / 16
    radius = 2.0 * step * step
    place = rng.permutation(n)
    seed_rows, free = place[:seeds], list(place[seeds:])
    truth = np.arange(n, dtype=np.int64)
    pairs, chains = [], []
    for s_at, s in enumerate(seed_rows.tolist()):
        copies = [int(free.pop()) for _ in range(int(rng.integers(1, 6)))]
        members = [s] + copies
        if s_at % 3 == 0:  # a chain along coordinate 0
            x[s, 0] = 32 if kind == "u8" else 0.25
            for k, c in enumerate(copies, start=1):
                x[c] = x[s]
                x[c, 0] = x[s, 0] + (step * k if kind == "u8" else np.float32(step * k))
            pairs.extend((members[k], members[k + 1]) for k in range(len(copies)))
            chains.append(members)
        else:  # a star
            for k, c in enumerate(copies):
                x[c] = x[s]
                if kind == "u8":  # one coordinate of its own moved by one: D(seed, copy) = 1, D(copy, copy) = 2
                    j = 1 + k
                    x[c, j] = x[s, j] + 1 if x[s, j] < 200 else x[s, j] - 1
                else:  # a perturbation of norm 0.4 step on coordinates that stay inside [0, 1]: D(copy, copy) <= 0.64 step^2 (+ rounding)
                    v = rng.standard_normal(dim).astype(np.float64)
                    v *= 0.4 * step / np.linalg.norm(v)
                    x[c] = (x[s].astype(np.float64) + v).astype(np.float32)
            pairs.extend((members[a], members[b]) for a in range(len(members)) for b in range(a + 1, len(members)))
        truth[members] = min(members)
    return x, float(radius), truth, np.array(pairs, dtype=np.int64), chains
