"""CPU: filter expressions of labels.py -- AnyOf, AllOf and Not over pattern dicts -- and their normal form over label columns
(LabelCodec.compile_any).  matches_filter is the definition; the compiled form is evaluated here exactly as the device evaluates it
(OR over clauses of AND over LabelTerm.select on the encoded columns) and must agree with it row by row.  No GPU and no library."""
import numpy as np
import pytest

from lab_1806_vec_db_amd.labels import (LABEL_NONE, MASK_MAX_SET_BITS, AllOf, AnyOf, Between, Exists, Ge, Gt, In, LabelCodec, LabelTerm, Le, Lt, Ne, Not,
                                        NotIn, filter_key, filter_patterns, matches_filter)

KEYS = ("tenant", "source", "year", "lang")
VALUES = {"tenant": [f"t{i}" for i in range(6)], "source": ["web", "mail", "scan", "api"], "year": [str(y) for y in range(1995, 2012)] + ["n/a", "2003.5"],
          "lang": ["de", "en", "fr"]}


def _rows(rng, n=200):
    rows = []
    for _ in range(n):
        m = {}
        for k in KEYS:
            if rng.random() < 0.75:
                m[k] = VALUES[k][int(rng.integers(len(VALUES[k])))]
        if rng.random() < 0.05:
            m["lang"] = None  # a key held with None reads as missing
        rows.append(m)
    return rows


def _codec(rows, keys=KEYS):
    codec = LabelCodec()
    assert codec.assign({k: None for k in keys}) == list(keys)
    return codec, {codec.column_of(k): codec.encode_rows(k, rows) for k in keys}


def _evaluate(clauses, cols, n):
    """what the device computes from a normal form: a row matches when it matches every term of some clause"""
    out = np.zeros(n, dtype=np.bool_)
    for c in clauses:
        ok = np.ones(n, dtype=np.bool_)
        for t in c:
            ok &= t.select(cols[t.column])
        out |= ok
    return out


def test_complement_is_exact():
    values = np.array([0, 1, 2, 3, 62, 63, 64, 65, 127, 128, 129, 200, 0xFFFFFFFE, LABEL_NONE], dtype=np.uint32)
    terms = []
    for neg in (False, True):
        for none in (False, True):
            terms += [LabelTerm(3, codes=[1, 63, 64, 128], negate=neg, none=none), LabelTerm(3, 0, 200, codes=[2, 129], negate=neg, none=none),
                      LabelTerm(3, 2, 128, negate=neg, none=none), LabelTerm(3, 64, 0xFFFFFFFF, negate=neg, none=none),
                      LabelTerm(3, 1, 0, negate=neg, none=none), LabelTerm(3, negate=neg, none=none), LabelTerm(3, 9, 4, negate=neg, none=none)]
    for t in terms:
        c = t.complement()
        assert np.array_equal(c.select(values), ~t.select(values)), t
        assert c.complement() == t and c.column == t.column and (c.lo, c.hi, c.codes) == (t.lo, t.hi, t.codes)
        assert c.negate != t.negate and c.none != t.none
    assert LabelTerm(0).matches_nothing() and LabelTerm(0).complement().matches_everything()
    assert not LabelTerm(0, 1, 0, none=True).matches_nothing() and not LabelTerm(0, 3, 3).complement().matches_everything()


def _random_value(rng, key):
    pool = VALUES[key] + ["never-seen"]
    pick = lambda: pool[int(rng.integers(len(pool)))]  # noqa: E731
    kind = int(rng.integers(0, 11))
    if kind <= 1:
        return pick()
    if kind == 2:
        return None
    if kind == 3:
        return In([pick() for _ in range(int(rng.integers(0, 4)))] + ([None] if rng.random() < 0.3 else []))
    if kind == 4:
        return NotIn([pick() for _ in range(int(rng.integers(0, 4)))] + ([None] if rng.random() < 0.3 else []))
    if kind == 5:
        return Ne(pick() if rng.random() < 0.8 else None)
    if kind == 6:
        return Exists(bool(rng.integers(0, 2)))
    if key == "year" and rng.random() < 0.7:  # numeric order ("n/a" never matches, "2003.5" parses)
        b = int(rng.integers(1993, 2014))
        return (Lt(b), Le(b), Gt(b), Ge(b + 0.5), Between(b - 4, b))[int(rng.integers(0, 5))]
    a, b = sorted((pick(), pick()))
    return (Lt(a), Le(a), Gt(a), Ge(a), Between(a, b))[int(rng.integers(0, 5))]  # string order


def _random_expr(rng, depth):
    kind = int(rng.integers(0, 4)) if depth > 0 else 0
    if kind == 0:
        keys = [k for k in KEYS if rng.random() < 0.4]
        return {k: _random_value(rng, k) for k in keys}
    if kind == 3:
        return Not(_random_expr(rng, depth - 1))
    return (AnyOf, AllOf)[kind - 1](*[_random_expr(rng, depth - 1) for _ in range(int(rng.integers(0, 4)))])


def test_random_expressions_agree_with_matches_filter():
    rng = np.random.default_rng(1806)
    rows = _rows(rng)
    codec, cols = _codec(rows)
    tables = [dict(t) for t in codec.codes]
    compiled = clause_counts = 0
    selected = set()
    for i in range(600):
        e = _random_expr(rng, 3)
        clauses = codec.compile_any(e)
        if clauses is None:  # only a size limit can refuse these: every key has a column, every value is legal
            continue
        compiled += 1
        clause_counts = max(clause_counts, len(clauses))
        assert len(clauses) <= 64 and all(len(c) <= 8 and all(isinstance(t, LabelTerm) for t in c) for c in clauses)
        got = _evaluate(clauses, cols, len(rows))
        want = np.array([matches_filter(e, m) for m in rows])
        assert np.array_equal(got, want), (i, e, clauses)
        selected.add(int(want.sum()))
    assert compiled >= 500 and clause_counts >= 4 and len(selected) > 50, (compiled, clause_counts, len(selected))
    assert [dict(t) for t in codec.codes] == tables  # the dictionary never grows


def test_empty_forms():
    rows = _rows(np.random.default_rng(2), 20)
    codec, cols = _codec(rows)
    for e, clauses, every in ((AnyOf(), [], False), (AllOf(), [[]], True), (Not(AnyOf()), [[]], True), (Not(AllOf()), [], False), ({}, [[]], True),
                              (Not({}), [], False), (AnyOf({"tenant": "never-seen"}), [], False), (AllOf({"lang": "de"}, AnyOf()), [], False),
                              (AnyOf({"lang": "de"}, AllOf()), [[]], True), (Not({"tenant": "never-seen"}), [[]], True)):
        assert codec.compile_any(e) == clauses, e
        assert all(matches_filter(e, m) == every for m in rows), e
    one = codec.compile_any(AnyOf({"lang": "de"}, {"lang": "de"}, AllOf({"lang": "de"}, {})))
    assert one == [[LabelTerm.of((codec.column_of("lang"), codec.codes[codec.column_of("lang")]["de"]))]]  # equal clauses and terms are kept once
    assert codec.compile_any({"lang": None}) == [[LabelTerm.of((codec.column_of("lang"), LABEL_NONE))]]


def test_what_is_not_expressible():
    rows = _rows(np.random.default_rng(3), 50)
    codec, _ = _codec(rows)
    two = lambda k: AnyOf({k: VALUES[k][0]}, {k: VALUES[k][1]})  # noqa: E731
    keys7 = ("tenant", "source", "year", "lang", "tenant", "source", "year")
    wide = AllOf(*[AnyOf({k: VALUES[k][j]}, {KEYS[(i + 1) % 4]: VALUES[KEYS[(i + 1) % 4]][j + 1]}) for i, (k, j) in enumerate(zip(keys7, (0, 0, 0, 0, 1, 1, 1)))])
    assert codec.compile_any(wide) is None  # seven 2-way ORs under an AND: 128 clauses
    assert len(codec.compile_any(AllOf(*[two(k) for k in KEYS]))) == 16
    assert codec.compile_any(AnyOf({"tenant": "t0"}, {"colour": "red"})) is None          # a key without a column
    assert codec.compile_any(AnyOf({"tenant": 7})) is None                                 # a value that is no str, None or predicate
    assert codec.compile_any(Not(AllOf({"tenant": "t0"}, {"tenant": ("t1",)}))) is None
    many = LabelCodec()
    ks = [f"k{i}" for i in range(9)]
    for k in ks:
        many.assign({k: None})
        many.encode_rows(k, [{k: "a"}, {k: "b"}])
    assert many.compile_any(AllOf(*[{k: "a"} for k in ks])) is None                        # one clause of 9 terms
    assert len(many.compile_any(Not(AllOf(*[{k: "a"} for k in ks])))) == 9                 # ... its negation: 9 clauses of one term
    assert many.compile_any(AllOf(*[{k: "a"} for k in ks[:8]])) is not None
    big = LabelCodec()
    big.assign({"id": None})
    big.codes[0].update({"a": 0, "b": MASK_MAX_SET_BITS})  # two codes whose bitmap spans more than a call may carry
    assert big.compile_any(AnyOf({"id": In(["a", "b"])})) is None and big.compile_any(AnyOf({"id": "b"})) is not None


def test_expressions_are_frozen_values():
    a = AnyOf({"tenant": "t1", "year": Ge(2010)}, Not({"lang": In(["de", "fr"])}))
    b = AnyOf({"year": Ge(2010), "tenant": "t1"}, Not({"lang": In(["fr", "de"])}))
    assert a == b and hash(a) == hash(b) and len({a, b}) == 1 and {a: 1}[b] == 1
    assert a != AllOf(*a.exprs) and Not(a) != a and Not(a) == Not(b) and AnyOf() != AllOf()
    assert AnyOf({"tenant": "t1"}, {"lang": "de"}) != AnyOf({"lang": "de"}, {"tenant": "t1"})  # operand order is part of the identity
    with pytest.raises(AttributeError):
        a.exprs = ()
    with pytest.raises(TypeError):
        AnyOf("tenant")
    with pytest.raises(TypeError):
        Not({"tenant": ["t1"]})  # cannot key a cache
    with pytest.raises(TypeError):
        Not()
    pat = {"tenant": "t1"}
    e = AllOf(pat)
    pat["tenant"] = "t2"
    assert e.exprs[0] == {"tenant": "t1"}  # operands are copied
    assert filter_key({"tenant": "t1", "lang": None}) == frozenset({("tenant", "t1"), ("lang", None)}) and filter_key(a) is a
    assert filter_patterns(a) == [{"tenant": "t1", "year": Ge(2010)}, {"lang": In(["de", "fr"])}] and filter_patterns(pat) == [pat]
    with pytest.raises(TypeError):
        matches_filter("tenant", {})
