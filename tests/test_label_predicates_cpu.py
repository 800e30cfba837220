"""CPU: the filter predicates of lab_1806_vec_db_amd/labels.py (In, NotIn, Ne, Exists, Lt, Le, Gt, Ge, Between), `matches` -- the one
definition of what they mean -- and LabelCodec.compile, which turns a pattern that holds them into LabelTerm set / range terms.
`matches` is compared with lambdas written out here, never with itself; `compile` by expanding its terms in numpy over the encoded
columns (LabelTerm.select restates the kernel's arithmetic) and comparing with the same lambdas row by row.  Pure Python."""
import math

import numpy as np
import pytest

from lab_1806_vec_db_amd.labels import (LABEL_NONE, MASK_MAX_TERMS, NOTHING, Between, Exists, Ge, Gt, In, LabelCodec, LabelTerm, Le, Lt, Ne,
                                        NotIn, matches)

LANGS = ("en", "fr", "de", "it", "es")
YEARS = ("1999", "2005", "2010", "2010.5", "2015", "2021", "n/a", "", "1e3", "nan")
META = []
for i in range(120):
    m = {"id": str(i)}
    if i % 7:
        m["lang"] = LANGS[i % 5]
    if i % 11:
        m["year"] = YEARS[i % len(YEARS)]
    if i == 50:
        m["lang"] = ["a", "list"]  # a value no dictionary can hold
    META.append(m)


def _num(x):
    """what a numeric bound compares: the float a str parses to, None for everything else"""
    if not isinstance(x, str):
        return None
    try:
        f = float(x)
    except ValueError:
        return None
    return None if math.isnan(f) else f


# (key, predicate, the same thing as a lambda on x = metadata.get(key))
CASES = [
    ("lang", In(["en", "de"]), lambda x: isinstance(x, str) and x in ("en", "de")),
    ("lang", In(["en", None]), lambda x: x is None or x == "en"),
    ("lang", In(["xx", None]), lambda x: x is None),
    ("lang", In([]), lambda x: False),
    ("lang", NotIn(["en", "de"]), lambda x: not (isinstance(x, str) and x in ("en", "de"))),
    ("lang", NotIn(["fr", None]), lambda x: x is not None and x != "fr"),
    ("lang", NotIn(["xx"]), lambda x: True),
    ("lang", Ne("it"), lambda x: x != "it"),
    ("lang", Ne("xx"), lambda x: True),
    ("lang", Ne(None), lambda x: x is not None),
    ("lang", Exists(), lambda x: x is not None),
    ("lang", Exists(False), lambda x: x is None),
    ("lang", Lt("es"), lambda x: isinstance(x, str) and x < "es"),
    ("lang", Le("es"), lambda x: isinstance(x, str) and x <= "es"),
    ("lang", Gt("es"), lambda x: isinstance(x, str) and x > "es"),
    ("lang", Ge("es"), lambda x: isinstance(x, str) and x >= "es"),
    ("lang", Between("en", "fr"), lambda x: isinstance(x, str) and "en" <= x <= "fr"),
    ("lang", Between("fr", "en"), lambda x: False),
    ("year", Ge(2010), lambda x: _num(x) is not None and _num(x) >= 2010),
    ("year", Gt(2010), lambda x: _num(x) is not None and _num(x) > 2010),
    ("year", Le(2010.5), lambda x: _num(x) is not None and _num(x) <= 2010.5),
    ("year", Lt(1000), lambda x: _num(x) is not None and _num(x) < 1000),
    ("year", Between(1000, 2010), lambda x: _num(x) is not None and 1000 <= _num(x) <= 2010),
    ("year", Ge(float("nan")), lambda x: False),
    ("year", Between(float("nan"), 3000), lambda x: False),
    ("year", Ge("2"), lambda x: isinstance(x, str) and x >= "2"),  # a string bound on the same key: string order ("n/a" >= "2")
    ("year", Lt(float("inf")), lambda x: _num(x) is not None and _num(x) < float("inf")),
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_matches_against_a_lambda(case):
    key, pred, want = CASES[case]
    seen = set()
    for m in META:
        x = m.get(key)
        assert matches(pred, x) is bool(want(x)), (pred, x)
        seen.add(bool(want(x)))
    # values the table does not hold
    for x in (None, 5, 2015, 3.5, ["en"], ("en",), "zz", "n/a", "-1", "inf"):
        assert matches(pred, x) is bool(want(x)), (pred, x)
    assert seen  # (the table was walked)


def test_hand_written_points():
    assert matches(Ge(2010), "2010") and not matches(Ge(2010), "2009.9") and not matches(Ge(2010), "n/a") and not matches(Ge(2010), None)
    assert not matches(Ge(2010), 2015)  # only strings that parse: the metadata of a table are strings
    assert matches(Lt("b"), "a") and not matches(Lt("b"), "b") and not matches(Lt("b"), None) and not matches(Lt("b"), 0)
    assert matches(Ne("a"), None) and matches(Ne("a"), "b") and not matches(Ne("a"), "a")
    assert matches(In([None]), None) and not matches(In(["a"]), None) and matches(NotIn(["a"]), None) and not matches(NotIn([None]), None)
    assert matches(Between(1, 2), "2") and not matches(Between(1, 2), "2.0001") and not matches(Between(1, 2), "nan")
    assert not matches(Ge(float("nan")), "1") and not matches(Lt(float("nan")), "1")
    # plain values: == as the host loop always compared
    assert matches("a", "a") and not matches("a", None) and matches(None, None) and not matches(None, "a") and matches(5, 5)


def test_predicates_are_frozen_hashable_values():
    assert In(["a", "b"]) == In(("b", "a")) and hash(In(["a", "b"])) == hash(In(["b", "a"]))
    assert In(["a"]) != NotIn(["a"]) and Ge(1) != Gt(1) and Ge(1) == Ge(1) and Between(1, 2) != Between(1, 3)
    assert len({frozenset({"k": Ge(2010)}.items()), frozenset({"k": Ge(2010)}.items()), frozenset({"k": Ge(2011)}.items())}) == 2
    with pytest.raises(AttributeError):
        Ge(1).bound = 2
    for bad in (lambda: Ge(True), lambda: Lt(None), lambda: Between(1, "2"), lambda: Between(False, 2), lambda: Le([1])):
        with pytest.raises(TypeError):
            bad()
    with pytest.raises(TypeError):
        In([["unhashable"]])


def test_label_term_values():
    t = LabelTerm(2, codes=[70, 3, 3, 64])
    assert (t.lo, t.hi, t.codes, t.flags, t.set_bits) == (3, 70, (3, 64, 70), 0, 128)
    words = t.bitmap()
    assert words.dtype == np.uint64 and [int(w) for w in words] == [1 | 1 << 61, 1 << 3]  # bit j = code lo + j
    assert LabelTerm(1, 0, 200, codes=[5]).set_bits == 256 and LabelTerm(1, 5, 9).set_bits == 0 and LabelTerm(1, 5, 9).bitmap().size == 0
    e = LabelTerm(4, negate=True, none=True)
    assert (e.lo, e.hi, e.codes, e.flags) == (1, 0, None, 3) and LabelTerm(4, codes=[]) == LabelTerm(4)
    assert LabelTerm(1, 5, 9) == LabelTerm(1, 5, 9) and hash(LabelTerm(1, 5, 9)) == hash(LabelTerm(1, 5, 9)) and LabelTerm(1, 5, 9) != LabelTerm(1, 5, 9, none=True)
    with pytest.raises(AttributeError):
        t.lo = 0
    for bad in (lambda: LabelTerm(0, 5, 9, codes=[4]), lambda: LabelTerm(0, 5), lambda: LabelTerm(0, codes=[LABEL_NONE]), lambda: LabelTerm(0, -1, 4)):
        with pytest.raises(ValueError):
            bad()
    # the two documented equivalences of the equality terms
    assert LabelTerm.of((3, 7)) == LabelTerm(3, 7, 7) and LabelTerm.of((3, LABEL_NONE)) == LabelTerm(3, 1, 0, none=True)
    v = np.array([0, 7, 8, LABEL_NONE], dtype=np.uint32)
    assert LabelTerm.of((3, 7)).select(v).tolist() == [False, True, False, False]
    assert LabelTerm.of((3, LABEL_NONE)).select(v).tolist() == [False, False, False, True]
    assert LabelTerm(0, 1, 0, negate=True).select(v).tolist() == [True, True, True, False]  # negate never inverts the NONE case


class _Twin:
    """a codec and the columns it encoded, as a table would keep them on the device"""

    def __init__(self, meta, keys):
        self.codec, self.meta, self.cols = LabelCodec(), meta, {}
        for k in self.codec.assign({k: "x" for k in keys}):
            self.cols[self.codec.column_of(k)] = self.codec.encode_rows(k, meta)

    def select(self, terms):
        ok = np.ones(len(self.meta), dtype=np.bool_)
        for t in terms:
            ok &= LabelTerm.of(t).select(self.cols[LabelTerm.of(t).column])
        return ok


@pytest.fixture(scope="module")
def twin():
    return _Twin(META, ("lang", "year"))


@pytest.mark.parametrize("case", range(len(CASES)))
def test_compile_against_a_lambda(twin, case):
    key, pred, want = CASES[case]
    before = [dict(d) for d in twin.codec.codes]
    terms = twin.codec.compile({key: pred})
    assert terms is not None
    expect = np.array([bool(want(m.get(key))) for m in META])
    assert np.array_equal(twin.select(terms), expect), (pred, terms)
    if terms is not NOTHING:
        assert len(terms) == 1 and all(isinstance(t, LabelTerm) for t in terms)
    assert twin.codec.codes == before  # a never-seen value does not grow the dictionary
    assert twin.codec.expressible({key: pred}) and twin.codec.missing({key: pred}) == []


def test_compile_mixed_patterns(twin):
    for pat, want in (
        ({"lang": In(["en", "fr"]), "year": Ge(2010)}, lambda m: m.get("lang") in ("en", "fr") and _num(m.get("year")) is not None and _num(m.get("year")) >= 2010),
        ({"lang": "de", "year": Ne("2010")}, lambda m: m.get("lang") == "de" and m.get("year") != "2010"),
        ({"lang": None, "year": Exists()}, lambda m: m.get("lang") is None and m.get("year") is not None),
        ({"lang": NotIn(["en"]), "year": "zz"}, lambda m: False),
    ):
        terms = twin.codec.compile(pat)
        assert np.array_equal(twin.select(terms), np.array([bool(want(m)) for m in META])), pat
    assert twin.codec.compile({}) == []


def test_nothing_none_and_plain_values(twin):
    c = twin.codec
    assert c.compile({"lang": In(["xx", "yy"])}) is NOTHING  # no known value: no row
    assert c.compile({"lang": "xx"}) is NOTHING and c.compile({"lang": In([])}) is NOTHING
    assert c.compile({"lang": In(["xx", None])}) == [LabelTerm(0, 1, 0, none=True)]  # ... but the rows without the key still match
    assert c.compile({"id": In(["1"])}) is None  # a key without a column
    nine = {f"k{i}": Exists() for i in range(MASK_MAX_TERMS + 1)}
    assert c.compile(nine) is None and not c.expressible(nine) and LabelCodec().assign(nine) is None
    # plain-value behaviour is unchanged: a value that is no string stays inexpressible, terms() knows no predicates
    assert not LabelCodec().expressible({"n": 5}) and not LabelCodec().expressible({"n": ["a"]})
    assert c.compile({"lang": 5}) is None and c.terms({"lang": In(["en"])}) is None
    assert c.terms({"lang": "en"}) == [(0, c.codes[0]["en"])] and c.terms({"lang": None}) == [(0, LABEL_NONE)]
    # predicates take part in column assignment like any other value
    d = LabelCodec()
    assert d.expressible({"a": Ge(1)}) and d.missing({"a": Ge(1), "b": "x"}) == ["a", "b"] and d.assign({"a": Ge(1)}) == ["a"]
    # a run of codes needs no bitmap; scattered codes carry one
    run = c.compile({"lang": In(["fr", "de", "it"])})[0]  # codes 0, 1, 2 in order of first appearance
    assert run.codes is None and (run.lo, run.hi) == (0, 2)


def test_bitmap_span_over_the_cap_is_not_expressible():
    c = LabelCodec()
    c.assign({"k": "x"})
    c.codes[0].update({"a": 0, "b": (1 << 27) + 64})  # two codes a dictionary of that size would hold
    assert c.compile({"k": In(["a", "b"])}) is None
    assert c.compile({"k": In(["a"])}) == [LabelTerm(0, 0, 0)]
