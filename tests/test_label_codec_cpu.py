"""CPU: LabelCodec (lab_1806_vec_db_amd/labels.py) -- which metadata keys become label columns, which code a value gets, and how a
filter pattern becomes (column, code) terms.  Pure Python: neither the library nor a GPU is touched."""
import numpy as np

from lab_1806_vec_db_amd.labels import LABEL_COLUMNS, LABEL_NONE, MASK_MAX_TERMS, NOTHING, LabelCodec

META = [{"id": str(i), "body": "text " * 50 + str(i), "lang": ("en", "fr", "de")[i % 3], **({"kind": "ab"[i % 2]} if i % 4 else {})} for i in range(40)]


def _host(meta, pattern):
    return np.array([all(m.get(k) == v for k, v in pattern.items()) for m in meta], dtype=np.bool_)


class _Twin:
    """a codec and the columns it encoded, as a table would keep them on the device"""

    def __init__(self, meta):
        self.codec, self.meta, self.cols = LabelCodec(), meta, {}

    def use(self, pattern):
        new = self.codec.assign(pattern)
        for k in new or ():
            self.cols[self.codec.column_of(k)] = self.codec.encode_rows(k, self.meta)
        return new

    def select(self, pattern):
        """what the pattern's terms select over the columns (NONE for a column never encoded): the kernel's arithmetic in numpy"""
        ok = np.ones(len(self.meta), dtype=np.bool_)
        for c, code in self.codec.terms(pattern):
            ok &= self.cols.get(c, np.full(len(self.meta), LABEL_NONE, dtype=np.uint32)) == code
        return ok


def test_columns_are_assigned_lazily_in_order_of_first_use():
    t = _Twin(META)
    c = t.codec
    assert c.keys() == [] and c.column_of("lang") is None
    assert c.terms({"lang": "en"}) is None  # no column yet: nothing is assigned by asking
    assert c.keys() == []
    assert t.use({"kind": "a"}) == ["kind"] and c.column_of("kind") == 0
    assert t.use({"lang": "en", "kind": "b"}) == ["lang"] and c.column_of("lang") == 1
    assert t.use({"lang": "fr"}) == []
    # ids and text bodies exist in every row and were never asked for: never interned
    assert c.keys() == ["kind", "lang"] and len(c.codes) == 2
    assert set(c.codes[0]) == {"a", "b"} and set(c.codes[1]) == {"en", "fr", "de"}
    # codes count up from 0 in order of first appearance
    assert c.codes[1] == {"en": 0, "fr": 1, "de": 2}


def test_missing_key_encodes_as_none_and_patterns_match_the_host_loop():
    t = _Twin(META)
    c = t.codec
    t.use({"kind": "a", "lang": "en"})
    kind = t.cols[0]
    assert kind.dtype == np.uint32
    assert [int(v) for v in kind[:5]] == [LABEL_NONE, 0, 1, 0, LABEL_NONE]  # rows 0, 4, .. have no "kind"
    for p in ({"kind": "a"}, {"lang": "de"}, {"kind": "b", "lang": "fr"}, {}, {"kind": None}, {"kind": "zz"}, {"lang": "en", "kind": "zz"}):
        assert np.array_equal(t.select(p), _host(META, p)), p
    assert c.terms({}) == []  # the empty pattern: zero terms, every row
    assert c.terms({"kind": None}) == [(0, LABEL_NONE)]


def test_unseen_value_matches_nothing_without_growing_the_dictionary():
    c = _Twin(META).codec
    c.assign({"lang": "en"})
    c.encode_rows("lang", META)
    before = dict(c.codes[0])
    t = c.terms({"lang": "xx"})
    assert t == list(NOTHING) and t[0][0] == t[1][0] and t[0][1] != t[1][1]  # two codes asked of one column: no row
    assert c.terms({"lang": "en"}) == [(0, 0)]
    assert c.codes[0] == before


def test_not_expressible_patterns():
    c = LabelCodec()
    nine = {f"k{i}": "v" for i in range(MASK_MAX_TERMS + 1)}
    assert not c.expressible(nine) and c.assign(nine) is None and c.terms(nine) is None and c.keys() == []
    eight = {f"k{i}": "v" for i in range(MASK_MAX_TERMS)}
    assert c.expressible(eight) and c.assign(eight) == list(eight)
    for i in range(MASK_MAX_TERMS, LABEL_COLUMNS):
        assert c.assign({f"k{i}": "v"}) == [f"k{i}"]
    assert len(c.keys()) == LABEL_COLUMNS
    # the 17th key gets no column, alone or next to keys that have one; nothing is assigned by the attempt
    assert not c.expressible({"k16": "v"}) and c.assign({"k16": "v"}) is None and c.terms({"k16": "v"}) is None
    assert c.assign({"k0": "v", "k16": "v"}) is None and len(c.keys()) == LABEL_COLUMNS and c.column_of("k16") is None
    assert c.expressible({"k0": "v", "k15": "w"})  # the keys that have columns still work
    # a value that is no string cannot be looked up as the host loop compares it
    assert not LabelCodec().expressible({"n": 5})
    # an assignment whose encoding failed is taken back
    d = LabelCodec()
    d.assign({"a": "1"})
    new = d.assign({"b": "1", "c": "2"})
    d.unassign(new)
    assert d.keys() == ["a"] and len(d.codes) == 1


def test_incremental_encode_equals_full_encode():
    more = [{"lang": ("it", "en", "fr")[i % 3], "kind": "c"} if i % 5 else {"id": "x"} for i in range(23)]
    full = LabelCodec()
    full.assign({"lang": "en", "kind": "a"})
    whole = {k: full.encode_rows(k, META + more) for k in ("lang", "kind")}
    inc = LabelCodec()
    inc.assign({"lang": "en", "kind": "a"})
    first = {k: inc.encode_rows(k, META) for k in ("lang", "kind")}
    second = {k: inc.encode_rows(k, more) for k in ("lang", "kind")}
    for k in ("lang", "kind"):
        assert np.array_equal(np.concatenate([first[k], second[k]]), whole[k]), k
    assert inc.codes == full.codes
    assert int(second["lang"][0]) == LABEL_NONE and int(second["kind"][1]) == 2  # a row without the keys / a value first seen in the new rows
