"""LabelCodec -- the host-side dictionary between metadata (key -> value dicts) and the integer label columns of an index.

Pure Python: no GPU and no library.  The codec decides WHICH metadata keys become label columns and which code a value gets; the
index holds the codes (GpuIndex.set_labels) and evaluates patterns over them (GpuIndex.make_mask_where).

  * Keys are assigned to columns LAZILY, in order of first use in a filter pattern, at most LABEL_COLUMNS of them.  Metadata of a
    retrieval table carries ids and whole text bodies: a key is never interned merely because rows have it.
  * Per column, values are interned to codes 0, 1, 2, .. in order of first appearance; a row without the key (or with None) encodes as
    LABEL_NONE, which is also what a pattern value of None encodes to -- `m.get(k) == v`, the match the host loop makes.
  * A pattern -- every key present with an equal value -- encodes to at most MASK_MAX_TERMS (column, code) terms, or to "matches
    nothing" when one of its values was never seen in its column (without growing the dictionary).
  * A pattern value may also be a PREDICATE on the key's value x = metadata.get(key): In, NotIn, Ne, Exists, Lt, Le, Gt, Ge, Between.
    `matches` is the one definition of what they mean.  Over a label column every predicate on one key is a SET OF CODES plus one bit for
    "rows without a value": LabelCodec.compile evaluates the predicate over the column's dictionary (one entry per distinct value) and
    emits LabelTerm objects (column, [lo, hi], negate, none, codes) that the index tests per row (GpuIndex.make_masks_where_sets).
  * A FILTER EXPRESSION joins patterns with AnyOf, AllOf and Not; `matches_filter` is the one definition of what it means.  Every term
    has an exact complement (LabelTerm.complement), so LabelCodec.compile_any pushes NOT down to the terms and returns the expression's
    disjunctive normal form: a list of clauses, each a list of LabelTerm, that the index evaluates in one pass
    (GpuIndex.make_masks_where_any).
"""
from __future__ import annotations

import math

import numpy as np

LABEL_COLUMNS = 16       # VDB_LABEL_COLUMNS
LABEL_NONE = 0xFFFFFFFF  # VDB_LABEL_NONE
MASK_MAX_TERMS = 8       # VDB_MASK_MAX_TERMS
TERM_NEGATE = 1          # VDB_TERM_NEGATE
TERM_NONE = 2            # VDB_TERM_NONE
MASK_MAX_SET_BITS = 1 << 27  # VDB_MASK_MAX_SET_BITS: bitmap bits per library call
MASK_MAX_CLAUSES = 64    # VDB_MASK_MAX_CLAUSES

# terms no row satisfies, whatever the columns hold: two different codes asked of one column
NOTHING = ((0, 0), (0, 1))

_UNHASHABLE = object()  # stands in for row values a dictionary cannot hold (they equal no pattern value the codec accepts)


class LabelTerm:
    """One set / range term of a device-built mask (vdb_mask_create_where_sets): a frozen, hashable value.  A row whose label in
    `column` is v matches when v is LABEL_NONE: iff `none` (negate never inverts this case); otherwise: inside = lo <= v <= hi and (codes
    is None or v in codes), and the row matches iff inside != negate.  `codes`: an iterable of codes -- lo / hi default to its min / max;
    with no codes and no bounds the term is the empty range (lo = 1, hi = 0): nothing, or with negate every labelled row.  Without
    `codes` the term is the plain range [lo, hi] and carries no bitmap."""
    __slots__ = ("column", "lo", "hi", "negate", "none", "codes")

    def __init__(self, column, lo=None, hi=None, negate=False, none=False, codes=None):
        cs = None if codes is None else tuple(sorted({int(c) for c in codes}))
        if cs is not None and any(not 0 <= c < LABEL_NONE for c in cs):
            raise ValueError("LabelTerm: codes are u32 below LABEL_NONE")
        if cs:
            lo = cs[0] if lo is None else int(lo)
            hi = cs[-1] if hi is None else int(hi)
            if not lo <= cs[0] <= cs[-1] <= hi:
                raise ValueError(f"LabelTerm: codes {cs[0]} .. {cs[-1]} outside [{lo}, {hi}]")
        elif cs is not None or (lo is None and hi is None):  # an empty set, whatever the bounds: the empty range
            lo, hi, cs = 1, 0, None
        elif lo is None or hi is None:
            raise ValueError("LabelTerm: give both lo and hi, or codes")
        lo, hi, column = int(lo), int(hi), int(column)
        if not (0 <= lo < 2 ** 32 and 0 <= hi < 2 ** 32 and 0 <= column < 2 ** 32):
            raise ValueError(f"LabelTerm({column}, {lo}, {hi}): column, lo and hi are u32")
        for k, v in (("column", column), ("lo", lo), ("hi", hi), ("negate", bool(negate)), ("none", bool(none)), ("codes", cs)):
            object.__setattr__(self, k, v)

    def __setattr__(self, k, v):
        raise AttributeError("LabelTerm is frozen")

    def _key(self):
        return (self.column, self.lo, self.hi, self.negate, self.none, self.codes)

    def __eq__(self, other):
        return isinstance(other, LabelTerm) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return f"LabelTerm({self.column}, {self.lo}, {self.hi}, negate={self.negate}, none={self.none}, codes={self.codes})"

    @property
    def flags(self) -> int:
        return (TERM_NEGATE if self.negate else 0) | (TERM_NONE if self.none else 0)

    @property
    def set_bits(self) -> int:
        """bits of the term's bitmap, whole 64-bit words (0: no bitmap)"""
        return 0 if self.codes is None else (self.hi - self.lo + 64) // 64 * 64

    def bitmap(self) -> np.ndarray:
        """the u64 words of the term's bitmap, bit j = code lo + j (no words without `codes`)"""
        if self.codes is None:
            return np.zeros(0, dtype=np.uint64)
        if len(self.codes) <= 64:  # a handful of codes: plain integers beat the array round trip
            words = [0] * (self.set_bits // 64)
            for c in self.codes:
                words[(c - self.lo) >> 6] |= 1 << ((c - self.lo) & 63)
            return np.array(words, dtype=np.uint64)
        bits = np.zeros(self.set_bits, dtype=np.uint8)
        bits[np.asarray(self.codes, dtype=np.int64) - self.lo] = 1
        return np.packbits(bits, bitorder="little").view(np.uint64)

    def select(self, values) -> np.ndarray:
        """the match over an array of u32 labels, in numpy (the arithmetic of k_mask_rows<MaskAll>, for hosts and tests)"""
        v = np.asarray(values, dtype=np.uint32).astype(np.int64)
        inside = (v >= self.lo) & (v <= self.hi)
        if self.codes is not None:
            inside &= np.isin(v, np.asarray(self.codes, dtype=np.int64))
        return np.where(v == LABEL_NONE, self.none, inside != self.negate)

    def complement(self) -> "LabelTerm":
        """the term that matches exactly the rows this one does not: `negate` and `none` toggled (negate never touches the rows without
        a value, so their bit is toggled on its own)"""
        return LabelTerm(self.column, self.lo, self.hi, negate=not self.negate, none=not self.none, codes=self.codes)

    def matches_nothing(self) -> bool:
        """True when no label value can match: the empty range, plain"""
        return self.lo > self.hi and not self.negate and not self.none

    def matches_everything(self) -> bool:
        return self.lo > self.hi and self.negate and self.none

    @staticmethod
    def of(term) -> "LabelTerm":
        """a LabelTerm as it is; an equality term (column, code) of make_mask_where as its documented equivalent: {lo = hi = code}, and
        (column, LABEL_NONE) as {lo = 1, hi = 0, none}"""
        if isinstance(term, LabelTerm):
            return term
        c, code = term
        return LabelTerm(c, 1, 0, none=True) if int(code) == LABEL_NONE else LabelTerm(c, int(code), int(code))


# ---- predicates: pattern values beyond `str` (equality) and None (key missing) -------------------------------------------------------
class _Pred:
    """frozen and hashable, so a pattern that holds predicates still keys the mask cache as frozenset(pattern.items())"""
    __slots__ = ("_k",)

    def __init__(self, *k):
        object.__setattr__(self, "_k", k)

    def __setattr__(self, k, v):
        raise AttributeError("predicates are frozen")

    def __eq__(self, other):
        return type(other) is type(self) and self._k == other._k

    def __hash__(self):
        return hash((type(self).__name__, self._k))

    def __repr__(self):
        return f"{type(self).__name__}{self._k!r}"


class In(_Pred):
    """x in values; None may be a member: rows without the key match then"""
    __slots__ = ()

    def __init__(self, values):
        super().__init__(frozenset(values))

    @property
    def values(self):
        return self._k[0]


class NotIn(In):
    """x not in values (rows without the key match unless None is a member)"""
    __slots__ = ()


class Ne(_Pred):
    """x != v; rows without the key match, as negating m.get(k) == v would have it"""
    __slots__ = ()

    def __init__(self, v):
        hash(v)
        super().__init__(v)


class Exists(_Pred):
    """(x is not None) == flag"""
    __slots__ = ()

    def __init__(self, flag=True):
        super().__init__(bool(flag))


def _bound_kind(b, who):
    if isinstance(b, bool) or not isinstance(b, (str, int, float)):
        raise TypeError(f"{who}: a bound is a str (string order) or an int / float (numeric order), not {type(b).__name__}")
    return "s" if isinstance(b, str) else "n"


class _Order(_Pred):
    """A str bound compares by Python string order and matches only when x is a str.  An int / float bound compares numerically and
    matches only when x is a str that float(x) parses to a non-NaN number.  A missing key never matches; a NaN bound matches nothing."""
    __slots__ = ()
    _op = None

    def __init__(self, bound):
        _bound_kind(bound, type(self).__name__)
        super().__init__(bound)

    def _cmp(self, x):
        return type(self)._op(x, self._k[0])

    def _kind(self):
        return "s" if isinstance(self._k[0], str) else "n"


class Lt(_Order):
    __slots__ = ()
    _op = staticmethod(lambda x, b: x < b)


class Le(_Order):
    __slots__ = ()
    _op = staticmethod(lambda x, b: x <= b)


class Gt(_Order):
    __slots__ = ()
    _op = staticmethod(lambda x, b: x > b)


class Ge(_Order):
    __slots__ = ()
    _op = staticmethod(lambda x, b: x >= b)


class Between(_Order):
    """lo <= x <= hi, both ends included; the two bounds are both strings or both numbers"""
    __slots__ = ()

    def __init__(self, lo, hi):
        if _bound_kind(lo, "Between") != _bound_kind(hi, "Between"):
            raise TypeError("Between: the two bounds are both strings or both numbers")
        _Pred.__init__(self, lo, hi)

    def _cmp(self, x):
        return self._k[0] <= x <= self._k[1]


def matches(value_or_pred, x) -> bool:
    """THE definition of a pattern entry against x = metadata.get(key): a plain value is `x == value` (what the host loop always did),
    a predicate what its class says."""
    p = value_or_pred
    if not isinstance(p, _Pred):
        return bool(x == p)
    if isinstance(p, In):  # (NotIn is a subclass)
        try:
            inside = x in p.values
        except TypeError:  # x cannot be hashed: it equals no member
            inside = False
        return inside != isinstance(p, NotIn)
    if isinstance(p, Ne):
        return bool(x != p._k[0])
    if isinstance(p, Exists):
        return (x is not None) == p._k[0]
    if not isinstance(x, str):
        return False
    if p._kind() == "n":
        try:
            x = float(x)
        except ValueError:
            return False
        if math.isnan(x):
            return False
    return bool(p._cmp(x))  # (a comparison with a NaN bound is False)


def is_predicate(v) -> bool:
    return isinstance(v, _Pred)


def has_predicates(pattern) -> bool:
    return any(isinstance(v, _Pred) for v in pattern.values())


# ---- filter expressions: patterns joined by OR, AND and NOT ---------------------------------------------------------------------------
def _leaf_key(e):
    """what an operand contributes to its parent's identity: a pattern dict as frozenset(items) -- the key the mask cache files a
    pattern under -- an expression as itself"""
    if isinstance(e, _Expr):
        return e
    if isinstance(e, dict):
        return frozenset(e.items())
    raise TypeError(f"a filter expression is built from pattern dicts, AnyOf, AllOf and Not, not {type(e).__name__}")


class _Expr:
    """frozen and hashable, so an expression keys the mask cache; operand order matters to equality, not to meaning"""
    __slots__ = ("exprs", "_k")

    def __init__(self, *exprs):
        k = tuple(_leaf_key(e) for e in exprs)
        hash(k)  # (a pattern value that cannot be hashed fails here, not inside a search)
        object.__setattr__(self, "exprs", tuple(dict(e) if isinstance(e, dict) else e for e in exprs))
        object.__setattr__(self, "_k", k)

    def __setattr__(self, k, v):
        raise AttributeError("filter expressions are frozen")

    def __eq__(self, other):
        return type(other) is type(self) and self._k == other._k

    def __hash__(self):
        return hash((type(self).__name__, self._k))

    def __repr__(self):
        return f"{type(self).__name__}({', '.join(repr(e) for e in self.exprs)})"


class AnyOf(_Expr):
    """matches when ANY operand matches; AnyOf() matches nothing"""
    __slots__ = ()


class AllOf(_Expr):
    """matches when EVERY operand matches; AllOf() matches everything"""
    __slots__ = ()


class Not(_Expr):
    """matches when its operand does not"""
    __slots__ = ()

    def __init__(self, expr):
        super().__init__(expr)

    @property
    def expr(self):
        return self.exprs[0]


def is_expression(f) -> bool:
    return isinstance(f, _Expr)


def filter_key(f):
    """the hashable identity of a filter: frozenset(items) of a pattern, an expression as itself"""
    return _leaf_key(f)


def filter_patterns(f) -> list:
    """the pattern dicts of a filter, left to right (a pattern: itself)"""
    if isinstance(f, dict):
        return [f]
    return [p for e in f.exprs for p in filter_patterns(e)]


def filter_keys(f) -> frozenset:
    """the metadata keys a filter names: a pattern's keys, for an expression the union over filter_patterns.  `f` may also be a key of the
    mask cache (filter_key: frozenset(items) of a pattern, an expression as itself).  A write that changes the values of some keys makes
    stale exactly the cached masks whose filter_keys intersect them -- the mask of {} names no key and survives every such write."""
    if isinstance(f, frozenset):
        return frozenset(k for k, _ in f)
    return frozenset(k for p in filter_patterns(f) for k in p)


def stale_filters(cache, changed_keys) -> list:
    """the entries of a mask cache (a dict keyed by filter_key) that a write to the metadata keys `changed_keys` makes stale"""
    changed = frozenset(changed_keys)
    return [key for key in cache if filter_keys(key) & changed]


def matches_filter(expr, metadata_row) -> bool:
    """THE definition of a filter against one metadata dict: a pattern matches when every entry does (`matches` on
    metadata_row.get(key): what the host loop does), AnyOf is any, AllOf is all, Not is not."""
    if isinstance(expr, dict):
        return all(matches(v, metadata_row.get(k)) for k, v in expr.items())
    if isinstance(expr, AnyOf):
        return any(matches_filter(e, metadata_row) for e in expr.exprs)
    if isinstance(expr, AllOf):
        return all(matches_filter(e, metadata_row) for e in expr.exprs)
    if isinstance(expr, Not):
        return not matches_filter(expr.expr, metadata_row)
    raise TypeError(f"a filter is a pattern dict, AnyOf, AllOf or Not, not {type(expr).__name__}")


def cap_groups(codes_in_order, group_size: int, k: int) -> list[int]:
    """THE host statement of the grouped k-NN's walk (GpuIndex.flat_knn_grouped, k_group_cap): the positions kept from a list of label codes
    given in the query's order -- a position without a label (None or LABEL_NONE) always, a position with code v iff fewer than
    group_size earlier positions carry v -- cut to the first k kept.  The codes may be any hashable values."""
    if int(group_size) < 1:
        raise ValueError("group_size must be at least 1")
    kept: list[int] = []
    seen: dict[object, int] = {}
    if k <= 0:
        return kept
    for pos, c in enumerate(codes_in_order):
        if isinstance(c, np.integer):
            c = int(c)
        if c is not None and c != LABEL_NONE:
            n = seen.get(c, 0)
            if n >= group_size:
                continue
            seen[c] = n + 1
        kept.append(pos)
        if len(kept) >= k:
            break
    return kept


def _f32_order_key(d) -> int:
    """the knn order of an f32 as an integer: -0 == +0, every NaN equal and last (f32_orderable of the library)"""
    u = int(np.array(np.float32(d) + np.float32(0.0), dtype=np.float32).view(np.uint32))
    if (u & 0x7FFFFFFF) > 0x7F800000:
        u = 0x7FC00000
    return (~u & 0xFFFFFFFF) if u & 0x80000000 else (u | 0x80000000)


def fuse_groups(lists, k: int, mode: str = "rrf", weights=None, c: float = 60.0, trunc_len=None):
    """THE host statement of the document-level fusion (GpuIndex.flat_knn_fused_groups, k_fuse_groups), for keys without a label column.
    `lists`: per sub-query (ids, distances, values) in rank order -- values[i] is the group of entry i, any hashable; None: the row is a
    group of its own.  Per list a group counts at its first entry; "rrf": the f32 fold of weight / ((rank among the list's groups + 1) + c),
    descending; "min": the smallest such distance; "sum": the fold over every non-empty list of that distance, or of the list's last
    distance where the list lacks the group; both ascending.  The representative of a group is its entry of the smallest (distance,
    list); ties go to the lower representative.  A list of trunc_len entries or more is a truncated one (None: none is).
    -> (representative ids, scores as float32, exact) cut at k; the arithmetic is the device's, rounding for rounding."""
    if mode not in ("rrf", "min", "sum"):
        raise ValueError(f"fusion {mode!r}: 'rrf', 'min' or 'sum'")
    f32 = np.float32
    c = f32(c)
    table: dict[object, list] = {}  # group -> [accumulator, representative id, its distance, the list that touched it last]
    prefix = f32(0.0)               # "sum": the fold of the last distances of the non-empty lists so far
    trunc_keys = []
    with np.errstate(all="ignore"):
        for s, (ids, dists, values) in enumerate(lists):
            if len(ids) == 0:
                continue
            f_s = f32(dists[len(ids) - 1])
            if trunc_len is not None and len(ids) >= trunc_len:
                trunc_keys.append(_f32_order_key(f_s))
            w = f32(1.0) if weights is None else f32(weights[s])
            rank = 0
            for i, d, v in zip(ids, dists, values):
                g = ("r", int(i)) if v is None else ("l", v)
                e = table.get(g)
                if e is not None and e[3] == s:
                    continue  # not the group's first entry in this list
                d = f32(d)
                if e is None:
                    e = table[g] = [prefix if mode == "sum" else f32(0.0), int(i), d, s]
                else:
                    e[3] = s
                    if _f32_order_key(d) < _f32_order_key(e[2]):
                        e[1], e[2] = int(i), d
                if mode == "rrf":
                    den = f32(f32(rank + 1) + c)
                    e[0] = f32(e[0] + f32(w / den))
                elif mode == "sum":
                    e[0] = f32(e[0] + d)
                rank += 1
            if mode == "sum":
                for e in table.values():
                    if e[3] != s:
                        e[0] = f32(e[0] + f_s)
                prefix = f32(prefix + f_s)
        nan = np.array(0x7FC00000, dtype=np.uint32).view(np.float32)[()]
        scored = []
        for e in table.values():
            score = e[2] if mode == "min" else (nan if mode == "sum" and np.isnan(e[0]) else e[0])
            scored.append((_f32_order_key(-score if mode == "rrf" else score), e[1], score))
    scored.sort(key=lambda t: t[:2])
    k = max(int(k), 0)
    exact = not trunc_keys and k > 0  # (k == 0: nothing is ranked, and `exact` is 0, as the library answers)
    if trunc_keys and mode == "min" and 0 < k <= len(scored):
        exact = scored[k - 1][0] < min(trunc_keys)
    top = scored[:k]
    return np.array([t[1] for t in top], dtype=np.uint64), np.array([t[2] for t in top], dtype=np.float32), int(exact)


class LabelCodec:
    def __init__(self, max_columns: int = LABEL_COLUMNS, max_terms: int = MASK_MAX_TERMS):
        self.max_columns = int(max_columns)
        self.max_terms = int(max_terms)
        self.columns: dict[str, int] = {}       # key -> column, in order of first use
        self.codes: list[dict[object, int]] = []  # per column: value -> code

    def column_of(self, key):
        """the key's column, or None when it has none (yet)"""
        return self.columns.get(key)

    def keys(self) -> list[str]:
        """the keys that have a column, in column order"""
        return list(self.columns)

    @staticmethod
    def _value_ok(v) -> bool:
        return v is None or isinstance(v, str)

    def expressible(self, pattern) -> bool:
        """True when the pattern can be evaluated over label columns: at most max_terms keys, every key has a column or can still get
        one, every value a string (or None: the key is missing) or a predicate.  Assigns nothing."""
        if len(pattern) > self.max_terms or not all(self._value_ok(v) or isinstance(v, _Pred) for v in pattern.values()):
            return False
        new = sum(1 for k in pattern if k not in self.columns)
        return len(self.columns) + new <= self.max_columns

    def missing(self, pattern) -> list[str]:
        """the pattern's keys that have no column yet, in pattern order"""
        return [k for k in pattern if k not in self.columns]

    def assign(self, pattern):
        """gives every key of an expressible pattern a column; returns the keys that got one now (their columns are still to be
        encoded: encode_rows), or None -- and assigns nothing -- when the pattern is not expressible"""
        if not self.expressible(pattern):
            return None
        new = self.missing(pattern)
        for k in new:
            self.columns[k] = len(self.codes)
            self.codes.append({})
        return new

    def unassign(self, keys) -> None:
        """takes the columns of `keys` back: they must be the most recently assigned ones (an assignment whose encoding failed)"""
        for k in reversed(list(keys)):
            assert self.columns[k] == len(self.codes) - 1, "only the last columns can be taken back"
            del self.columns[k]
            self.codes.pop()

    def encode_rows(self, key, metadata) -> np.ndarray:
        """the u32 codes of `metadata` (a sequence of dicts) in the key's column, interning values not seen before.  Encoding a table in
        pieces, in row order, gives what encoding it at once gives."""
        table = self.codes[self.columns[key]]
        out = np.empty(len(metadata), dtype=np.uint32)
        for i, m in enumerate(metadata):
            v = m.get(key)
            if v is None:
                out[i] = LABEL_NONE
                continue
            try:
                c = table.get(v)
            except TypeError:
                v, c = _UNHASHABLE, table.get(_UNHASHABLE)
            if c is None:
                c = table[v] = len(table)
            out[i] = c
        return out

    def encode_value(self, key, v) -> int:
        """the code of ONE value in the key's column, interning a value not seen before; None is LABEL_NONE.  An unhashable value takes
        encode_rows' stand-in: encode_value(k, m.get(k)) == encode_rows(k, [m])[0] for every metadata dict m."""
        if v is None:
            return LABEL_NONE
        table = self.codes[self.columns[key]]
        try:
            c = table.get(v)
        except TypeError:
            v, c = _UNHASHABLE, table.get(_UNHASHABLE)
        if c is None:
            c = table[v] = len(table)
        return c

    def value_codes(self, key):
        """(values, codes) of the key's dictionary, entry for entry -- what decodes a count per code (GpuIndex.label_counts) into a count
        per value -- or None when the key has no column, or when its dictionary holds the stand-in for values it could not hold (a
        count under that code is a count of several different values: the host has to look at the rows)"""
        col = self.columns.get(key)
        if col is None or _UNHASHABLE in self.codes[col]:
            return None
        table = self.codes[col]
        return list(table), list(table.values())

    def terms(self, pattern):
        """the (column, code) terms of a pattern whose keys all have columns: a list (empty for the empty pattern), NOTHING when a value
        was never seen in its column (the dictionary does not grow), None when the pattern is not expressible or a key has no column"""
        if len(pattern) > self.max_terms:
            return None
        out = []
        nothing = False
        for k, v in pattern.items():
            col = self.columns.get(k)
            if col is None or not self._value_ok(v):
                return None
            if v is None:
                out.append((col, LABEL_NONE))
                continue
            code = self.codes[col].get(v)
            if code is None:
                nothing = True
            else:
                out.append((col, code))
        return list(NOTHING) if nothing else out

    def _entry_term(self, k, p):
        """the one LabelTerm of a pattern entry (key k, value or predicate p) over the key's column -- the empty range when it can match
        no row -- or None: the key has no column, or p is neither str, None nor a predicate"""
        col = self.columns.get(k)
        if col is None or not (self._value_ok(p) or isinstance(p, _Pred)):
            return None
        table = self.codes[col]
        negate = False
        if p is None:
            return LabelTerm.of((col, LABEL_NONE))
        if isinstance(p, str):
            return LabelTerm.of((col, table[p])) if p in table else LabelTerm(col)
        if isinstance(p, In):
            codes, none = [table[v] for v in p.values if v is not None and v in table], None in p.values
            negate = isinstance(p, NotIn)
        elif isinstance(p, Ne):
            v = p._k[0]
            codes, none, negate = [table[v]] if v is not None and v in table else [], v is None, True
        elif isinstance(p, Exists):
            codes, none, negate = [], True, p._k[0]  # the rows without a value, or their complement
        else:
            codes, none = [c for v, c in table.items() if matches(p, v)], False
        if negate:
            none = not none  # the complement within "rows without a value" too
        if codes and max(codes) - min(codes) + 1 == len(set(codes)):
            return LabelTerm(col, min(codes), max(codes), negate=negate, none=none)  # a run of codes: a range, no bitmap
        return LabelTerm(col, negate=negate, none=none, codes=codes)

    def compile(self, pattern):
        """the LabelTerm list of a pattern that may hold predicates, one term per key: a list (empty for the empty pattern), NOTHING
        when some entry can match no row (an In whose values were all never seen, an unseen plain value), None when the pattern is not
        expressible: a key without a column, more than max_terms keys, a plain value that is neither str nor None, a bitmap span over
        MASK_MAX_SET_BITS.  The dictionary never grows.  In / NotIn / Ne are dictionary look-ups; the order predicates evaluate
        `matches` over the column's dictionary entries: O(distinct values of the key), not O(rows) -- a column of unique ids makes that
        as slow as the host loop, and still correct.  A row value the dictionary could not hold (the _UNHASHABLE entry) needs no
        special case: it equals no pattern value and is no str."""
        if len(pattern) > self.max_terms:
            return None
        out = []
        nothing = False
        for k, p in pattern.items():
            term = self._entry_term(k, p)
            if term is None:
                return None
            if term.matches_nothing():
                nothing = True
                continue
            out.append(term)
        if sum(t.set_bits for t in out) > MASK_MAX_SET_BITS:  # (one library call must be able to carry the pattern)
            return None
        return NOTHING if nothing else out

    def compile_any(self, expr, max_clauses: int = MASK_MAX_CLAUSES):
        """the disjunctive normal form of a filter (a pattern dict, AnyOf, AllOf, Not, nested) over the label columns: a list of clauses,
        each a list of LabelTerm -- a row matches when it matches every term of some clause.  [] means nothing matches, a clause []
        every row.  None when the filter is not expressible: a key without a column, a value that is not a str, None or a predicate, a
        normal form over max_clauses clauses (at any stage of the expansion), a clause over max_terms terms, bitmaps over
        MASK_MAX_SET_BITS.  NOT is pushed to the terms by De Morgan and LabelTerm.complement, which is exact.  A clause that holds a
        term no row can match is dropped, a term every row matches is left out, equal terms and equal clauses are kept once.  The
        dictionary never grows."""
        clauses = self._dnf(expr, False, max_clauses)
        if clauses is None:
            return None
        if sum(t.set_bits for c in clauses for t in c) > MASK_MAX_SET_BITS:  # (one library call must be able to carry the filter)
            return None
        return [list(c) for c in clauses]

    def _clauses(self, clauses, max_clauses):
        """tidies a list of clauses (tuples of terms): see compile_any; None when a limit is passed"""
        out, seen = [], set()
        for c in clauses:
            if any(t.matches_nothing() for t in c):
                continue
            c = tuple(dict.fromkeys(t for t in c if not t.matches_everything()))
            if not c:
                return [()]  # a clause every row matches: so does the filter
            if len(c) > self.max_terms:
                return None
            if c not in seen:
                seen.add(c)
                out.append(c)
        return out if len(out) <= max_clauses else None

    def _dnf(self, e, negated, max_clauses):
        if isinstance(e, dict):
            terms = [self._entry_term(k, p) for k, p in e.items()]
            if any(t is None for t in terms):
                return None
            # a pattern is the AND of its entries; negated, the OR of their complements
            return self._clauses([(t.complement(),) for t in terms] if negated else [tuple(terms)], max_clauses)
        if isinstance(e, Not):
            return self._dnf(e.expr, not negated, max_clauses)
        if not isinstance(e, (AnyOf, AllOf)):
            return None
        parts = []
        for sub in e.exprs:
            d = self._dnf(sub, negated, max_clauses)
            if d is None:
                return None
            parts.append(d)
        if isinstance(e, AnyOf) != negated:  # an OR: the clauses of all operands
            return self._clauses([c for d in parts for c in d], max_clauses)
        acc = [()]  # an AND: the products of one clause per operand, operand by operand
        for d in parts:
            acc = self._clauses([a + c for a in acc for c in d], max_clauses)
            if acc is None:
                return None
        return acc


__all__ = ["LabelCodec", "LabelTerm", "LABEL_COLUMNS", "LABEL_NONE", "MASK_MAX_TERMS", "MASK_MAX_SET_BITS", "MASK_MAX_CLAUSES", "NOTHING", "TERM_NEGATE",
           "TERM_NONE", "In", "NotIn", "Ne", "Exists", "Lt", "Le", "Gt", "Ge", "Between", "matches", "is_predicate", "has_predicates",
           "AnyOf", "AllOf", "Not", "matches_filter", "is_expression", "filter_key", "filter_patterns", "filter_keys", "stale_filters",
           "cap_groups"]
