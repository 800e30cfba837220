"""LabelCodec -- the host-side dictionary between metadata (key -> value dicts) and the integer label columns of an index.

Pure Python: no GPU and no library.  The codec decides WHICH metadata keys become label columns and which code a value gets; the
index holds the codes (GpuIndex.set_labels) and evaluates patterns over them (GpuIndex.make_mask_where).

  * Keys are assigned to columns LAZILY, in order of first use in a filter pattern, at most LABEL_COLUMNS of them.  Metadata of a
    retrieval table carries ids and whole text bodies: a key is never interned merely because rows have it.
  * Per column, values are interned to codes 0, 1, 2, .. in order of first appearance; a row without the key (or with None) encodes as
    LABEL_NONE, which is also what a pattern value of None encodes to -- `m.get(k) == v`, the match the host loop makes.
  * A pattern -- every key present with an equal value -- encodes to at most MASK_MAX_TERMS (column, code) terms, or to "matches
    nothing" when one of its values was never seen in its column (without growing the dictionary).
"""
from __future__ import annotations

import numpy as np

LABEL_COLUMNS = 16       # VDB_LABEL_COLUMNS
LABEL_NONE = 0xFFFFFFFF  # VDB_LABEL_NONE
MASK_MAX_TERMS = 8       # VDB_MASK_MAX_TERMS

# terms no row satisfies, whatever the columns hold: two different codes asked of one column
NOTHING = ((0, 0), (0, 1))

_UNHASHABLE = object()  # stands in for row values a dictionary cannot hold (they equal no pattern value the codec accepts)


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
        one, every value a string (or None: the key is missing).  Assigns nothing."""
        if len(pattern) > self.max_terms or not all(self._value_ok(v) for v in pattern.values()):
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


__all__ = ["LabelCodec", "LABEL_COLUMNS", "LABEL_NONE", "MASK_MAX_TERMS", "NOTHING"]
