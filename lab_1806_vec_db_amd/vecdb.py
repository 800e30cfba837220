"""VecDB-shaped host surface over the C ABI (mirror of lab_1806_vec_db.pyi / src/pyo3/mod.rs:55-296).

Scope: this mirrors the reference's table / search semantics so the hot path can sit behind
`db.search() / add() / build_*_index()`; tables live in memory (HBM + host metadata).  Persistence, the
directory lock and the autosave thread (src/database/{mod,thread_save}.rs) are the reference's control
plane and are out of scope -- `dir` is accepted for signature compatibility only.

Semantics reproduced from src/database/metadata_vec_table.rs:
  * add / batch_add clear the PQ table (:64-81); an HNSW graph survives add (examples/test_pyo3.py:19);
  * delete(pattern) clears HNSW and PQ, then swap-removes matches in descending order (:163-187);
  * build_hnsw_index only when currently Flat, M=16, ef_construction=200 unless given (:84-98);
  * build_pq_table: proportion 0.1 default, m = ceil(dim/3) default, n_bits is validated but the table is
    always built with 4 bits (:112-152 -- a reference quirk, kept);
  * search dispatch (:194-212): (ef, pq) -> knn_pq; (ef, no pq) -> knn_with_ef; else knn; then the
    `distance <= upper_bound` filter.

Beyond the reference: search_within(key, query, upper_bound) returns the COMPLETE set inside the bound (exact Flat range search);
search / search_within take `filter`, a metadata pattern matched as delete matches: only matching rows are searched, exactly;
batch_search(key, queries, k, ..., filters) answers a batch of queries, each under a pattern of its own, in one library call.
The keys filter patterns use are kept on the device as integer label columns (labels.py: a key gets a column when a pattern first names
it, one pass over the metadata; add / delete keep the columns in step), and the patterns' row masks are built there
(GpuIndex.make_masks_where); a pattern the columns cannot express (a 17th key, more than 8 keys) is matched on the host as before.
A pattern value may be a predicate of labels.py (In, NotIn, Ne, Exists, Lt, Le, Gt, Ge, Between; labels.matches defines them): such a
pattern is compiled over the columns' dictionaries into set / range terms and its mask is built on the device as well
(GpuIndex.make_masks_where_sets); patterns of plain values keep their path.
A filter may also be an EXPRESSION of labels.py -- AnyOf, AllOf and Not over patterns, nested (labels.matches_filter defines them): its
disjunctive normal form over the label columns (LabelCodec.compile_any) is evaluated on the device in one pass
(GpuIndex.make_masks_where_any); an expression that has no such form (a 17th key, more than 64 clauses) is assembled from the masks of
its operands with GpuIndex.combine_masks.  A pattern dict keeps its path; delete takes a pattern only.
count(key, filter) is the number of matching rows (the mask's count); count_by(key, field, filter) the matching rows per value of a
metadata key, from one pass over the key's label column on the device (GpuIndex.label_counts).
search / batch_search take `group_by`, a metadata key, and `group_size`: at most that many hits per value of the key, nearest first, rows
without the key always kept -- exact, from the Flat rows, in one library call over the key's label column (GpuIndex.flat_knn_grouped).
search / batch_search take `mmr_lambda` and `fetch_k`: maximal marginal relevance, the k hits close to the query and not near-copies of
each other, chosen greedily among the fetch_k nearest -- exact, from the Flat rows, in one library call (GpuIndex.flat_knn_mmr).
search_like / batch_search_like search by EXAMPLE ROWS: the rows a `positive` filter matches, steered away from the rows a `negative` filter
matches, the examples left out of the answer -- the query vector is made on the device, the batch is one library call (GpuIndex.flat_knn_like).
search_fused / batch_search_fused join SEVERAL searches of one question -- several query vectors, or one vector under several filters --
into one ranked answer on the device, by reciprocal rank fusion or by the smallest distance; the batch is one library call
(GpuIndex.flat_knn_fused).  With `group_by` they rank DOCUMENTS, the rows that share a value of a metadata key -- also by the
late-interaction sum, fusion="sum" -- still one library call (GpuIndex.flat_knn_fused_groups).
get(key, filter, limit) returns the vectors and metadata of the matching rows, and every search takes `with_vectors`: the hits' vectors
ride along, all of a call's from one bulk fetch (GpuIndex.get_rows / get_rows_mask); extract_data reads the table with one such call.
update_metadata(key, pattern, changes) / batch_update_metadata change the METADATA of the matching rows in place: row ids, vectors, the
HNSW graph and the PQ table stay, the live label columns are written by one scattered write on the device (GpuIndex.set_labels_mask /
set_labels_rows), and only the cached masks whose filter names a changed key are dropped.
upsert(key, id_field, vec, metadata) / batch_upsert write BY A KEY FIELD: an entry whose value of the field a row carries replaces that row's
vector and metadata in place, the others are appended; get_by(key, field, values) fetches the rows that carry given values.  Both find
their rows with ONE pass over the field's label column whatever the number of values (GpuIndex.label_lookup), not with a mask per value.
"""
from __future__ import annotations

import collections
import threading
from contextlib import contextmanager

import numpy as np

from ._lib import VdbError
from .index import FUSE_MAX_FETCH, LIKE_MAX_EXAMPLES, MMR_MAX_FETCH, ROW_NONE, GpuIndex, RowMask, parse_dist
from .labels import LABEL_NONE, MASK_MAX_SET_BITS, AnyOf, LabelCodec, LabelTerm, Not, cap_groups, filter_key, fuse_groups, filter_patterns, has_predicates, is_expression, stale_filters
from .labels import matches as value_matches

_DIST_STR = {0: "l2sqr", 1: "cosine"}

# _Table.masks_for: the smallest group of uncached one-key patterns on one column that is built by GpuIndex.make_masks_partition instead
# of make_masks_where; None: never.  The masks are the same either way.  The value is the smallest group size of the sweep of
# tools/bench_mask_partition.py (profiles/mask_partition_1M.json) FROM WHICH ON the partition call was the faster of the two: it also won
# at 2 .. 16 codes, by microseconds, and lost at 32, and batches of up to 50 patterns keep the one make_masks_where call they are
# tested to make (docs/DESIGN_flat.md 4.1p has the sweep and the decision).
PARTITION_MIN: int | None = 64

# _Table.match_rows: the smallest group of uncached, plain, one-key patterns on one column whose rows are found by ONE
# GpuIndex.label_lookup call -- the patterns that match at most one row are answered from it, the others join the make_masks_where call --
# instead of a mask per pattern; None: never.  The rows are the same either way.  Never below 64: batches of up to 50 patterns keep the
# one make_masks_where call they are tested to make.  In the sweep behind it, part B of tools/bench_lookup.py
# (profiles/label_lookup_1M.json; docs/DESIGN_flat.md 4.1aa), the lookup won at every group size from 2 to 4096, by 4.5 x to 43 x, so the
# value is that floor.
LOOKUP_MIN: int | None = 64


def _differ(a, b) -> bool:
    """True unless two metadata values are known to be equal (a comparison that raises or answers with no bool counts as a change)"""
    try:
        return bool(a != b)
    except Exception:
        return True


class _RwLock:
    """Reader/writer exclusion of one table: the reference wraps every table in an RwLock -- read guard in search /
    extract_data / len (database/mod.rs:248-256), write guard in add / delete / build_* / clear_* (thread_save.rs:108-113).
    The library's read-side calls are re-entrant on one handle, its write-side calls reallocate HBM buffers under running
    kernels, so a search must never overlap a write on the same table.  Writers are preferred (a waiting writer holds
    back new readers), like std's RwLock on Linux."""

    def __init__(self):
        self._cv = threading.Condition(threading.Lock())
        self._readers = 0
        self._writer = False
        self._writers_waiting = 0

    @contextmanager
    def read(self):
        with self._cv:
            while self._writer or self._writers_waiting:
                self._cv.wait()
            self._readers += 1
        try:
            yield
        finally:
            with self._cv:
                self._readers -= 1
                if self._readers == 0:
                    self._cv.notify_all()

    @contextmanager
    def write(self):
        with self._cv:
            self._writers_waiting += 1
            while self._writer or self._readers:
                self._cv.wait()
            self._writers_waiting -= 1
            self._writer = True
        try:
            yield
        finally:
            with self._cv:
                self._writer = False
                self._cv.notify_all()


class _Table:
    def __init__(self, dim: int, dist: str, device: int):
        self.index = GpuIndex(dim, dist, device)
        self.metadata: list[dict[str, str]] = []
        self.lock = _RwLock()
        self.seed = 0x1806
        # row masks of the filters searched with (search(filter=...)), keyed by labels.filter_key -- frozenset(pattern.items()) of a
        # pattern, an expression as itself: filled under mask_mu by searches (which hold the READ lock, several at a time), closed and
        # cleared by every write under the WRITE lock
        self.masks: dict[object, RowMask] = {}
        self.mask_mu = threading.Lock()
        # which metadata keys are label columns of the index, and the value -> code dictionary of each: changed under the WRITE lock only
        self.codec = LabelCodec()

    def host_match(self, pattern: dict[str, str]) -> np.ndarray:
        """the host loop: a bool per row, True where the metadata holds every key of `pattern` with an equal value -- or, for a
        predicate, a value it accepts (labels.matches)"""
        return np.fromiter((all(value_matches(v, m.get(k)) for k, v in pattern.items()) for m in self.metadata), dtype=np.bool_, count=len(self.metadata))

    def live_terms(self, pattern):
        """the pattern's terms when every key has a label column, else None: (column, code) terms for a pattern of plain values
        (labels.py: terms), LabelTerm set / range terms for one that holds predicates (labels.py: compile)"""
        return self.codec.compile(pattern) if has_predicates(pattern) else self.codec.terms(pattern)

    def device_mask(self, pattern, terms) -> RowMask:
        """the mask of live_terms' terms: plain patterns through make_mask_where, patterns with a predicate through make_mask_where_sets"""
        return self.index.make_mask_where_sets(terms) if has_predicates(pattern) else self.index.make_mask_where(terms)

    def create_columns(self, patterns) -> None:
        """UNDER THE WRITE LOCK: gives the keys of every expressible pattern their label columns -- one pass over the metadata per new
        key to encode it, then set_labels.  Patterns that cannot be expressed are left to the host loop."""
        for p in patterns:
            new = self.codec.assign(p) or []
            for i, k in enumerate(new):
                try:
                    self.index.set_labels(self.codec.column_of(k), self.codec.encode_rows(k, self.metadata))
                except BaseException:
                    self.codec.unassign(new[i:])  # a column that was not written is no column: the host loop answers
                    raise

    def prepare(self, patterns) -> None:
        """BEFORE the read lock of a search is taken: a key a pattern names for the first time gets its column under the WRITE lock --
        readers build masks from the columns and read the codec's dictionaries, so nobody may be reading while one is made.  Two
        threads that first-use a key at once both come here; the second finds the column made.  The check itself only reads the
        codec, which changes under the write lock alone: a stale answer costs a useless turn through the lock, nothing else."""
        patterns = [p for f in patterns for p in filter_patterns(f)]  # (an expression: its patterns, each as if searched with alone)
        if all(not self.codec.missing(p) or not self.codec.expressible(p) for p in patterns):
            return
        with self.lock.write():
            self.create_columns(patterns)

    def mask_for(self, pattern: dict[str, str]) -> RowMask:
        """the mask of the rows whose metadata holds every key of `pattern` with an equal value (an empty pattern: every row): built on
        the device from the label columns when every key of the pattern has one, else from the host loop"""
        with self.mask_mu:
            return self.mask_locked(pattern)

    def mask_locked(self, f) -> RowMask:
        """UNDER mask_mu: the cached mask of a pattern or an expression, made on first use"""
        key = filter_key(f)
        mk = self.masks.get(key)
        if mk is None:
            if is_expression(f):
                self.expr_masks([f])
                return self.masks[key]
            terms = self.live_terms(f)
            if terms is not None:
                mk = self.masks[key] = self.device_mask(f, terms)
            else:
                mk = self.masks[key] = self.index.make_mask(self.host_match(f))
        return mk

    def expr_masks(self, exprs) -> None:
        """UNDER mask_mu: caches the masks of the expressions not cached yet.  The ones with a normal form over the label columns
        (LabelCodec.compile_any) are built by ONE make_masks_where_any call (more than one only when their bitmaps together pass the
        library's MASK_MAX_SET_BITS per call); every other one is assembled from its operands' masks (assemble)."""
        todo: dict[object, list] = {}
        rest = []
        for e in exprs:
            if e in self.masks or e in todo:
                continue
            clauses = self.codec.compile_any(e)
            if clauses is not None:
                todo[e] = clauses
            elif e not in rest:
                rest.append(e)
        batch, bits = [], 0
        for e in list(todo) + [None]:
            need = 0 if e is None else sum(t.set_bits for c in todo[e] for t in c)
            if batch and (e is None or bits + need > MASK_MAX_SET_BITS):
                for be, mk in zip(batch, self.index.make_masks_where_any([todo[be] for be in batch])):
                    self.masks[be] = mk
                batch, bits = [], 0
            if e is not None:
                batch.append(e)
                bits += need
        for e in rest:
            self.masks[e] = self.assemble(e)

    def assemble(self, e) -> RowMask:
        """UNDER mask_mu: the mask of an expression the columns cannot express, from the masks of its operands -- each cached under
        its own key, built on the device where it can be and by the host loop where not -- joined with combine_masks, eight at a
        time; a Not operand is its operand's mask, complemented inside the join"""
        if isinstance(e, Not):
            return self.index.combine_masks("and", [self.mask_locked(e.expr)], [True])
        op = "or" if isinstance(e, AnyOf) else "and"
        self.expr_masks([y for y in (x.expr if isinstance(x, Not) else x for x in e.exprs) if is_expression(y)])  # (one call for those the columns express)
        parts = [(self.mask_locked(x.expr), True) if isinstance(x, Not) else (self.mask_locked(x), False) for x in e.exprs]
        acc = None  # the join of the operands so far: an intermediate mask of this call, closed once it has been read
        while parts:
            take = 8 if acc is None else 7
            head, parts = parts[:take], parts[take:]
            if acc is not None:
                head.insert(0, (acc, False))
            nxt = self.index.combine_masks(op, [m for m, _ in head], [inv for _, inv in head])
            if acc is not None:
                acc.close()
            acc = nxt
        return acc

    def masks_for(self, patterns) -> list[RowMask]:
        """mask_for for many patterns: the ones not cached yet whose keys all have columns are built by ONE make_masks_where call for
        the patterns of plain values and ONE make_masks_where_sets call for the ones that hold predicates (more than one only when
        their bitmaps together pass the library's MASK_MAX_SET_BITS per call).  Among the plain ones, those of exactly one (column,
        code) term are grouped by column first, and a group of at least PARTITION_MIN goes to ONE make_masks_partition call: the
        same masks from one read of the column."""
        with self.mask_mu:
            self.expr_masks([p for p in patterns if is_expression(p)])  # expressions: one make_masks_where_any call of their own
            todo: dict[frozenset, list] = {}
            todo_sets: dict[frozenset, list] = {}
            for p in patterns:
                if is_expression(p):
                    continue
                key = frozenset(p.items())
                if key not in self.masks and key not in todo and key not in todo_sets:
                    terms = self.live_terms(p)
                    if terms is not None:
                        (todo_sets if has_predicates(p) else todo)[key] = terms
            if todo and PARTITION_MIN is not None:  # one-term patterns, by column: a large enough group is ONE read of its column
                groups: dict[int, list] = {}
                for key, terms in todo.items():
                    if len(terms) == 1:
                        groups.setdefault(terms[0][0], []).append(key)
                for col, keys in groups.items():
                    if len(keys) >= PARTITION_MIN:  # (different patterns on one key have different values, so different codes)
                        for key, mk in zip(keys, self.index.make_masks_partition(col, [todo[key][0][1] for key in keys])):
                            self.masks[key] = mk
                            del todo[key]
            if todo:
                for key, mk in zip(todo, self.index.make_masks_where(list(todo.values()))):
                    self.masks[key] = mk
            batch, bits = [], 0
            for key in list(todo_sets) + [None]:
                need = 0 if key is None else sum(LabelTerm.of(t).set_bits for t in todo_sets[key])
                if batch and (key is None or bits + need > MASK_MAX_SET_BITS):
                    for bk, mk in zip(batch, self.index.make_masks_where_sets([todo_sets[bk] for bk in batch])):
                        self.masks[bk] = mk
                    batch, bits = [], 0
                if key is not None:
                    batch.append(key)
                    bits += need
        return [self.mask_for(p) for p in patterns]

    def drop_masks(self):
        with self.mask_mu:
            for mk in self.masks.values():
                mk.close()
            self.masks.clear()

    def drop_masks_naming(self, changed_keys) -> None:
        """UNDER THE WRITE LOCK, after a write that changed the VALUES of the metadata keys `changed_keys` and nothing else: closes and
        drops exactly the cached masks whose filter names one of them (labels.filter_keys); every other mask selects the rows it
        selected -- the {} mask included -- and stays, host-built ones too."""
        with self.mask_mu:
            for key in stale_filters(self.masks, changed_keys):
                self.masks.pop(key).close()

    def match_rows(self, patterns) -> list:
        """UNDER THE WRITE LOCK: per pattern the ascending rows it matches, as delete finds them: from a cached or device-built mask
        when the pattern's keys are label columns already (no key gets a column here), from the host loop otherwise; the plain patterns
        not cached yet share ONE make_masks_where call.  Among those, the patterns of exactly one (column, code) term are grouped by
        column first, and a group of at least LOOKUP_MIN distinct codes goes through ONE label_lookup call: a pattern that matches no
        row or one row is answered from it, one that matches more stays with the make_masks_where call."""
        matches: list = [None] * len(patterns)
        todo = []
        with self.mask_mu:
            for i, p in enumerate(patterns):
                mk = self.masks.get(frozenset(p.items()))
                if mk is not None:
                    matches[i] = mk.rows()[1]
                    continue
                terms = self.live_terms(p)
                if terms is None:
                    matches[i] = np.flatnonzero(self.host_match(p))
                elif has_predicates(p):
                    mk = self.device_mask(p, terms)
                    matches[i] = mk.rows()[1]
                    mk.close()
                else:
                    todo.append((i, terms))
        if todo and LOOKUP_MIN is not None:  # one-term patterns, by column and code: a large enough group is ONE read of its column
            groups: dict[int, dict[int, list[int]]] = {}
            for at, (_, terms) in enumerate(todo):
                if len(terms) == 1:
                    groups.setdefault(terms[0][0], {}).setdefault(terms[0][1], []).append(at)
            done = set()
            for col, by_code in groups.items():
                if len(by_code) < LOOKUP_MIN:
                    continue
                first, counts = self.index.label_lookup(col, np.fromiter(by_code, dtype=np.uint64, count=len(by_code)))
                for ats, f, c in zip(by_code.values(), first.tolist(), counts.tolist()):
                    if c <= 1:  # (more rows than one: the pattern's mask lists them)
                        for at in ats:
                            matches[todo[at][0]] = np.array([f] if c else [], dtype=np.uint32)
                        done.update(ats)
            todo = [x for at, x in enumerate(todo) if at not in done]
        if todo:
            for (i, _), mk in zip(todo, self.index.make_masks_where([terms for _, terms in todo])):
                matches[i] = mk.rows()[1]
                mk.close()
        return matches

    def find_values(self, field: str, values):
        """UNDER THE TABLE'S LOCK: (first, counts, rows_of) for the DISTINCT hashable `values` of the metadata key `field` (None: the rows
        without the key) -- counts[j] = the rows whose metadata carries values[j], first[j] = the lowest of them (ROW_NONE: none),
        both uint64.  With a usable label column (LabelCodec.value_codes): values the dictionary has never seen match nothing and do not
        grow it, the others go through ONE label_lookup call, and rows_of is None.  Otherwise -- no column (a 17th key), or a dictionary
        that holds the stand-in for unhashable values -- ONE pass over the metadata builds rows_of: value -> its ascending rows."""
        first = np.full(len(values), ROW_NONE, dtype=np.uint64)
        counts = np.zeros(len(values), dtype=np.uint64)
        if self.codec.value_codes(field) is not None:
            col = self.codec.column_of(field)
            table = self.codec.codes[col]
            known = [(j, LABEL_NONE if v is None else table[v]) for j, v in enumerate(values) if v is None or v in table]
            if known:
                at = [j for j, _ in known]
                first[at], counts[at] = self.index.label_lookup(col, np.array([c for _, c in known], dtype=np.uint64))
            return first, counts, None
        rows_of: dict[object, list[int]] = {v: [] for v in values}
        for r, m in enumerate(self.metadata):
            v = m.get(field)
            try:
                hit = rows_of.get(v)
            except TypeError:  # (an unhashable row value equals no value asked for)
                continue
            if hit is not None:
                hit.append(r)
        for j, v in enumerate(values):
            if rows_of[v]:
                first[j], counts[j] = rows_of[v][0], len(rows_of[v])
        return first, counts, rows_of

    def next_seed(self) -> int:
        self.seed = (self.seed * 6364136223846793005 + 1442695040888963407) & ((1 << 64) - 1)
        return self.seed


class VecDB:
    def __init__(self, dir: str = "", device: int = 0) -> None:
        self.dir = dir
        self.device = device
        self._tables: dict[str, _Table] = {}
        self._mu = threading.Lock()

    # ---- table management (in memory) -----------------------------------------------------------------
    def create_table_if_not_exists(self, key: str, dim: int, dist: str = "cosine") -> bool:
        parse_dist(dist)  # ValueError on a bad name (pyo3/mod.rs:15-22)
        with self._mu:
            if key in self._tables:
                return False
            self._tables[key] = _Table(dim, dist, self.device)
            return True

    def _t(self, key: str) -> _Table:
        try:
            return self._tables[key]
        except KeyError:
            raise RuntimeError(f"Table {key} not found") from None

    def get_len(self, key: str) -> int:
        t = self._t(key)
        with t.lock.read():
            return len(t.index)

    def get_dim(self, key: str) -> int:
        return self._t(key).index.dim

    def get_dist(self, key: str) -> str:
        return _DIST_STR[self._t(key).index.dist]

    def delete_table(self, key: str) -> bool:
        with self._mu:
            t = self._tables.pop(key, None)
        if t is None:
            return False
        with t.lock.write():  # wait for searches still running on the table
            t.drop_masks()
            t.index.close()
        return True

    def get_all_keys(self) -> list[str]:
        return sorted(self._tables)

    def contains_key(self, key: str) -> bool:
        return key in self._tables

    def get_cached_tables(self) -> list[str]:
        return self.get_all_keys()

    def contains_cached(self, key: str) -> bool:
        return key in self._tables

    def remove_cached_table(self, key: str) -> None:
        return None  # nothing is spilled to disk in this mirror

    def force_save(self) -> None:
        return None

    # ---- writes ---------------------------------------------------------------------------------------------
    def add(self, key: str, vec, metadata: dict[str, str]) -> None:
        self.batch_add(key, [vec], [metadata])

    def batch_add(self, key: str, vec_list, metadata_list) -> None:
        t = self._t(key)
        rows = np.asarray(vec_list, dtype=np.float32)
        if rows.ndim != 2 or rows.shape[1] != t.index.dim:  # database/mod.rs:427-429,445-447
            raise RuntimeError(f"Dimension mismatch: table dim {t.index.dim}, got {rows.shape}")
        if len(metadata_list) != rows.shape[0]:
            raise RuntimeError("vec_list and metadata_list differ in length")
        with t.lock.write():
            t.drop_masks()
            t.index.pq_clear()  # metadata_vec_table.rs:65,77
            first = len(t.metadata)
            t.metadata.extend(dict(m) for m in metadata_list)
            t.index.batch_add(rows)
            for k in t.codec.keys():  # the new rows' values of the live columns (the library left them unlabelled)
                t.index.set_labels(t.codec.column_of(k), t.codec.encode_rows(k, t.metadata[first:]), first_row=first)

    def delete(self, key: str, pattern: dict[str, str]) -> int:
        if not isinstance(pattern, dict):
            raise TypeError("delete takes a metadata pattern (a dict), not a filter expression")
        t = self._t(key)
        with t.lock.write():
            t.drop_masks()
            t.index.hnsw_clear()  # :170
            t.index.pq_clear()    # :171
            # the matches from the device mask of the pattern when its keys are label columns already (a delete gives no key a column:
            # deleting by id must not intern every id); the columns follow the removal inside the library
            terms = t.live_terms(pattern)
            if terms is not None:
                mk = t.device_mask(pattern, terms)
                matches = mk.rows()[1].tolist()
                mk.close()
            else:
                matches = np.flatnonzero(t.host_match(pattern)).tolist()
            if matches:  # one call; the metadata follow the moves it reports (the net effect of swap_remove in descending order)
                dst, src = t.index.remove_rows(matches)
                for d, s in zip(dst.tolist(), src.tolist()):
                    t.metadata[d] = t.metadata[s]
                del t.metadata[len(t.metadata) - len(matches):]
            return len(matches)

    def update(self, key: str, pattern: dict[str, str], vec) -> int:
        """New vector for every row `pattern` matches (batch_update with one pattern); returns the number of rows."""
        return self.batch_update(key, [pattern], [vec])[0]

    def batch_update(self, key: str, patterns, vec_list) -> list[int]:
        """Replaces the VECTORS of existing rows in place: every row that patterns[i] matches -- a metadata pattern exactly as delete
        takes one -- gets vec_list[i]; a row several patterns match gets the LAST one's vector.  Returns the matches per pattern.  The rows
        keep their ids and their metadata, nothing else moves, and the table's cached filter masks stay valid (a filter is a set of rows,
        and the set did not change).  One library call for the whole batch; like delete it clears the HNSW index and the PQ table first --
        unless nothing matched, then nothing at all is changed.
        The METADATA of existing rows is changed by update_metadata / batch_update_metadata.  An upsert -- batch_update plus batch_add of
        what matched nothing -- is batch_upsert, which finds its rows in one pass over the key's column."""
        t = self._t(key)
        patterns = list(patterns)
        for p in patterns:
            if not isinstance(p, dict):
                raise TypeError("update takes a metadata pattern (a dict), not a filter expression")
        vecs = np.asarray(vec_list, dtype=np.float32)
        if len(patterns) == 0 and vecs.size == 0:
            return []
        if vecs.ndim != 2 or vecs.shape[1] != t.index.dim:  # (batch_add's wording)
            raise RuntimeError(f"Dimension mismatch: table dim {t.index.dim}, got {vecs.shape}")
        if len(patterns) != vecs.shape[0]:
            raise RuntimeError("patterns and vec_list differ in length")
        with t.lock.write():
            # the matches as delete finds them: from a cached or device-built mask when the pattern's keys are label columns already (an
            # update gives no key a column), from the host loop otherwise; the plain patterns not cached yet share ONE make_masks_where call
            matches = t.match_rows(patterns)
            winner: dict[int, int] = {}  # row -> the last pattern that matches it (the library wants distinct ids)
            for i, rows in enumerate(matches):
                for r in np.asarray(rows).tolist():
                    winner[int(r)] = i
            if winner:
                t.index.hnsw_clear()
                t.index.pq_clear()
                rows = np.fromiter(winner.keys(), dtype=np.uint64, count=len(winner))
                t.index.update_rows(rows, vecs[np.fromiter(winner.values(), dtype=np.int64, count=len(winner))])
            return [int(len(m)) for m in matches]

    @staticmethod
    def _apply_changes(m: dict, changes: dict) -> None:
        for k, v in changes.items():
            if v is None:
                m.pop(k, None)
            else:
                m[k] = v

    def update_metadata(self, key: str, pattern: dict[str, str], changes: dict) -> int:
        """metadata.update(changes) for every row `pattern` matches -- a metadata pattern exactly as delete takes one; a value None in
        `changes` REMOVES the key from the row.  Returns the number of rows matched.  The rows keep their ids and vectors, nothing moves,
        and the HNSW graph and the PQ table stay.  Like delete and update it gives NO key a label column: for the keys of `changes`
        that have one already the new values are interned and written by ONE GpuIndex.set_labels_mask call over the pattern's mask
        (cached, built on the device, or from the host loop); the other keys change on the host only -- a column they get later is encoded
        from the updated metadata.  Order: intern, device write, host dicts, so a failed library call leaves the table as it was.
        Afterwards exactly the cached filter masks that name a changed key are dropped (labels.filter_keys).  Nothing matched, or empty
        `changes`: nothing changes at all and no mask is dropped."""
        if not isinstance(pattern, dict):
            raise TypeError("update_metadata takes a metadata pattern (a dict), not a filter expression")
        changes = dict(changes)
        t = self._t(key)
        with t.lock.write():
            with t.mask_mu:
                mk = t.masks.get(frozenset(pattern.items()))
            own = mk is None
            if own:
                terms = t.live_terms(pattern)
                mk = t.device_mask(pattern, terms) if terms is not None else t.index.make_mask(t.host_match(pattern))
            try:
                rows = mk.rows()[1].tolist()
                if not rows or not changes:
                    return len(rows)
                live = [k for k in changes if t.codec.column_of(k) is not None]
                if live:
                    t.index.set_labels_mask(mk, [t.codec.column_of(k) for k in live], [t.codec.encode_value(k, changes[k]) for k in live])
            finally:
                if own:
                    mk.close()
            for r in rows:
                self._apply_changes(t.metadata[r], changes)
            t.drop_masks_naming(changes)
            return len(rows)

    def batch_update_metadata(self, key: str, patterns, changes_list) -> list[int]:
        """update_metadata for many (pattern, changes) pairs at once; returns the matches per pattern.  ALL patterns are matched against
        the table as it stands BEFORE the call (the unbuilt plain ones share one make_masks_where call, as in batch_update); a row several
        patterns match receives their changes in pattern order, so per key the LAST one wins.  The device write is ONE
        GpuIndex.set_labels_rows call over the union of the matched rows and every live column some change names: the code of (row,
        column) is that of the row's FINAL value, so a row a column's changes do not reach is re-written with the value it has."""
        t = self._t(key)
        patterns = list(patterns)
        for p in patterns:
            if not isinstance(p, dict):
                raise TypeError("update_metadata takes a metadata pattern (a dict), not a filter expression")
        changes_list = [dict(c) for c in changes_list]
        if len(patterns) != len(changes_list):
            raise RuntimeError("patterns and changes_list differ in length")
        with t.lock.write():
            matches = t.match_rows(patterns)
            merged: dict[int, dict] = {}  # row -> its changes, merged in pattern order
            changed: dict[str, None] = {}  # the keys some effective change names, in order of first appearance
            for rows, ch in zip(matches, changes_list):
                if ch and len(rows):
                    changed.update(dict.fromkeys(ch))
                    for r in np.asarray(rows).tolist():
                        merged.setdefault(int(r), {}).update(ch)
            if merged:
                live = [k for k in changed if t.codec.column_of(k) is not None]
                if live:
                    codes = np.empty((len(live), len(merged)), dtype=np.uint32)
                    for c, k in enumerate(live):
                        codes[c] = [t.codec.encode_value(k, ch[k] if k in ch else t.metadata[r].get(k)) for r, ch in merged.items()]
                    t.index.set_labels_rows(np.fromiter(merged.keys(), dtype=np.uint64, count=len(merged)),
                                            [t.codec.column_of(k) for k in live], codes)
                for r, ch in merged.items():
                    self._apply_changes(t.metadata[r], ch)
                t.drop_masks_naming(changed)
            return [int(len(m)) for m in matches]

    def upsert(self, key: str, id_field: str, vec, metadata: dict[str, str]) -> tuple[int, int]:
        """batch_upsert of one entry."""
        return self.batch_upsert(key, id_field, [vec], [metadata])

    def batch_upsert(self, key: str, id_field: str, vec_list, metadata_list) -> tuple[int, int]:
        """The idempotent write by a key field: entry i is (vec_list[i], metadata_list[i]), and metadata_list[i][id_field] -- a str --
        names it.  A value no row carries: the entry is appended, in the batch order of the surviving entries.  A value ONE row carries:
        that row gets the new vector and its metadata dict is REPLACED by the new one; its row id is kept.  A value several rows carry:
        ValueError naming it -- the key is not unique -- and nothing at all is changed.  Two entries with the same value: the LAST one
        wins and the earlier ones are dropped (batch_update's rule).  Returns (rows updated, rows added).
        `id_field` gets a label column on first use, as count_by's field does, and the rows are found by ONE GpuIndex.label_lookup call
        over the values the column's dictionary knows (a value it has never seen matches nothing and does not grow it for the lookup).
        A key that cannot have a column (a 17th key) or whose dictionary holds the stand-in for unhashable values is looked up by one
        pass over the metadata.  Everything is validated before anything changes; then hnsw_clear / pq_clear as batch_update does them
        when a row is updated (pq_clear alone, as batch_add, when rows are only added), ONE update_rows, ONE set_labels_rows over the
        updated rows and every live column, ONE batch_add with set_labels per live column, the host dicts.  Masks: all dropped when a
        row was added; otherwise exactly those whose filter names a key whose value changed in some updated row."""
        t = self._t(key)
        rows = np.asarray(vec_list, dtype=np.float32)
        metadata_list = list(metadata_list)
        if len(metadata_list) == 0 and rows.size == 0:
            return 0, 0
        if rows.ndim != 2 or rows.shape[1] != t.index.dim:  # (batch_add's checks and wording)
            raise RuntimeError(f"Dimension mismatch: table dim {t.index.dim}, got {rows.shape}")
        if len(metadata_list) != rows.shape[0]:
            raise RuntimeError("vec_list and metadata_list differ in length")
        last: dict[str, int] = {}
        for i, m in enumerate(metadata_list):
            v = m.get(id_field) if isinstance(m, dict) else None
            if not isinstance(v, str):
                raise ValueError(f"upsert: entry {i} carries no str value of {id_field!r}")
            last[v] = i
        keep = sorted(last.values())  # the surviving entries, in batch order
        values = [metadata_list[i][id_field] for i in keep]
        with t.lock.write():
            if t.codec.column_of(id_field) is None:
                t.create_columns([{id_field: None}])  # (taken back if its write fails; a 17th key gets none)
            first, counts, _ = t.find_values(id_field, values)
            many = np.flatnonzero(counts > 1)
            if many.size:
                j = int(many[0])
                raise ValueError(f"upsert: {id_field} = {values[j]!r} is carried by {int(counts[j])} rows: the key is not unique")
            upd = np.flatnonzero(counts == 1)
            add = np.flatnonzero(counts == 0)
            live = t.codec.keys()
            if upd.size:
                t.index.hnsw_clear()
            t.index.pq_clear()
            changed: dict[str, None] = {}
            if upd.size:
                urows = first[upd]
                new = [metadata_list[keep[j]] for j in upd.tolist()]
                t.index.update_rows(urows, rows[[keep[j] for j in upd.tolist()]])
                if live:
                    codes = np.empty((len(live), len(new)), dtype=np.uint32)
                    for c, k in enumerate(live):
                        codes[c] = [t.codec.encode_value(k, m.get(k)) for m in new]
                    t.index.set_labels_rows(urows, [t.codec.column_of(k) for k in live], codes)
            if add.size:
                fresh = [dict(metadata_list[keep[j]]) for j in add.tolist()]
                first_new = len(t.metadata)
                t.index.batch_add(rows[[keep[j] for j in add.tolist()]])
                for k in live:
                    t.index.set_labels(t.codec.column_of(k), t.codec.encode_rows(k, fresh), first_row=first_new)
            if upd.size:
                for r, m in zip(urows.tolist(), new):
                    old = t.metadata[r]
                    changed.update(dict.fromkeys(k for k in old.keys() | m.keys() if _differ(old.get(k), m.get(k))))
                    t.metadata[r] = dict(m)
            if add.size:
                t.metadata.extend(fresh)
                t.drop_masks()
            elif changed:
                t.drop_masks_naming(changed)
            return int(upd.size), int(add.size)

    def get_by(self, key: str, field: str, values, with_vectors: bool = False) -> list:
        """The fetch by a key field: per entry of `values` (hashable; None: the rows without the key) the list of (metadata,) -- or
        (metadata, vector) with `with_vectors` -- of the rows whose metadata carries it under `field`, ascending by row; a value no row
        carries, or one never seen, gives [].  `field` gets a label column on first use, as a filter key does; the rows come from ONE
        GpuIndex.label_lookup call, the few values that several rows carry from ONE make_masks_where call on top of it, and all vectors
        from ONE get_rows call.  A field without a usable column takes one pass over the metadata instead."""
        t = self._t(key)
        values = list(values)
        distinct = list(dict.fromkeys(values))
        t.prepare([{field: None}])
        with t.lock.read():
            first, counts, rows_of = t.find_values(field, distinct)
            if rows_of is None:
                rows_of = {v: [int(f)] if c == 1 else [] for v, f, c in zip(distinct, first.tolist(), counts.tolist())}
                many = [v for v, c in zip(distinct, counts.tolist()) if c > 1]
                if many:
                    col = t.codec.column_of(field)
                    table = t.codec.codes[col]
                    for v, mk in zip(many, t.index.make_masks_where([[(col, LABEL_NONE if v is None else table[v])] for v in many])):
                        rows_of[v] = mk.rows()[1].tolist()
                        mk.close()
            flat = [r for v in values for r in rows_of[v]]
            if not with_vectors:
                it = iter((dict(t.metadata[r]),) for r in flat)
            else:
                vecs = t.index.get_rows(np.array(flat, dtype=np.uint64)) if flat else np.zeros((0, t.index.dim), dtype=np.float32)
                it = iter((dict(t.metadata[r]), vecs[j].copy()) for j, r in enumerate(flat))
            return [[next(it) for _ in rows_of[v]] for v in values]

    def build_hnsw_index(self, key: str, ef_construction: int | None = None) -> None:
        t = self._t(key)
        with t.lock.write():
            if t.index.has_hnsw():
                return
            t.index.hnsw_build(M=16, ef_construction=200 if ef_construction is None else ef_construction,
                               seed=t.next_seed(), batch=1, nthreads=1)

    def clear_hnsw_index(self, key: str) -> None:
        t = self._t(key)
        with t.lock.write():
            t.index.hnsw_clear()

    def has_hnsw_index(self, key: str) -> bool:
        t = self._t(key)
        with t.lock.read():
            return t.index.has_hnsw()

    def build_pq_table(self, key: str, train_proportion: float | None = None, n_bits: int | None = None,
                       m: int | None = None) -> None:
        t = self._t(key)
        with t.lock.write():
            if t.index.has_pq():
                return
            n = len(t.index)
            if n == 0:
                raise RuntimeError("Cannot build PQ table for an empty table")
            prop = 0.1 if train_proportion is None else train_proportion
            if prop <= 0.0 or prop >= 1.0:
                raise RuntimeError("Train proportion must be in (0, 1)")
            train = int(max(np.float32(n) * np.float32(prop), np.float32(1.0)))
            nb = 4 if n_bits is None else n_bits
            if nb not in (4, 8):
                raise RuntimeError("n_bits must be 4 or 8")
            dim = t.index.dim
            mm = -(-dim // 3) if m is None else m
            if mm == 0 or mm > dim:
                raise RuntimeError("m must be in 1..=dim")
            # the reference validates n_bits but hard-codes 4 in the PQConfig (metadata_vec_table.rs:140)
            t.index.pq_build(n_bits=4, m=mm, train_n=train, max_iter=20, tol=1e-6, seed=t.next_seed())

    def clear_pq_table(self, key: str) -> None:
        t = self._t(key)
        with t.lock.write():
            t.index.pq_clear()

    def has_pq_table(self, key: str) -> bool:
        t = self._t(key)
        with t.lock.read():
            return t.index.has_pq()

    # ---- reads ------------------------------------------------------------------------------------------------
    def search(self, key: str, query, k: int, ef: int | None = None, upper_bound: float | None = None,
               filter: dict[str, str] | None = None, group_by: str | None = None, group_size: int = 1, with_vectors: bool = False,
               mmr_lambda: float | None = None, fetch_k: int | None = None):
        """MetadataVecTable::search.  `filter`: a metadata pattern matched exactly as delete matches (every key present with an equal
        value; an empty pattern matches every row) -- only matching rows are searched.  With a filter the answer is always EXACT, from
        the table's Flat rows, whatever indexes the table has, and `ef` is ignored.  `group_by`: a metadata key -- at most `group_size`
        hits per value of it (batch_search states the rule); exact as with a filter, same return shape.  `with_vectors`: entries become
        (metadata, distance, vector) -- the hits' vectors (float32 arrays) from ONE get_rows call over the hit ids.  `mmr_lambda` /
        `fetch_k`: diversified hits in selection order (batch_search states the rule); exact as with a filter."""
        t = self._t(key)
        ix = t.index
        q = np.asarray(query, dtype=np.float32).ravel()
        if group_by is not None or mmr_lambda is not None or fetch_k is not None:
            return self.batch_search(key, q.reshape(1, -1), k, ef, upper_bound, filter, group_by, group_size, with_vectors, mmr_lambda, fetch_k)[0]
        if filter is not None:
            t.prepare([filter])
        with t.lock.read():  # database/mod.rs:255: read guard for the whole search, metadata lookup included
            if filter is not None:
                idx, dist = ix.flat_knn_filtered(q, k, t.mask_for(filter))
                ub = np.float32(np.inf) if upper_bound is None else np.float32(upper_bound)
                if with_vectors:
                    return self._hits_with_vectors(t, [idx], [dist], ub)[0]
                return [(dict(t.metadata[int(i)]), float(d)) for i, d in zip(idx, dist) if d <= ub]
            if ef is not None and ix.has_pq():
                idx, dist = ix.knn_pq(q, k, ef)
            elif ef is not None:
                idx, dist = ix.knn_with_ef(q, k, ef)
            else:
                idx, dist = ix.knn(q, k)
            ub = np.float32(np.inf) if upper_bound is None else np.float32(upper_bound)
            if with_vectors:
                return self._hits_with_vectors(t, [idx], [dist], ub)[0]
            return [(dict(t.metadata[int(i)]), float(d)) for i, d in zip(idx, dist) if d <= ub]

    def batch_search(self, key: str, queries, k: int, ef: int | None = None, upper_bound: float | None = None, filters=None,
                     group_by: str | None = None, group_size: int = 1, with_vectors: bool = False, mmr_lambda: float | None = None,
                     fetch_k: int | None = None):
        """search for a batch of queries in ONE library call: entry q of the returned list is what search(key, queries[q], k, ef,
        upper_bound, filter) returns.  `filters`: None, ONE metadata pattern for every query, or a list of len(queries) patterns (the
        multi-tenant batch: every query restricted to its own rows; {} matches every row).  With filters the answers are exact, from
        the table's Flat rows, through one flat_knn_filtered_multi call over one mask per distinct pattern; without, the batch is
        dispatched as search dispatches a query (knn_pq, knn_with_ef or knn).
        `group_by`: a metadata key.  Walking a query's matching rows nearest first (ties by row), a row without the key is always kept
        and a row with value v is kept iff fewer than `group_size` rows before it carry v; the answer is the first k kept rows -- always
        exact, from the Flat rows (`ef` is ignored), a flat list as without it; `upper_bound` is applied afterwards.  The key gets a label
        column on first use, as count_by's field does, and the batch is ONE flat_knn_grouped call (under the filters' masks when there
        are filters).  A key that cannot have a column (a 17th key) or whose values a dictionary cannot keep apart takes the host
        fallback: the ungrouped search at a growing k, walked by labels.cap_groups over the metadata values.
        `with_vectors`: entries become (metadata, distance, vector); the vectors of all hits of the batch come from ONE get_rows call
        over the hit ids (no call when the batch has no hit).
        `mmr_lambda`: a number in [0, 1] -- maximal marginal relevance.  From a query's `fetch_k` nearest matching rows (default 4 k,
        raised to k, clamped to 4096) the nearest is taken first and then, greedily, the row with the smallest
        mmr_lambda * d(query, row) - (1 - mmr_lambda) * min over the rows taken of d(row, taken), ties to the nearer row, until k are taken:
        1 is the plain search, 0 the farthest-first walk of the candidates.  Always exact, from the Flat rows (`ef` is ignored); the batch
        is ONE flat_knn_mmr call (under the filters' masks when there are filters); entries come IN SELECTION ORDER, not by distance;
        `upper_bound` is applied afterwards.  Not together with `group_by`; `fetch_k` without `mmr_lambda` is an error."""
        if group_by is not None and int(group_size) < 1:
            raise ValueError("group_size must be at least 1")
        if mmr_lambda is not None and group_by is not None:
            raise ValueError("mmr_lambda and group_by cannot be combined")
        if fetch_k is not None and mmr_lambda is None:
            raise ValueError("fetch_k needs mmr_lambda")
        t = self._t(key)
        ix = t.index
        q = np.asarray(queries, dtype=np.float32)
        if q.ndim != 2 or q.shape[1] != ix.dim:
            raise RuntimeError(f"Dimension mismatch: table dim {ix.dim}, got {q.shape}")
        nq = q.shape[0]
        if filters is not None and not isinstance(filters, dict) and not is_expression(filters):
            filters = list(filters)
            if len(filters) != nq:
                raise RuntimeError(f"filters: one pattern per query is needed ({nq}), got {len(filters)}")
        if nq == 0:
            return []
        pats = None
        if filters is not None:
            pats = [filters] * nq if isinstance(filters, dict) or is_expression(filters) else filters
            t.prepare(pats)
        if group_by is not None:
            t.prepare([{group_by: None}])  # (the key's column, as count_by makes it)
        with t.lock.read():  # one read guard for the whole batch, mask building and metadata lookup included
            masks = mask_of = None
            if pats is not None:
                slot: dict[object, int] = {}
                distinct, mask_of = [], np.zeros(nq, dtype=np.uint32)
                for i, p in enumerate(pats):
                    pk = filter_key(p)
                    if pk not in slot:
                        slot[pk] = len(distinct)
                        distinct.append(p)
                    mask_of[i] = slot[pk]
                masks = t.masks_for(distinct)  # the ones not cached yet: one library call
            if group_by is not None:
                if t.codec.value_codes(group_by) is not None:
                    idx, dist, cnt = ix.flat_knn_grouped(q, k, t.codec.column_of(group_by), group_size, masks, mask_of)
                else:
                    idx, dist, cnt = self._grouped_on_host(t, q, k, group_by, group_size, masks, mask_of)
            elif mmr_lambda is not None:
                fk = min(max(4 * int(k) if fetch_k is None else int(fetch_k), int(k)), MMR_MAX_FETCH)
                idx, dist, cnt = ix.flat_knn_mmr(q, k, fk, mmr_lambda, masks, mask_of)
            elif pats is not None:
                idx, dist, cnt = ix.flat_knn_filtered_multi(q, k, masks, mask_of)
            elif ef is not None and ix.has_pq():
                idx, dist, cnt = ix.knn_pq(q, k, ef)
            elif ef is not None:
                idx, dist, cnt = ix.knn_with_ef(q, k, ef)
            else:
                idx, dist, cnt = ix.knn(q, k)
            ub = np.float32(np.inf) if upper_bound is None else np.float32(upper_bound)
            if with_vectors:
                return self._hits_with_vectors(t, [idx[j, :int(cnt[j])] for j in range(nq)], [dist[j, :int(cnt[j])] for j in range(nq)], ub)
            return [[(dict(t.metadata[int(i)]), float(d)) for i, d in zip(idx[j, :int(cnt[j])], dist[j, :int(cnt[j])]) if d <= ub]
                    for j in range(nq)]

    def search_like(self, key: str, positive, k: int, negative=None, filter=None, upper_bound: float | None = None,
                    exclude_examples: bool = True, with_vectors: bool = False):
        """Search by example rows: batch_search_like for one query (it states the rule); same return shape as search."""
        return self.batch_search_like(key, [positive], k, None if negative is None else [negative], filter, upper_bound, exclude_examples,
                                      with_vectors)[0]

    def batch_search_like(self, key: str, positives, k: int, negatives=None, filters=None, upper_bound: float | None = None,
                          exclude_examples: bool = True, with_vectors: bool = False):
        """"More like these rows, and not like those", for a batch of queries in ONE library call (GpuIndex.flat_knn_like).  `positives`:
        one filter per query, of any kind search accepts (a pattern, a pattern with predicates, an expression) -- the rows it matches,
        in ascending row order, are the query's positive examples; `negatives`: None, or one filter (or None) per query for the rows to
        steer away from.  The query vector is the average of the positives, plus its difference from the average of the negatives
        (ap + ap - an per element, in f32), made on the device from the stored rows; the k nearest rows to it come back exactly, from the
        table's Flat rows, with every example left out unless `exclude_examples` is False.  `filters` restricts the rows searched, as in
        batch_search; `upper_bound` is applied afterwards; `with_vectors` as in batch_search.  A positive filter that matches no row,
        and a query with more than 1024 examples, raise ValueError and name the query.  Entry q of the returned list is what
        search(key, <that query vector>, k, ...) returns, less the examples."""
        t = self._t(key)
        ix = t.index
        positives = list(positives)
        nq = len(positives)
        negatives = [None] * nq if negatives is None else list(negatives)
        if len(negatives) != nq:
            raise RuntimeError(f"negatives: one filter (or None) per query is needed ({nq}), got {len(negatives)}")
        if filters is not None and not isinstance(filters, dict) and not is_expression(filters):
            filters = list(filters)
            if len(filters) != nq:
                raise RuntimeError(f"filters: one pattern per query is needed ({nq}), got {len(filters)}")
        if nq == 0:
            return []
        pats = None
        if filters is not None:
            pats = [filters] * nq if isinstance(filters, dict) or is_expression(filters) else filters
        wanted = positives + [f for f in negatives if f is not None] + (pats or [])
        t.prepare(wanted)
        with t.lock.read():  # one read guard for the whole batch: masks, example rows, the search and the metadata lookup
            slot: dict[object, int] = {}
            distinct = []
            for f in wanted:
                fk = filter_key(f)
                if fk not in slot:
                    slot[fk] = len(distinct)
                    distinct.append(f)
            all_masks = t.masks_for(distinct)  # the ones not cached yet: one library call per kind
            rows_of: dict[int, np.ndarray] = {}

            def rows(f):
                s = slot[filter_key(f)]
                if s not in rows_of:
                    rows_of[s] = all_masks[s].rows()[1]  # ascending row ids
                return rows_of[s]

            pos_rows, neg_rows = [], []
            for i in range(nq):
                p = rows(positives[i])
                g = rows(negatives[i]) if negatives[i] is not None else p[:0]
                if len(p) == 0:
                    raise ValueError(f"search_like: query {i}: the positive filter matches no row")
                if len(p) + len(g) > LIKE_MAX_EXAMPLES:
                    raise ValueError(f"search_like: query {i} has {len(p) + len(g)} example rows, at most {LIKE_MAX_EXAMPLES} are allowed")
                pos_rows.append(p)
                neg_rows.append(g)
            masks = mask_of = None
            if pats is not None:
                used: dict[int, int] = {}
                masks, mask_of = [], np.zeros(nq, dtype=np.uint32)
                for i, f in enumerate(pats):
                    s = slot[filter_key(f)]
                    if s not in used:
                        used[s] = len(masks)
                        masks.append(all_masks[s])
                    mask_of[i] = used[s]
            idx, dist, cnt = ix.flat_knn_like(pos_rows, k, neg_rows if any(len(g) for g in neg_rows) else None, exclude_examples, masks, mask_of)
            ub = np.float32(np.inf) if upper_bound is None else np.float32(upper_bound)
            if with_vectors:
                return self._hits_with_vectors(t, [idx[j, :int(cnt[j])] for j in range(nq)], [dist[j, :int(cnt[j])] for j in range(nq)], ub)
            return [[(dict(t.metadata[int(i)]), float(d)) for i, d in zip(idx[j, :int(cnt[j])], dist[j, :int(cnt[j])]) if d <= ub]
                    for j in range(nq)]

    def search_fused(self, key: str, queries, k: int, fusion: str = "rrf", weights=None, filters=None, fetch_k: int | None = None,
                     rrf_c: float = 60.0, upper_bound: float | None = None, with_vectors: bool = False, group_by: str | None = None,
                     return_exact: bool = False):
        """Several searches of ONE question joined into one ranked answer: batch_search_fused for one question (it states the rule).
        `queries`: the vectors of the question; `weights`: None or one per vector; `filters`: None, one filter for every vector, or one
        per vector.  Entries are (metadata, score[, vector]); with return_exact the result is (entries, exact)."""
        res = self.batch_search_fused(key, [queries], k, fusion, None if weights is None else [weights], None if filters is None else [filters],
                                      fetch_k, rrf_c, upper_bound, with_vectors, group_by, return_exact)
        return (res[0][0], res[1][0]) if return_exact else res[0]

    def batch_search_fused(self, key: str, query_groups, k: int, fusion: str = "rrf", weights=None, filters=None, fetch_k: int | None = None,
                           rrf_c: float = 60.0, upper_bound: float | None = None, with_vectors: bool = False, group_by: str | None = None,
                           return_exact: bool = False):
        """Fused multi-query search for a batch of questions in ONE library call (GpuIndex.flat_knn_fused).  `query_groups`: per
        question its 1 to 32 query vectors (paraphrases, a HyDE passage, sub-questions -- or one vector repeated under several filters).
        Every vector is searched exactly, from the table's Flat rows, for its `fetch_k` nearest matching rows (default 4 k, raised to k,
        clamped to 4096) and the lists of a question are joined on the device:
          fusion="rrf": reciprocal rank fusion -- a row's score is the sum, over the lists that hold it in list order, of
            weight / (rank + 1 + rrf_c) in f32; hits by score descending (ties: the lower row), the entry's second item is the score.
          fusion="min": a row's score is its smallest distance to any of the vectors; hits ascending -- exactly the k matching rows
            nearest to any of the vectors; `weights` must be None.
        `weights`: None, or per question None or one positive number per vector.  `filters`: None; ONE filter for every vector of the
        batch; or per question None, one filter, or one filter (or None: every row) per vector -- of any kind search accepts, through
        the mask cache, one mask per distinct filter.  `upper_bound`: fusion="min" only (the score is a distance), applied afterwards;
        with "rrf" it is a ValueError.  `with_vectors` as in batch_search.  One read guard covers the batch.
        `group_by`: a metadata key -- the unit of ranking becomes the GROUP, the matching rows that share a value of the key (rows are
        chunks, the key names the document); a row without the key is a group of its own.  In every list a group counts once, at its
        first (nearest) row, and an entry is (metadata of the group's representative row -- its nearest over the vectors --, score[,
        vector]).  "rrf" ranks by the group's rank among the GROUPS of each list; "min" by its smallest distance; fusion="sum" (with
        group_by only) by the sum over the vectors of the group's nearest distance, a vector whose list lacks the group counting with its
        list's last distance: the late-interaction score, a lower bound of the true sum while a list is cut at fetch_k.  `weights` go
        with "rrf" only.  ONE library call (GpuIndex.flat_knn_fused_groups); the key gets a label column on first use, as
        batch_search(group_by=) gives it one, and a key that cannot have a column (a 17th key) or whose values a dictionary cannot keep
        apart takes the host fallback: batch_search's lists at fetch_k, joined by labels.fuse_groups over the metadata values.
        `return_exact` (group_by only): the result becomes (answers, exact) -- exact[q] is True when the whole table would give this
        answer ("rrf", "sum": no list was cut at fetch_k; "min": that, or the k-th score lies strictly before every cut)."""
        if fusion not in ("rrf", "min") and not (fusion == "sum" and group_by is not None):
            raise ValueError(f"fusion {fusion!r}: 'rrf' or 'min'" + (", or 'sum'" if group_by is not None else " ('sum' needs group_by)"))
        if upper_bound is not None and fusion != "min":
            raise ValueError("upper_bound applies to fusion='min' only: an RRF score or a sum is no distance")
        if return_exact and group_by is None:
            raise ValueError("return_exact needs group_by")
        if group_by is not None and weights is not None and fusion != "rrf" and any(x is not None for x in weights):
            raise ValueError("weights belong to fusion='rrf' only")
        t = self._t(key)
        ix = t.index
        groups = [np.asarray(g, dtype=np.float32) for g in query_groups]
        groups = [g.reshape(1, -1) if g.ndim == 1 else g for g in groups]
        nq = len(groups)
        for i, g in enumerate(groups):
            if g.ndim != 2 or g.shape[1] != ix.dim or g.shape[0] == 0:
                raise RuntimeError(f"Dimension mismatch: table dim {ix.dim}, question {i} got {g.shape}")
        if nq == 0:
            return ([], []) if return_exact else []
        sizes = [g.shape[0] for g in groups]
        lims = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
        w = None
        if weights is not None:
            weights = list(weights)
            if len(weights) != nq:
                raise RuntimeError(f"weights: one list (or None) per question is needed ({nq}), got {len(weights)}")
            if any(x is not None for x in weights):
                parts = [np.ones(sizes[i], dtype=np.float32) if x is None else np.asarray(x, dtype=np.float32).ravel() for i, x in enumerate(weights)]
                for i, x in enumerate(parts):
                    if x.shape[0] != sizes[i]:
                        raise RuntimeError(f"weights: question {i} has {sizes[i]} vectors and {x.shape[0]} weights")
                w = np.concatenate(parts)
        pats = None  # one filter per sub-query, or None: unfiltered
        if filters is not None:
            one = lambda f: isinstance(f, dict) or is_expression(f)  # noqa: E731
            if one(filters):
                pats = [filters] * int(lims[-1])
            else:
                filters = list(filters)
                if len(filters) != nq:
                    raise RuntimeError(f"filters: one entry per question is needed ({nq}), got {len(filters)}")
                pats = []
                for i, f in enumerate(filters):
                    if f is None or one(f):
                        pats += [{} if f is None else f] * sizes[i]
                    else:
                        f = list(f)
                        if len(f) != sizes[i]:
                            raise RuntimeError(f"filters: question {i} has {sizes[i]} vectors and {len(f)} filters")
                        pats += [{} if x is None else x for x in f]
            t.prepare(pats)
        q = np.ascontiguousarray(np.concatenate(groups, axis=0))
        fk = min(max(4 * int(k) if fetch_k is None else int(fetch_k), int(k)), FUSE_MAX_FETCH)
        if group_by is not None:
            t.prepare([{group_by: None}])  # (the key's column, as count_by makes it)
        with t.lock.read():  # one read guard for the whole batch, mask building and metadata lookup included
            masks = mask_of = None
            if pats is not None:
                slot: dict[object, int] = {}
                distinct, mask_of = [], np.zeros(len(pats), dtype=np.uint32)
                for i, p in enumerate(pats):
                    pk = filter_key(p)
                    if pk not in slot:
                        slot[pk] = len(distinct)
                        distinct.append(p)
                    mask_of[i] = slot[pk]
                masks = t.masks_for(distinct)  # the ones not cached yet: one library call
            exact = None
            if group_by is None:
                idx, dist, cnt = ix.flat_knn_fused(q, lims, k, fk, fusion, w, rrf_c, masks, mask_of)
            elif t.codec.value_codes(group_by) is not None:
                idx, dist, cnt, exact = ix.flat_knn_fused_groups(q, lims, k, fk, t.codec.column_of(group_by), fusion, w, rrf_c, masks, mask_of,
                                                                 return_exact=True)
            else:
                idx, dist, cnt, exact = self._fused_groups_on_host(t, q, lims, k, fk, group_by, fusion, w, rrf_c, masks, mask_of)
            ub = np.float32(np.inf) if upper_bound is None else np.float32(upper_bound)
            if with_vectors:
                res = self._hits_with_vectors(t, [idx[j, :int(cnt[j])] for j in range(nq)], [dist[j, :int(cnt[j])] for j in range(nq)], ub)
            else:
                res = [[(dict(t.metadata[int(i)]), float(d)) for i, d in zip(idx[j, :int(cnt[j])], dist[j, :int(cnt[j])]) if d <= ub]
                       for j in range(nq)]
            return (res, [bool(x) for x in exact]) if return_exact else res

    @staticmethod
    def _fused_groups_on_host(t: _Table, q: np.ndarray, lims, k: int, fk: int, field: str, fusion: str, w, rrf_c: float, masks, mask_of):
        """UNDER THE READ LOCK: search_fused(group_by=) for a field without a usable label column -- the exact lists of every vector at
        fetch_k from ONE ungrouped search, joined per question by labels.fuse_groups over the metadata values (unhashable values are told
        apart by a scan).  -> (idx, dist, cnt, exact) as GpuIndex.flat_knn_fused_groups(return_exact=True) returns them."""
        ix = t.index
        nq, k = len(lims) - 1, int(k)
        if masks is None:
            idx, dist, cnt = ix.flat_knn(q, fk)
            max_m = len(ix)
        else:
            idx, dist, cnt = ix.flat_knn_filtered_multi(q, fk, masks, mask_of)
            max_m = max(len(masks[int(m)]) for m in mask_of)
        trunc = None if fk >= max_m else fk  # (fetch_k reaches the longest allowed set: every list is whole, as the library reasons)
        o_idx, o_dist = np.zeros((nq, max(k, 1)), np.uint64), np.zeros((nq, max(k, 1)), np.float32)
        o_cnt, o_exact = np.zeros(nq, np.uint64), np.zeros(nq, np.uint8)
        for j in range(nq):
            if k == 0:
                continue  # (nothing is ranked: zero counts, zero exact, as the library answers)
            odd, lists = [], []
            for s in range(int(lims[j]), int(lims[j + 1])):
                c = int(cnt[s])
                values = []
                for i in idx[s, :c]:
                    v = t.metadata[int(i)].get(field)
                    try:
                        hash(v)
                    except TypeError:
                        if v not in odd:
                            odd.append(v)
                        v = ("unhashable", odd.index(v), id(odd))
                    values.append(v)
                lists.append((idx[s, :c], dist[s, :c], values))
            ws = None if w is None else w[int(lims[j]):int(lims[j + 1])]
            gi, gd, ge = fuse_groups(lists, k, fusion, ws, rrf_c, trunc_len=trunc)
            o_cnt[j], o_exact[j] = len(gi), ge
            o_idx[j, :len(gi)], o_dist[j, :len(gi)] = gi, gd
        return o_idx[:, :k], o_dist[:, :k], o_cnt, o_exact

    @staticmethod
    def _grouped_on_host(t: _Table, q: np.ndarray, k: int, field: str, group_size: int, masks, mask_of):
        """UNDER THE READ LOCK: group_by for a field without a usable label column -- the exact ungrouped search at a growing k (4 k, then
        4 x that), each query's list walked by cap_groups over the metadata values, until every query has k kept rows or its list was
        every row it may see.  Values are told apart by equality (unhashable ones by a scan)."""
        ix = t.index
        nq = q.shape[0]
        k = int(k)
        kk = max(k, 1) * 4
        n = len(ix)
        while True:
            if masks is None:
                idx, dist, cnt = ix.flat_knn(q, kk)
            else:
                idx, dist, cnt = ix.flat_knn_filtered_multi(q, kk, masks, mask_of)
            o_idx, o_dist, o_cnt = np.zeros((nq, max(k, 1)), np.uint64), np.zeros((nq, max(k, 1)), np.float32), np.zeros(nq, np.uint64)
            short = False
            for j in range(nq):
                c = int(cnt[j])
                codes, odd = [], []
                for i in idx[j, :c]:
                    v = t.metadata[int(i)].get(field)
                    try:
                        hash(v)
                    except TypeError:
                        if v not in odd:
                            odd.append(v)
                        v = ("unhashable", odd.index(v), id(odd))
                    codes.append(v)
                kept = cap_groups(codes, group_size, k)
                short = short or (len(kept) < k and c == kk and kk < n)
                o_cnt[j] = len(kept)
                o_idx[j, :len(kept)] = idx[j, kept]
                o_dist[j, :len(kept)] = dist[j, kept]
            if not short:
                return o_idx[:, :k], o_dist[:, :k], o_cnt
            kk = min(kk * 4, n)

    def search_within(self, key: str, query, upper_bound: float, limit: int | None = None, filter: dict[str, str] | None = None,
                      with_vectors: bool = False):
        """Every row within `upper_bound` of the query (distance <= upper_bound, as search's filter compares), nearest first: what
        search(k, upper_bound=...) returns once k covers the whole set, without having to guess k.  Always answered exactly from the
        table's rows (FlatIndex::knn distances), whatever indexes the table has.  `limit`: at most that many, the nearest ones.
        `filter`: a metadata pattern as in search -- only matching rows are returned.  `with_vectors`: as in search."""
        t = self._t(key)
        q = np.asarray(query, dtype=np.float32).ravel()
        if filter is not None:
            t.prepare([filter])
        with t.lock.read():
            if filter is not None:
                _, idx, dist = t.index.range_search(q, np.float32(upper_bound), limit, mask=t.mask_for(filter))
                if with_vectors:
                    return self._hits_with_vectors(t, [idx], [dist], None)[0]
                return [(dict(t.metadata[int(i)]), float(d)) for i, d in zip(idx, dist)]
            _, idx, dist = t.index.range_search(q, np.float32(upper_bound), limit)
            if with_vectors:
                return self._hits_with_vectors(t, [idx], [dist], None)[0]
            return [(dict(t.metadata[int(i)]), float(d)) for i, d in zip(idx, dist)]

    def batch_search_within(self, key: str, queries, upper_bound, limit: int | None = None, filters=None, with_vectors: bool = False):
        """search_within for a batch of queries in ONE library call: entry q of the returned list is what search_within(key,
        queries[q], upper_bound[q], limit, filter_q) returns.  `upper_bound`: one value, or one per query.  `filters`: None, ONE
        metadata pattern for every query, or a list of len(queries) patterns ({} matches every row).  With filters the batch is one
        range_search_multi call over one mask per distinct pattern; without, one range_search call.  `with_vectors`: as in batch_search."""
        t = self._t(key)
        ix = t.index
        q = np.asarray(queries, dtype=np.float32)
        if q.ndim != 2 or q.shape[1] != ix.dim:
            raise RuntimeError(f"Dimension mismatch: table dim {ix.dim}, got {q.shape}")
        nq = q.shape[0]
        if filters is not None and not isinstance(filters, dict) and not is_expression(filters):
            filters = list(filters)
            if len(filters) != nq:
                raise RuntimeError(f"filters: one pattern per query is needed ({nq}), got {len(filters)}")
        ub = np.asarray(upper_bound, dtype=np.float32).reshape(-1)
        if ub.shape[0] not in (1, nq):
            raise RuntimeError(f"upper_bound: one value, or one per query ({nq}), got {ub.shape[0]}")
        if nq == 0:
            return []
        pats = None
        if filters is not None:
            pats = [filters] * nq if isinstance(filters, dict) or is_expression(filters) else filters
            t.prepare(pats)
        with t.lock.read():  # one read guard for the whole batch, mask building and metadata lookup included
            if pats is not None:
                slot: dict[object, int] = {}
                distinct, mask_of = [], np.zeros(nq, dtype=np.uint32)
                for i, p in enumerate(pats):
                    pk = filter_key(p)
                    if pk not in slot:
                        slot[pk] = len(distinct)
                        distinct.append(p)
                    mask_of[i] = slot[pk]
                masks = t.masks_for(distinct)  # the ones not cached yet: one library call
                lims, idx, dist = ix.range_search_multi(q, ub, masks, mask_of, limit)
            else:
                lims, idx, dist = ix.range_search(q, ub, limit)
            if with_vectors:
                return self._hits_with_vectors(t, [idx[int(lims[j]):int(lims[j + 1])] for j in range(nq)],
                                               [dist[int(lims[j]):int(lims[j + 1])] for j in range(nq)], None)
            return [[(dict(t.metadata[int(i)]), float(d)) for i, d in zip(idx[int(lims[j]):int(lims[j + 1])], dist[int(lims[j]):int(lims[j + 1])])]
                    for j in range(nq)]

    @staticmethod
    def _dup_rows(t: _Table, radius: float, filter, limit):
        """UNDER THE TABLE'S LOCK: (matched, groups, stats) of GpuIndex.dup_groups under the filter's mask -- matched: the ascending rows
        the filter matches (None without a filter: every row); groups: the groups of at least two rows, each the ascending array of its
        rows (so the representative, the lowest row, comes first), ordered by representative; stats: the call's dict."""
        mk = None if filter is None else t.mask_for(filter)
        group, stats = t.index.dup_groups(radius, mk, limit)
        matched = None if mk is None else mk.rows()[1]
        rows = np.arange(group.shape[0], dtype=np.int64) if matched is None else np.asarray(matched, dtype=np.int64)
        counts = np.unique(group[rows], return_counts=True)[1]  # (per representative, ascending)
        order = np.argsort(group[rows], kind="stable")      # (rows ascending: a stable sort by representative keeps them so)
        groups, at = [], 0
        for c in counts.tolist():
            if c >= 2:
                groups.append(rows[order[at:at + c]])
            at += c
        return matched, groups, stats

    def find_duplicates(self, key: str, radius: float, filter=None, limit: int | None = None):
        """(groups, truncated): the groups of at least two rows that lie within `radius` of each other, by SINGLE LINKAGE -- rows A and C
        share a group when a chain A-B-..-C of rows exists whose neighbours are within `radius` (the distance search_within compares),
        even when d(A, C) > radius.  Each group is the list of its rows' metadata dicts in ascending row order, the representative (the
        lowest row) first; the groups are ordered by representative.  `filter`: a pattern, a pattern with predicates or an expression, as
        in search -- only matching rows are grouped, and a row outside it never bridges two inside.  `limit`: every row looks at its
        `limit` nearest rows within the radius only (itself included); each group is then a subset of a true one, and `truncated` counts
        the rows whose list was full.  One library call (GpuIndex.dup_groups) under the read lock."""
        t = self._t(key)
        if filter is not None:
            t.prepare([filter])
        with t.lock.read():
            _, groups, stats = self._dup_rows(t, radius, filter, limit)
            return [[dict(t.metadata[int(r)]) for r in g] for g in groups], stats["truncated"]

    def mark_duplicates(self, key: str, radius: float, field: str, filter=None, limit: int | None = None) -> tuple[int, int]:
        """Writes find_duplicates' grouping into the metadata key `field`: first `field` is REMOVED from every row the filter matches
        (every row without one), then every row of a group of at least two gets the decimal ordinal of its group ("0", "1", ..: the
        order find_duplicates lists them in).  Rows alone keep no value, and under group_by a row without the key is always kept, so
        search(..., group_by=field, group_size=1) then returns at most one hit per duplicate group and every unique row.  Returns
        (groups, rows in them).  The write goes the way batch_update_metadata's does: ONE GpuIndex.set_labels_rows call when `field`
        has a label column, then the host dicts, then exactly the cached masks that name `field` are dropped; ids, vectors, HNSW and PQ
        state stay."""
        t = self._t(key)
        if filter is not None:
            t.prepare([filter])
        with t.lock.write():
            matched, groups, _ = self._dup_rows(t, radius, filter, limit)
            rows = np.arange(len(t.metadata), dtype=np.int64) if matched is None else np.asarray(matched, dtype=np.int64)
            value: dict[int, str] = {int(r): str(g) for g, members in enumerate(groups) for r in members.tolist()}
            touched = [r for r in rows.tolist() if r in value or field in t.metadata[r]]
            if touched:
                col = t.codec.column_of(field)
                if col is not None:
                    codes = np.array([[t.codec.encode_value(field, value.get(r)) for r in touched]], dtype=np.uint32)
                    t.index.set_labels_rows(np.asarray(touched, dtype=np.uint64), [col], codes)
                for r in touched:
                    self._apply_changes(t.metadata[r], {field: value.get(r)})
                t.drop_masks_naming([field])
            return len(groups), len(value)

    def delete_duplicates(self, key: str, radius: float, filter=None, limit: int | None = None) -> int:
        """Removes every row of a find_duplicates group except its representative (the lowest row); returns the number removed.  ONE
        GpuIndex.remove_rows call; the metadata follow the moves it reports, and the HNSW index and the PQ table are cleared, as delete
        does.  Because the grouping is single linkage, the representatives that remain may again lie within `radius` of each other
        through a row that is gone: a second call at the same radius need not return 0."""
        t = self._t(key)
        if filter is not None:
            t.prepare([filter])
        with t.lock.write():
            _, groups, _ = self._dup_rows(t, radius, filter, limit)
            gone = sorted(int(r) for g in groups for r in g[1:].tolist())
            t.drop_masks()
            t.index.hnsw_clear()
            t.index.pq_clear()
            if gone:
                dst, src = t.index.remove_rows(gone)
                for d, s in zip(dst.tolist(), src.tolist()):
                    t.metadata[d] = t.metadata[s]
                del t.metadata[len(t.metadata) - len(gone):]
            return len(gone)

    def count(self, key: str, filter=None) -> int:
        """the number of rows that match `filter` -- a pattern, a pattern with predicates or an expression, handled exactly as search
        handles it -- from the count of its cached mask; no filter: get_len"""
        t = self._t(key)
        if filter is not None:
            t.prepare([filter])
        with t.lock.read():
            return len(t.index) if filter is None else len(t.mask_for(filter))

    def count_by(self, key: str, field: str, filter=None) -> dict:
        """{value: rows} over the values of the metadata key `field` among the rows that match `filter` (every row without one); rows
        without the key are counted under None; values no matching row carries are left out.  `field` gets a label column on first
        use, as a filter key does, and the answer is then ONE pass over that column on the device (GpuIndex.label_counts over every
        code of the column's dictionary, under the filter's mask).  A field that cannot have a column (a 17th key) or whose column
        holds values a dictionary cannot keep apart is counted by the host loop over the metadata."""
        t = self._t(key)
        t.prepare(([] if filter is None else [filter]) + [{field: None}])
        with t.lock.read():
            mk = None if filter is None else t.mask_for(filter)
            vc = t.codec.value_codes(field)
            if vc is not None:
                values, codes = vc
                cnt = t.index.label_counts(t.codec.column_of(field), codes + [LABEL_NONE], mk)
                return {v: int(c) for v, c in zip(values + [None], cnt.tolist()) if c}
            rows = range(len(t.metadata)) if mk is None else mk.rows()[1].tolist()
            return dict(collections.Counter(t.metadata[i].get(field) for i in rows))

    def get(self, key: str, filter=None, limit: int | None = None):
        """(vectors, metadata) of the rows that match `filter`, ascending by row: an (m, dim) float32 array and the list of the rows'
        metadata dicts.  `filter`: a pattern, a pattern with predicates or an expression, resolved exactly as count resolves it; None:
        every row.  `limit`: the first `limit` matching rows.  The vectors come from ONE library call under the read lock
        (GpuIndex.get_rows_mask over the filter's cached mask; get_rows over a run of rows without a filter or under a limit)."""
        if limit is not None and int(limit) < 0:
            raise ValueError("limit must be at least 0")
        t = self._t(key)
        if filter is not None:
            t.prepare([filter])
        with t.lock.read():
            ix = t.index
            if filter is None:
                m = len(ix) if limit is None else min(int(limit), len(ix))
                return ix.get_rows(np.arange(m, dtype=np.uint64)), [dict(x) for x in t.metadata[:m]]
            mk = t.mask_for(filter)
            if limit is None or int(limit) >= len(mk):
                rows = mk.rows()[1]
                return ix.get_rows_mask(mk), [dict(t.metadata[int(i)]) for i in rows]
            rows = mk.rows()[1][:int(limit)]
            return ix.get_rows(rows), [dict(t.metadata[int(i)]) for i in rows]

    def extract_data(self, key: str):
        t = self._t(key)
        with t.lock.read():
            n = len(t.index)
            vecs = t.index.get_rows(np.arange(n, dtype=np.uint64))  # ONE call (a run of rows: one copy out of the table)
            return [(vecs[i].tolist(), dict(t.metadata[i])) for i in range(n)]

    @staticmethod
    def _hits_with_vectors(t: _Table, idx_per_query, dist_per_query, ub):
        """UNDER THE READ LOCK: per query the entries (metadata, distance, vector) of its hits (ids / distances already cut at the
        query's count) with distance <= ub (None: all of them).  The vectors of all hits of the call come from ONE get_rows call over
        the hit ids; a call without a hit makes none."""
        hits = [[(int(i), float(d)) for i, d in zip(ids, ds) if ub is None or d <= ub] for ids, ds in zip(idx_per_query, dist_per_query)]
        flat = np.fromiter((i for h in hits for i, _ in h), dtype=np.uint64)
        vecs = t.index.get_rows(flat) if flat.size else np.zeros((0, t.index.dim), dtype=np.float32)
        out, at = [], 0
        for h in hits:
            out.append([(dict(t.metadata[i]), d, vecs[at + r].copy()) for r, (i, d) in enumerate(h)])
            at += len(h)
        return out


__all__ = ["VecDB", "VdbError"]
