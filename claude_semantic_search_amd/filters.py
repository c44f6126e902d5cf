"""Filter dicts compiled into ``IndexFlat.where`` clauses (``StorageConfig.attribute_filters``).

``HybridStorage._matches_filters`` (``src/storage.py:508-543`` of the reference) decides a filter one chunk at a time in
Python.  ``AttrCatalog`` keeps, for every filterable column of the ``chunks`` table, the int32 code of every index row
and what a code means; ``compile_filters`` turns a filter dict into clauses over those codes whose answer on the device
is, row by row, the answer of ``_matches_filters`` -- or returns ``None`` when it cannot promise that, and the caller
falls back to the host loop.  Pure Python and numpy: nothing here touches the library.

Codes.  ``project_name``, ``session_id``, ``chunk_type``, ``file_path``: the position of the string in a dictionary in
order of first appearance, NULL as ``-1``.  ``has_code``, ``has_tools``: 0 / 1.  ``word_count``, ``char_count``,
``message_count``: the value itself.  ``timestamp``: the RANK of the value among the sorted distinct stored values
under Python's own comparison, NULL as ``-1``; a bound becomes a ``bisect`` position in that list, so the integer
comparison on the device decides exactly what the string comparison of ``_matches_filters`` decides, whatever the
format of the timestamps.  A row without a live chunk has ``-1`` everywhere (the tombstone mask leaves it out)."""
from __future__ import annotations

from bisect import bisect_left, bisect_right
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

DICT_COLUMNS = ("project_name", "session_id", "chunk_type", "file_path")
FLAG_COLUMNS = ("has_code", "has_tools")
INT_COLUMNS = ("word_count", "char_count", "message_count")
RANK_COLUMNS = ("timestamp",)
ATTR_COLUMNS = DICT_COLUMNS + FLAG_COLUMNS + INT_COLUMNS + RANK_COLUMNS      # the slot of a column is its position here
# every key a chunk row has (``SELECT * FROM chunks``): a filter key outside this set is ignored, as on the host
CHUNK_KEYS = frozenset(ATTR_COLUMNS + ("id", "text", "metadata", "faiss_id", "created_at", "updated_at"))
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
MAX_TABLE_BITS = 1 << 27
_RANGE = {"gte": ">=", "lte": "<=", "gt": ">", "lt": "<"}

Clause = Tuple[int, str, Any]


class AttrCatalog:
    """The codes of rows ``[0, rows)`` per column and their meaning.  ``extend`` appends rows and says what to push."""

    def __init__(self) -> None:
        self.rows = 0
        self.codes: Dict[str, np.ndarray] = {c: np.zeros(0, np.int32) for c in ATTR_COLUMNS}
        self.words: Dict[str, Dict[str, int]] = {c: {} for c in DICT_COLUMNS}        # value -> code
        self.sorted: Dict[str, List[str]] = {c: [] for c in RANK_COLUMNS}             # code -> value, ascending
        self.has_null = {c: False for c in ATTR_COLUMNS}     # a live chunk with NULL in the column
        self.mixed: Dict[str, Optional[str]] = {c: None for c in ATTR_COLUMNS}    # why the column cannot be filtered here

    def slot(self, column: str) -> int:
        return ATTR_COLUMNS.index(column)

    def values(self, column: str) -> list:
        """``values[code]`` of a dictionary, flag or rank column."""
        if column in DICT_COLUMNS:
            return list(self.words[column])
        return [False, True] if column in FLAG_COLUMNS else list(self.sorted[column])

    def extend(self, chunks: Sequence[Optional[Dict[str, Any]]]) -> Dict[str, int]:
        """Append one entry per index row (the chunk's row as a mapping, ``None`` for a row without a live chunk);
        returns ``{column: first row whose code is new or changed}`` -- the tail, or 0 for a rank column whose earlier
        codes moved because a value arrived that sorts in front of a stored one."""
        n, lo = len(chunks), self.rows
        first = {c: lo for c in ATTR_COLUMNS}
        for col in ATTR_COLUMNS:
            raw = [None if ch is None else ch.get(col) for ch in chunks]
            live = [ch is not None for ch in chunks]
            if any(v is None and ok for v, ok in zip(raw, live)):
                self.has_null[col] = True
            out = np.full(n, -1, dtype=np.int64)
            if col in DICT_COLUMNS:
                words = self.words[col]
                for i, v in enumerate(raw):
                    if isinstance(v, str):
                        out[i] = words.setdefault(v, len(words))
                    elif v is not None:
                        self.mixed[col] = f"{col} holds a value that is not a string"
            elif col in RANK_COLUMNS:
                order = self.sorted[col]
                for v in raw:
                    if v is not None and not isinstance(v, str):
                        self.mixed[col] = f"{col} holds a value that is not a string"
                new = sorted({v for v in raw if isinstance(v, str)} - set(order))
                if new:
                    merged = sorted(order + new)
                    if order and new[0] < order[-1]:      # stored codes move: re-rank them
                        remap = np.array([bisect_left(merged, v) for v in order], dtype=np.int32)
                        old = self.codes[col]
                        self.codes[col] = np.where(old >= 0, remap[np.maximum(old, 0)], -1).astype(np.int32)
                        first[col] = 0
                    self.sorted[col] = order = merged
                for i, v in enumerate(raw):
                    if isinstance(v, str):
                        out[i] = bisect_left(order, v)
            else:
                flag = col in FLAG_COLUMNS
                for i, v in enumerate(raw):
                    if v is None:
                        continue
                    if isinstance(v, (bool, int, np.integer)) and (not flag or v in (0, 1)) and I32_MIN <= int(v) <= I32_MAX:
                        out[i] = int(v)
                    else:
                        self.mixed[col] = f"{col} holds a value that is not " + ("0 / 1" if flag else "an int32")
                if not flag and self.has_null[col]:
                    self.mixed[col] = f"{col} holds a NULL (an int32 column has no code for it)"
            self.codes[col] = np.concatenate([self.codes[col], out.astype(np.int32)])
        self.rows += n
        return first


def _as_int(v) -> Optional[int]:
    """The integer a stored int compares equal to (``True == 1``, ``10.0 == 10``); ``None`` when there is none."""
    if isinstance(v, (bool, int, np.integer)):
        return int(v)
    if isinstance(v, (float, np.floating)) and v == v and abs(v) != float("inf") and float(v).is_integer():
        return int(v)
    return None


def compile_filters(filters: Optional[Dict[str, Any]], catalog: AttrCatalog, why: Optional[list] = None) -> Optional[List[Clause]]:
    """``filters`` as a list of ``(slot, op, operand)`` clauses for ``IndexFlat.where`` whose conjunction holds for
    exactly the rows of LIVE chunks that ``_matches_filters`` accepts; ``None`` when that cannot be promised (the reason
    is appended to ``why``) and the caller must use the host loop.  Keys that are not chunk columns are ignored, as on
    the host.  Exact match: ``==``; a list: ``in``; the case-insensitive ``project_name`` substring: ``in`` over the
    dictionary entries that contain it; range dicts: ``>= <= > <``.  A filter no row can pass becomes ``in []``."""
    def decline(reason: str):
        if why is not None:
            why.append(reason)
        return None

    never = lambda s: (s, "in", [])   # noqa: E731
    out: List[Clause] = []
    for key, want in (filters or {}).items():
        if key not in CHUNK_KEYS:
            continue
        if key not in ATTR_COLUMNS:
            return decline(f"{key} is a chunk column without an attribute slot")
        if catalog.mixed[key]:
            return decline(f"mixed-type column: {catalog.mixed[key]}")
        s = catalog.slot(key)
        numeric = key in FLAG_COLUMNS + INT_COLUMNS
        if isinstance(want, dict):
            for op, bound in want.items():
                if op not in _RANGE:
                    return decline(f"unknown op {op!r} on {key}")
                if catalog.has_null[key]:
                    return decline(f"a NULL under a range op on {key} (the host comparison raises)")
                if numeric:
                    if isinstance(bound, (bool, int, np.integer)):
                        if not I32_MIN <= int(bound) <= I32_MAX:
                            return decline(f"a value outside int32 on {key}")
                        out.append((s, _RANGE[op], int(bound)))
                    else:
                        return decline(f"a range bound on {key} that is not an integer")
                elif key in RANK_COLUMNS:
                    if not isinstance(bound, str):
                        return decline(f"a range bound on {key} that is not a string")
                    order = catalog.sorted[key]
                    lo, hi = bisect_left(order, bound), bisect_right(order, bound)
                    out.append({"gte": (s, ">=", lo), "gt": (s, ">=", hi), "lte": (s, "<=", hi - 1), "lt": (s, "<=", lo - 1)}[op])
                else:
                    return decline(f"a range on the dictionary column {key}")
        elif isinstance(want, list):
            if any(w is None for w in want):
                return decline(f"None in a list on {key}")
            if numeric:
                members = {m for m in (_as_int(w) for w in want) if m is not None and I32_MIN <= m <= I32_MAX}
                if any(m < 0 or m >= MAX_TABLE_BITS for m in members):
                    return decline(f"a list member on {key} outside [0, 2^27)")
            elif key in RANK_COLUMNS:
                order = catalog.sorted[key]
                at = [(w, bisect_left(order, w)) for w in want if isinstance(w, str)]
                members = {i for w, i in at if i < len(order) and order[i] == w}
            else:
                members = {catalog.words[key][w] for w in want if isinstance(w, str) and w in catalog.words[key]}
            out.append((s, "in", sorted(members)))
        elif want is None:
            return decline(f"None as the value of {key}")
        elif key == "project_name" and isinstance(want, str):
            needle = want.lower()
            out.append((s, "in", sorted(code for word, code in catalog.words[key].items() if needle in word.lower())))
        elif numeric:
            m = _as_int(want)
            if m is not None and not I32_MIN <= m <= I32_MAX:
                return decline(f"a value outside int32 on {key}")
            if key in FLAG_COLUMNS and m not in (0, 1):
                m = None                                    # (a code of -1 is a NULL, which equals nothing)
            out.append(never(s) if m is None else (s, "==", m))
        elif key in RANK_COLUMNS:
            order = catalog.sorted[key]
            at = bisect_left(order, want) if isinstance(want, str) else len(order)
            out.append((s, "==", at) if at < len(order) and order[at] == want else never(s))
        else:
            code = catalog.words[key].get(want) if isinstance(want, str) else None
            out.append(never(s) if code is None else (s, "==", code))
    if len(out) > 16:
        return decline("more than 16 clauses")
    return out
