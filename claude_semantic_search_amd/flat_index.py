"""Flat exact index on the MI355X, duck-typing what the reference uses of faiss.

The reference touches exactly these faiss members: the classes
``IndexFlatIP`` / ``IndexFlatL2`` (``src/storage.py:256-258``), ``index.ntotal``
(``:358``, ``:421``), ``index.add(x)`` (``:359``), ``index.search(q, k)``
(``:436``), ``faiss.read_index`` / ``write_index`` (``:306``, ``:879-884``,
``:895``, ``:913``) and the device toggles ``index_cpu_to_gpu`` /
``index_gpu_to_cpu`` / ``StandardGpuResources`` / ``get_num_gpus`` (``:274-296``,
``src/gpu_utils.py:117-118``).  This module provides the same names over
``libcss_hip.so``; the index always lives in HBM (there is no CPU index).
"""
from __future__ import annotations

import ctypes
import math
import struct
from typing import Callable, List, NamedTuple, Optional, Tuple

import numpy as np

from . import _native as nat

METRIC_INNER_PRODUCT = nat.METRIC_IP
METRIC_L2 = nat.METRIC_L2


def _as_f32_2d(x, d: int, what: str) -> np.ndarray:
    a = np.ascontiguousarray(x, dtype=np.float32)
    if a.ndim == 1:
        a = a.reshape(1, -1)
    if a.ndim != 2 or a.shape[1] != d:
        raise ValueError(f"{what}: expected shape (n, {d}), got {tuple(np.shape(x))}")
    return a


MAX_K = nat.MAX_K


def pack_allow_bits(allow, ntotal: int) -> np.ndarray:
    """Boolean row mask -> the uint32 bitmap of ``css_index_search_masked`` (bit r & 31 of word r >> 5)."""
    m = np.asarray(allow)
    if m.dtype != np.bool_ or m.ndim != 1 or m.shape[0] != ntotal:
        raise ValueError(f"allow must be a boolean array of ntotal={ntotal} entries")
    by = np.packbits(m, bitorder="little")
    words = (ntotal + 31) // 32
    out = np.zeros(words * 4, dtype=np.uint8)
    out[: by.shape[0]] = by
    return out.view("<u4")


def keep_mask_from_ids(ids, ntotal: int) -> np.ndarray:
    """What ``remove_ids`` is given -> boolean keep mask of ``ntotal`` entries (True = the row stays).

    ``ids`` is an array-like of integer row ids, or a boolean mask of length ``ntotal`` meaning "remove".  faiss'
    semantics: ids outside ``[0, ntotal)`` and repeated ids are ignored, so the number of rows removed is
    ``ntotal - keep.sum()``.  A mask of another length and ids that are not integers raise ``ValueError``."""
    a = np.asarray(ids)
    if a.dtype == np.bool_:
        if a.ndim != 1 or a.shape[0] != ntotal:
            raise ValueError(f"remove_ids: a boolean mask must have ntotal={ntotal} entries, got shape {a.shape}")
        return ~a
    if a.size == 0:
        return np.ones(ntotal, dtype=np.bool_)
    if not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"remove_ids: ids must be integers or a boolean mask, got dtype {a.dtype}")
    a = a.reshape(-1)
    if a.dtype == np.uint64:
        a = a[a < np.uint64(ntotal)]
    a = a.astype(np.int64, copy=False)
    keep = np.ones(ntotal, dtype=np.bool_)
    keep[a[(a >= 0) & (a < ntotal)]] = False
    return keep


def ids_as_int64(ids, what: str = "search_by_ids") -> np.ndarray:
    """Array-like of integer row ids -> contiguous 1-D int64 array; anything else (floats, booleans, strings, ids
    beyond int64) raises ``ValueError``."""
    a = np.asarray(ids)
    if a.size == 0:
        return np.zeros(0, dtype=np.int64)
    if not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"{what}: ids must be integers, got dtype {a.dtype}")
    a = a.reshape(-1)
    if a.dtype == np.uint64 and bool((a > np.uint64(np.iinfo(np.int64).max)).any()):
        raise ValueError(f"{what}: id beyond int64")
    return np.ascontiguousarray(a, dtype=np.int64)


def drop_self(D: np.ndarray, I: np.ndarray, ids: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """Host statement of the library's ``k_drop_self``: ``[nq, k + 1]`` sorted results -> ``[nq, k]`` without the
    anchor ``ids[j]`` of row ``j`` -- its entry goes where it is present, the last entry otherwise; order is kept.
    (The sharded index drops the anchor here, after the merge of the shards' lists.)"""
    nq, kk = I.shape
    gone = I == np.asarray(ids, dtype=np.int64).reshape(-1, 1)
    pos = np.where(gone.any(axis=1), gone.argmax(axis=1), kk - 1)
    keep = np.arange(kk)[None, :] != pos[:, None]
    return (np.ascontiguousarray(D[keep].reshape(nq, kk - 1)), np.ascontiguousarray(I[keep].reshape(nq, kk - 1)))


MAX_GROUP_K = nat.MAX_GROUP_K


def labels_as_int32(labels, what: str = "set_groups") -> np.ndarray:
    """Array-like of integer group labels -> contiguous 1-D int32 array; anything else (floats, booleans, strings,
    more than one dimension, values beyond int32) raises ``ValueError``.  Negative labels mean "ungrouped"."""
    a = np.asarray(labels)
    if a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"{what}: labels must be integers, got dtype {a.dtype}")
    if a.ndim != 1:
        raise ValueError(f"{what}: labels must be one-dimensional, got shape {a.shape}")
    if a.size and (int(a.min()) < np.iinfo(np.int32).min or int(a.max()) > np.iinfo(np.int32).max):
        raise ValueError(f"{what}: label beyond int32")
    return np.ascontiguousarray(a, dtype=np.int32)


def collapse_groups(D, I, G, k: int, metric: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The collapse rule of ``search_grouped``, stated in numpy for best-first lists that already carry labels:
    ``D, I, G`` are ``[nq, kk]`` (scores, ids, group labels; pads ``I = -1`` at the tail).  An entry survives iff its
    label is negative (an ungrouped row is a group of its own) or no earlier entry of its row has the same label; the
    first ``k`` survivors are returned in order as ``[nq, k]``, padded like ``search`` with ``G = -1``.  Because the
    list is best first, a survivor is the best row of its group, and every group absent from the list has its best
    row below the list's last entry.  (The sharded index merges the shards' grouped lists with this.)"""
    D, I, G = np.asarray(D, np.float32), np.asarray(I, np.int64), np.asarray(G, np.int32)
    nq, kk = I.shape
    k = int(k)
    Do = np.full((nq, k), -np.finfo(np.float32).max if metric == METRIC_INNER_PRODUCT else np.finfo(np.float32).max,
                 dtype=np.float32)
    Io = np.full((nq, k), -1, dtype=np.int64)
    Go = np.full((nq, k), -1, dtype=np.int32)
    for j in range(nq):
        first = np.zeros(kk, dtype=np.bool_)
        first[np.unique(G[j], return_index=True)[1]] = True   # first occurrence of every label value
        sel = np.flatnonzero((I[j] >= 0) & (first | (G[j] < 0)))[:k]
        Do[j, :sel.size], Io[j, :sel.size] = D[j, sel], I[j, sel]
        Go[j, :sel.size] = np.maximum(G[j, sel], -1)
    return Do, Io, Go


MAX_FACET_BUCKETS = nat.MAX_FACET_BUCKETS


class FacetCounts(NamedTuple):
    """What ``facets`` returns: per query and bucket the number of hits (``counts`` int64 ``[nq, nb]``) and the best
    hit (``best_score`` float32, ``best_id`` int64 ``[nq, nb]``; an empty bucket has count 0, id ``-1`` and the score
    ``search`` pads with), and per query all hits (``total``) and those outside every bucket (``unbucketed``), int64
    ``[nq]``: ``total == counts.sum(1) + unbucketed``."""
    counts: np.ndarray
    best_score: np.ndarray
    best_id: np.ndarray
    total: np.ndarray
    unbucketed: np.ndarray


def facet_args(thresh, buckets, nbuckets, ntotal: int, what: str = "facets") -> Tuple[float, Optional[np.ndarray], int]:
    """The argument rules of ``facets``, stated once: ``(thresh, buckets as int32 or None, nbuckets)``.  ``thresh`` is a
    number, not NaN.  ``buckets`` is ``None`` (the ``set_groups`` labels; ``nbuckets`` is then required) or an integer
    array of ``ntotal`` entries that fit int32; ``nbuckets=None`` then means ``max(buckets) + 1``, at least 1.
    ``1 <= nbuckets <= MAX_FACET_BUCKETS``.  Anything else raises ``ValueError``."""
    thresh = float(thresh)
    if math.isnan(thresh):
        raise ValueError(f"{what}: the threshold is NaN")
    b = None
    if buckets is not None:
        b = labels_as_int32(buckets, what)
        if b.shape[0] != ntotal:
            raise ValueError(f"{what}: buckets must have ntotal={ntotal} entries, got {b.shape[0]}")
        if nbuckets is None:
            nbuckets = max(int(b.max()) + 1, 1) if b.size else 1
    elif nbuckets is None:
        raise ValueError(f"{what}: nbuckets is required when the buckets are the set_groups labels")
    if isinstance(nbuckets, (bool, np.bool_)) or not isinstance(nbuckets, (int, np.integer)):
        raise ValueError(f"{what}: nbuckets must be an integer, got {type(nbuckets).__name__}")
    nbuckets = int(nbuckets)
    if nbuckets < 1 or nbuckets > MAX_FACET_BUCKETS:
        raise ValueError(f"{what}: nbuckets={nbuckets} outside [1, {MAX_FACET_BUCKETS}]")
    return thresh, b, nbuckets


MAX_ATTRS = nat.MAX_ATTRS
MAX_CLAUSES = nat.MAX_CLAUSES
MAX_TABLE_BITS = nat.MAX_TABLE_BITS
ATTR_I32, ATTR_F32 = nat.ATTR_I32, nat.ATTR_F32
WHERE_OPS = nat.WHERE_OPS
_WHERE_IN = WHERE_OPS.index("in")


def attr_slot(slot, what: str = "set_attribute") -> int:
    """An attribute slot number as int; anything but an integer in ``[0, MAX_ATTRS)`` raises ``ValueError``."""
    if isinstance(slot, (bool, np.bool_)) or not isinstance(slot, (int, np.integer)):
        raise ValueError(f"{what}: the slot must be an integer, got {type(slot).__name__}")
    if slot < 0 or slot >= MAX_ATTRS:
        raise ValueError(f"{what}: attribute slot {int(slot)} outside [0, {MAX_ATTRS})")
    return int(slot)


def attr_values(values, what: str = "set_attribute") -> Tuple[np.ndarray, int]:
    """Array-like of per-row attribute values -> ``(contiguous 1-D array, ATTR_I32 | ATTR_F32)``: an integer (or
    boolean) dtype gives int32 and is range-checked, a floating dtype gives float32 (rounded; NaN and infinity are
    values like any other).  Anything else (strings, objects, complex, more than one dimension) raises ``ValueError``."""
    a = np.asarray(values)
    if a.ndim != 1:
        raise ValueError(f"{what}: values must be one-dimensional, got shape {a.shape}")
    if a.dtype == np.bool_ or np.issubdtype(a.dtype, np.integer):
        if a.size and (int(a.min()) < np.iinfo(np.int32).min or int(a.max()) > np.iinfo(np.int32).max):
            raise ValueError(f"{what}: value beyond int32")
        return np.ascontiguousarray(a, dtype=np.int32), ATTR_I32
    if np.issubdtype(a.dtype, np.floating):
        with np.errstate(over="ignore"):
            return np.ascontiguousarray(a, dtype=np.float32), ATTR_F32
    raise ValueError(f"{what}: values must be integers or real numbers, got dtype {a.dtype}")


class WhereArgs(NamedTuple):
    """What ``where_args`` returns: per clause ``(slot, op code, value bits as int32, table_off, table_bits)`` and the
    table words of the call (uint32; empty without ``in`` clauses)."""
    clauses: List[Tuple[int, int, int, int, int]]
    tables: np.ndarray


def where_args(clauses, type_of: Callable[[int], int], what: str = "where") -> WhereArgs:
    """The argument rules of ``where``, stated once, and the packing of the ``in`` tables.  ``clauses`` is a sequence
    of at most ``MAX_CLAUSES`` triples ``(slot, op, operand)`` with ``op`` one of ``WHERE_OPS``; ``type_of(slot)`` gives
    the slot's type (``ATTR_I32``, ``ATTR_F32`` or ``-1`` for a slot that was never set).  On an int32 slot the operand
    of a comparison is an integer that fits int32; on a float32 slot any real number, rounded to float32 (NaN and
    infinity included).  ``in`` / ``not in`` exist on int32 slots only; their operand is an iterable of non-negative
    integers below ``MAX_TABLE_BITS`` and becomes a bit table of ``max + 1`` bits (an empty iterable: no bits, nothing
    is in).  Anything else raises ``ValueError``."""
    try:
        clauses = list(clauses)
    except TypeError:
        raise ValueError(f"{what}: clauses must be a sequence of (slot, op, operand)") from None
    if len(clauses) > MAX_CLAUSES:
        raise ValueError(f"{what}: {len(clauses)} clauses, at most {MAX_CLAUSES}")
    out: List[Tuple[int, int, int, int, int]] = []
    tables: List[np.ndarray] = []
    words = 0
    for c, cl in enumerate(clauses):
        if not isinstance(cl, (tuple, list)) or len(cl) != 3:
            raise ValueError(f"{what}: clause {c} is not (slot, op, operand)")
        slot, op, operand = cl
        slot = attr_slot(slot, f"{what}: clause {c}")
        if not isinstance(op, str) or op not in WHERE_OPS:
            raise ValueError(f"{what}: clause {c}: unknown op {op!r} (one of {', '.join(WHERE_OPS)})")
        code = WHERE_OPS.index(op)
        typ = int(type_of(slot))
        if typ < 0:
            raise ValueError(f"{what}: clause {c}: attribute slot {slot} was never set")
        if code >= _WHERE_IN:
            if typ != ATTR_I32:
                raise ValueError(f"{what}: clause {c}: {op!r} on attribute slot {slot}, which holds float32 values")
            try:
                vals = np.asarray(list(operand))
            except TypeError:
                raise ValueError(f"{what}: clause {c}: the operand of {op!r} must be an iterable of integers") from None
            if vals.size and (vals.dtype == np.bool_ or not np.issubdtype(vals.dtype, np.integer)):
                raise ValueError(f"{what}: clause {c}: the operand of {op!r} must hold integers, got dtype {vals.dtype}")
            vals = vals.reshape(-1)
            if vals.size and (int(vals.min()) < 0 or int(vals.max()) >= MAX_TABLE_BITS):
                raise ValueError(f"{what}: clause {c}: the operand of {op!r} must lie in [0, {MAX_TABLE_BITS})")
            nbits = int(vals.max()) + 1 if vals.size else 0
            member = np.zeros(nbits, dtype=np.bool_)
            member[vals.astype(np.int64)] = True
            tab = pack_allow_bits(member, nbits)
            out.append((slot, code, 0, words, nbits))
            tables.append(tab)
            words += tab.shape[0]
            continue
        if isinstance(operand, (bool, np.bool_)):
            operand = int(operand)
        if typ == ATTR_I32:
            if not isinstance(operand, (int, np.integer)):
                raise ValueError(f"{what}: clause {c}: attribute slot {slot} holds int32 values; the operand of {op!r} must "
                                 f"be an integer, got {type(operand).__name__}")
            if operand < np.iinfo(np.int32).min or operand > np.iinfo(np.int32).max:
                raise ValueError(f"{what}: clause {c}: operand {int(operand)} beyond int32")
            out.append((slot, code, int(operand), 0, 0))
        else:
            if not isinstance(operand, (int, float, np.integer, np.floating)):
                raise ValueError(f"{what}: clause {c}: the operand of {op!r} must be a real number, got "
                                 f"{type(operand).__name__}")
            with np.errstate(over="ignore"):
                bits = int(np.asarray(operand, dtype=np.float32).reshape(1).view(np.int32)[0])
            out.append((slot, code, bits, 0, 0))
    tabs = np.concatenate(tables).astype("<u4") if tables else np.zeros(0, dtype="<u4")
    return WhereArgs(out, np.ascontiguousarray(tabs))


def where_numpy(columns, clauses, ntotal: int, allow=None) -> np.ndarray:
    """What ``where`` computes, stated in numpy (the tests compare the device with this): the boolean mask of the rows
    that pass every clause and ``allow``.  ``columns`` maps a slot to its int32 or float32 array of ``ntotal`` values;
    the comparisons are numpy's own on those dtypes (a NaN fails everything but ``!=``, ``-0.0 == 0.0``); a value is
    ``in`` when it equals one of the operand's members -- those are non-negative, so a negative value never is."""
    mask = np.ones(ntotal, dtype=np.bool_) if allow is None else np.array(allow, dtype=np.bool_, copy=True)
    typed = where_args(clauses, lambda s: ATTR_F32 if np.asarray(columns[s]).dtype == np.float32 else ATTR_I32, "where_numpy")
    for (slot, op, operand), (_, code, bits, _, _) in zip(clauses, typed.clauses):
        col = np.asarray(columns[slot])
        if col.shape != (ntotal,) or col.dtype not in (np.int32, np.float32):
            raise ValueError(f"where_numpy: column {slot} must be an int32 or float32 array of {ntotal} entries")
        if code >= _WHERE_IN:
            members = np.asarray(list(operand), dtype=np.int64).reshape(-1)
            ok = np.isin(col.astype(np.int64), members)
            ok = ok if code == _WHERE_IN else ~ok
        else:
            x = np.array([bits], dtype=np.int32).view(col.dtype)[0]   # the operand in the column's own dtype
            with np.errstate(invalid="ignore"):
                ok = (col == x, col != x, col < x, col <= x, col > x, col >= x)[code]
        mask &= ok
    return mask


MAX_PRIOR_K = nat.MAX_PRIOR_K


def priors_as_f32(priors, what: str = "set_priors") -> np.ndarray:
    """Array-like of real per-row priors -> contiguous 1-D float32 array; anything else (booleans, complex numbers,
    strings, objects, more than one dimension) raises ``ValueError``.  Values are not looked at here: the library
    refuses NaN and infinity and names the row."""
    a = np.asarray(priors)
    if a.dtype == np.bool_ or not (np.issubdtype(a.dtype, np.integer) or np.issubdtype(a.dtype, np.floating)):
        raise ValueError(f"{what}: priors must be real numbers, got dtype {a.dtype}")
    if a.ndim != 1:
        raise ValueError(f"{what}: priors must be one-dimensional, got shape {a.shape}")
    return np.ascontiguousarray(a, dtype=np.float32)


MAX_HYBRID_K = nat.MAX_HYBRID_K
MAX_QUERY_TERMS = nat.MAX_QUERY_TERMS


def hybrid_args(terms, weights, k, alpha, k1, b, avgdl, what: str = "search_hybrid"):
    """The checked arguments of a hybrid search: ``(terms uint32 [m], weights float32 [m], k, alpha, k1, b, avgdl)``;
    what the library would refuse raises ``ValueError`` here (``avgdl`` may still be ``None``)."""
    t = np.asarray(terms if terms is not None else (), dtype=np.int64).reshape(-1)
    w = np.ascontiguousarray(np.asarray(weights if weights is not None else (), dtype=np.float32).reshape(-1))
    if t.shape[0] != w.shape[0]:
        raise ValueError(f"{what}: {t.shape[0]} terms but {w.shape[0]} weights")
    if t.shape[0] > MAX_QUERY_TERMS:
        raise ValueError(f"{what}: {t.shape[0]} query terms (at most {MAX_QUERY_TERMS})")
    if t.size and (int(t.min()) < 0 or int(t.max()) >= nat.TERM_SPACE):
        raise ValueError(f"{what}: a term outside [0, 2^24)")
    uniq, counts = np.unique(t, return_counts=True)
    if (counts > 1).any():
        raise ValueError(f"{what}: term {int(uniq[counts > 1][0])} is repeated")
    if not np.isfinite(w).all():
        raise ValueError(f"{what}: the weight of term {int(t[~np.isfinite(w)][0])} is not finite")
    k, alpha, k1, b = int(k), float(alpha), float(k1), float(b)
    if k < 1 or k > MAX_HYBRID_K:
        raise ValueError(f"k={k} outside [1, {MAX_HYBRID_K}]")
    if not np.isfinite(alpha):
        raise ValueError(f"{what}: alpha={alpha} is not finite")
    if not np.isfinite(k1) or k1 < 0.0:
        raise ValueError(f"{what}: k1={k1} must be finite and >= 0")
    if not np.isfinite(b) or b < 0.0 or b > 1.0:
        raise ValueError(f"{what}: b={b} must lie in [0, 1]")
    if avgdl is not None:
        avgdl = float(avgdl)
        if not np.isfinite(avgdl) or avgdl <= 0.0:
            raise ValueError(f"{what}: avgdl={avgdl} must be finite and > 0")
    return np.ascontiguousarray(t, dtype=np.uint32), w, k, alpha, k1, b, avgdl


MAX_SPARSE_QUERY_TERMS = nat.MAX_SPARSE_QUERY_TERMS
MAX_SPARSE_WEIGHT = nat.MAX_SPARSE_WEIGHT


def sparse_args(terms, weights, k, alpha=None, what: str = "search_sparse"):
    """The checked arguments of a sparse search: ``(terms uint32 [m], weights float32 [m], k, alpha)``; what the library
    would refuse raises ``ValueError`` here.  ``terms`` may be a ``SparseVector`` (``weights=None``).  At most 64 distinct
    terms below 2^24; weights finite, nonzero and at most 65536 in size (negative ones are allowed); ``1 <= k <= 128``;
    ``alpha`` (hybrid only) finite."""
    if weights is None and isinstance(terms, tuple) and len(terms) == 2:
        terms, weights = terms
    t = np.asarray(terms if terms is not None else (), dtype=np.int64)
    w = np.asarray(weights if weights is not None else (), dtype=np.float32)
    if t.ndim > 1 or w.ndim > 1:
        raise ValueError(f"{what}: one query per call, got terms of shape {t.shape} and weights of shape {w.shape}")
    t, w = t.reshape(-1), np.ascontiguousarray(w.reshape(-1))
    if t.shape[0] != w.shape[0]:
        raise ValueError(f"{what}: {t.shape[0]} terms but {w.shape[0]} weights")
    if t.shape[0] > MAX_SPARSE_QUERY_TERMS:
        raise ValueError(f"{what}: {t.shape[0]} query terms (at most {MAX_SPARSE_QUERY_TERMS})")
    if t.size and (int(t.min()) < 0 or int(t.max()) >= nat.TERM_SPACE):
        raise ValueError(f"{what}: a term outside [0, 2^24)")
    uniq, counts = np.unique(t, return_counts=True)
    if (counts > 1).any():
        raise ValueError(f"{what}: term {int(uniq[counts > 1][0])} is repeated")
    bad = ~np.isfinite(w) | (w == 0.0) | (np.abs(w) > MAX_SPARSE_WEIGHT)
    if bad.any():
        raise ValueError(f"{what}: the weight {float(w[bad][0])} of term {int(t[bad][0])} must be finite, nonzero and at most "
                         f"{MAX_SPARSE_WEIGHT:g} in size")
    k = int(k)
    if k < 1 or k > MAX_HYBRID_K:
        raise ValueError(f"k={k} outside [1, {MAX_HYBRID_K}]")
    if alpha is not None:
        alpha = float(alpha)
        if not np.isfinite(alpha):
            raise ValueError(f"{what}: alpha={alpha} is not finite")
    return np.ascontiguousarray(t, dtype=np.uint32), w, k, alpha


def sparse_as_csr(vectors, what: str = "set_sparse") -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Sparse vectors as CSR ``(offsets int64 [n + 1] from 0, terms uint32, weights float32)``.  ``vectors`` is a
    sequence of ``SparseVector`` or ``(terms, weights)`` pairs (one per row, any order within a row, empty allowed) or
    an ``(offsets, terms, weights)`` triple of arrays.  What the library would refuse in the entries raises
    ``ValueError`` here and names the row (of this call): a term outside ``[0, 2^24)`` or repeated within a row, a
    weight that is not finite, not ``> 0`` or above 65536, a row of more than 65536 entries.  The shape of the offsets
    is the library's to check."""
    if isinstance(vectors, tuple) and len(vectors) == 3 and isinstance(vectors[0], np.ndarray):
        off = np.ascontiguousarray(vectors[0], dtype=np.int64).reshape(-1)
        t, w = np.asarray(vectors[1]).reshape(-1), np.asarray(vectors[2]).reshape(-1)
        if off.shape[0] < 1:
            raise ValueError(f"{what}: offsets must hold n + 1 values")
    else:
        rows = [(np.asarray(v[0]).reshape(-1), np.asarray(v[1]).reshape(-1)) for v in vectors]
        for r, (a, b) in enumerate(rows):
            if a.shape[0] != b.shape[0]:
                raise ValueError(f"{what}: row {r} (of this call) has {a.shape[0]} terms but {b.shape[0]} weights")
            if a.size and (a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer)):
                raise ValueError(f"{what}: the terms of row {r} (of this call) must be integers, got dtype {a.dtype}")
        off = np.zeros(len(rows) + 1, dtype=np.int64)
        if rows:
            np.cumsum([a.shape[0] for a, _ in rows], out=off[1:])
        t = np.concatenate([a.astype(np.int64) for a, _ in rows]) if rows else np.zeros(0, np.int64)
        w = np.concatenate([b.astype(np.float32) for _, b in rows]) if rows else np.zeros(0, np.float32)
    if t.shape[0] != w.shape[0]:
        raise ValueError(f"{what}: {t.shape[0]} terms but {w.shape[0]} weights")
    if t.size and (t.dtype == np.bool_ or not np.issubdtype(t.dtype, np.integer)):
        raise ValueError(f"{what}: terms must be integers, got dtype {t.dtype}")
    t = t.astype(np.int64)
    w = np.ascontiguousarray(w, dtype=np.float32)
    well_formed = off[0] == 0 and off[-1] == t.shape[0] and (np.diff(off) >= 0).all()
    row_of = (lambda e: int(np.searchsorted(off, e, side="right")) - 1) if well_formed else (lambda e: -1)
    bad = np.flatnonzero((t < 0) | (t >= nat.TERM_SPACE))
    if bad.size:
        raise ValueError(f"{what}: term {int(t[bad[0]])} of row {row_of(bad[0])} (of this call) is outside [0, 2^24)")
    bad = np.flatnonzero(~np.isfinite(w) | ~(w > 0.0) | (w > MAX_SPARSE_WEIGHT))
    if bad.size:
        raise ValueError(f"{what}: the weight {float(w[bad[0]])} of term {int(t[bad[0]])} of row {row_of(bad[0])} (of this call) "
                         f"must be finite, > 0 and <= {MAX_SPARSE_WEIGHT:g}")
    if well_formed:
        lens = np.diff(off)
        if lens.size and int(lens.max()) > nat.MAX_SPARSE_ROW_ENTRIES:
            raise ValueError(f"{what}: row {int(lens.argmax())} (of this call) has {int(lens.max())} entries "
                             f"(at most {nat.MAX_SPARSE_ROW_ENTRIES})")
        key = np.repeat(np.arange(lens.shape[0], dtype=np.int64), lens) << 24 | t
        uniq, counts = np.unique(key, return_counts=True)
        if (counts > 1).any():
            rep = int(uniq[counts > 1][0])
            raise ValueError(f"{what}: term {rep & (nat.TERM_SPACE - 1)} is repeated in row {rep >> 24} (of this call)")
    return off, np.ascontiguousarray(t, dtype=np.uint32), w


MAX_QUERY_TOKENS = nat.MAX_QUERY_TOKENS
MAX_ROW_TOKEN_VECTORS = nat.MAX_ROW_TOKEN_VECTORS
MAX_MAXSIM_ROWS = nat.MAX_MAXSIM_ROWS
MAX_MAXSIM_QUERIES = nat.MAX_MAXSIM_QUERIES
MAXSIM_BATCH_GROUP = nat.MAXSIM_BATCH_GROUP


def _bf16_bits(m, what: str, name: str) -> np.ndarray:
    """uint16 bf16 bit patterns of a token matrix: uint16 as it is, float32 only where every value IS a bf16 value (the
    low 16 bits are zero) -- rounding is the caller's decision, never a silent one.  ``name`` says whose matrix it is."""
    a = np.asarray(m)
    if a.dtype == np.uint16:
        return a
    if a.dtype != np.float32:
        raise ValueError(f"{what}: {name} must be uint16 (bf16 bits) or bf16-exact float32, got dtype {a.dtype}")
    u = np.ascontiguousarray(a).view(np.uint32)
    if (u & 0xFFFF).any():
        raise ValueError(f"{what}: {name} holds float32 values that are not bf16 values (round them first)")
    return (u >> 16).astype(np.uint16)


def _token_dim_ok(P: int) -> bool:
    return 32 <= P <= nat.MAX_TOKEN_DIM and P % 32 == 0


def tokens_as_csr(mats, keep=None, what: str = "set_tokens") -> Tuple[np.ndarray, np.ndarray, int]:
    """Token matrices as CSR ``(offsets int64 [n + 1] from 0 in tokens, tokens uint16 [offsets[n], P], P)``.  ``mats`` is
    a sequence of ``[m_i, P]`` matrices, uint16 bf16 bits or bf16-exact float32 (one per row, empty allowed), or an
    ``(offsets, tokens [E, P], P)`` triple.  ``keep`` (sequence form only; per row one flag per token, or ``None``) is
    ColBERT's skiplist as in ``LateInteraction.score``: a token whose flag is 0 is DROPPED here and not stored.  What
    the library would refuse raises ``ValueError`` here and names the row (of this call): a width that is not a
    multiple of 32 in [32, 128] or differs between rows, a NaN or infinite component, more than 512 tokens."""
    if isinstance(mats, tuple) and len(mats) == 3 and isinstance(mats[0], np.ndarray) and np.ndim(mats[2]) == 0:
        if keep is not None:
            raise ValueError(f"{what}: keep flags go with a sequence of matrices, not with the CSR form")
        off = np.ascontiguousarray(mats[0], dtype=np.int64).reshape(-1)
        P = int(mats[2])
        if off.shape[0] < 1:
            raise ValueError(f"{what}: offsets must hold n + 1 values")
        if not _token_dim_ok(P):
            raise ValueError(f"{what}: P={P} must be a multiple of 32 in [32, {nat.MAX_TOKEN_DIM}]")
        tok = _bf16_bits(mats[1], what, "the tokens")
        if tok.size % P:
            raise ValueError(f"{what}: {tok.size} components are no whole tokens of P={P}")
        tok = tok.reshape(-1, P)
    else:
        mats = list(mats)
        if keep is not None and len(keep) != len(mats):
            raise ValueError(f"{what}: {len(keep)} keep arrays for {len(mats)} matrices")
        rows, P = [], 0
        for r, m in enumerate(mats):
            a = _bf16_bits(m, what, f"the matrix of row {r} (of this call)")
            if a.ndim != 2:
                raise ValueError(f"{what}: the matrix of row {r} (of this call) has shape {a.shape}, not [m, P]")
            if not _token_dim_ok(a.shape[1]):
                raise ValueError(f"{what}: row {r} (of this call) has P={a.shape[1]}, not a multiple of 32 in "
                                 f"[32, {nat.MAX_TOKEN_DIM}]")
            if P and a.shape[1] != P:
                raise ValueError(f"{what}: row {r} (of this call) has P={a.shape[1]}, the rows before it P={P}")
            P = a.shape[1]
            if keep is not None and keep[r] is not None:
                f = np.asarray(keep[r]).reshape(-1) != 0
                if f.shape[0] != a.shape[0]:
                    raise ValueError(f"{what}: {f.shape[0]} keep flags for the {a.shape[0]} tokens of row {r} (of this call)")
                a = a[f]
            rows.append(a)
        P = P or 32   # (no row: nothing is stored, any width serves)
        off = np.zeros(len(rows) + 1, dtype=np.int64)
        if rows:
            np.cumsum([a.shape[0] for a in rows], out=off[1:])
        tok = np.concatenate(rows) if rows else np.zeros((0, P), np.uint16)
    tok = np.ascontiguousarray(tok, dtype=np.uint16)
    well_formed = off[0] == 0 and off[-1] == tok.shape[0] and (np.diff(off) >= 0).all()
    bad = np.flatnonzero(((tok & 0x7F80) == 0x7F80).any(axis=1))
    if bad.size:
        row = int(np.searchsorted(off, bad[0], side="right")) - 1 if well_formed else -1
        raise ValueError(f"{what}: token {int(bad[0] - off[row]) if well_formed else int(bad[0])} of row {row} (of this call) "
                         "has a NaN or infinite component")
    if well_formed:
        lens = np.diff(off)
        if lens.size and int(lens.max()) > MAX_ROW_TOKEN_VECTORS:
            raise ValueError(f"{what}: row {int(lens.argmax())} (of this call) has {int(lens.max())} tokens "
                             f"(at most {MAX_ROW_TOKEN_VECTORS})")
    return off, tok, P


def maxsim_args(q_mat, k=None, ids=None, what: str = "search_maxsim"):
    """The checked arguments of a MaxSim call: ``(q uint16 [mq, P], k or None, ids int64 [n] or None)``; what the library
    would refuse raises ``ValueError`` here.  ``q_mat`` is ONE ``[mq, P]`` matrix, uint16 bf16 bits or bf16-exact
    float32, ``1 <= mq <= 64``, P a multiple of 32 in [32, 128], finite; ``1 <= k <= 128``; at most 65536 ``ids``."""
    q = _bf16_bits(q_mat, what, "the query matrix")
    if q.ndim != 2:
        raise ValueError(f"{what}: one query matrix [mq, P] per call, got shape {q.shape}")
    if not 1 <= q.shape[0] <= MAX_QUERY_TOKENS:
        raise ValueError(f"{what}: {q.shape[0]} query tokens outside [1, {MAX_QUERY_TOKENS}]")
    if not _token_dim_ok(q.shape[1]):
        raise ValueError(f"{what}: P={q.shape[1]} must be a multiple of 32 in [32, {nat.MAX_TOKEN_DIM}]")
    q = np.ascontiguousarray(q, dtype=np.uint16)
    bad = np.flatnonzero(((q & 0x7F80) == 0x7F80).any(axis=1))
    if bad.size:
        raise ValueError(f"{what}: query token {int(bad[0])} has a NaN or infinite component")
    if k is not None:
        k = int(k)
        if k < 1 or k > MAX_HYBRID_K:
            raise ValueError(f"k={k} outside [1, {MAX_HYBRID_K}]")
    if ids is not None:
        ids = np.ascontiguousarray(np.asarray(ids, dtype=np.int64).reshape(-1))
        if ids.shape[0] > MAX_MAXSIM_ROWS:
            raise ValueError(f"{what}: {ids.shape[0]} ids (at most {MAX_MAXSIM_ROWS})")
    return q, k, ids


def maxsim_batch_args(q_mats, k, what: str = "search_maxsim_batch"):
    """The checked arguments of a batched MaxSim call: ``(offsets int64 [nq + 1], tokens uint16 [offsets[nq], P], k)``;
    what the library would refuse raises ``ValueError`` here and names the query.  ``q_mats`` is a sequence of 1 to 1024
    ``[mq_b, P]`` matrices, each as ``maxsim_args`` takes one, all of one P; ``1 <= k <= 128``."""
    mats = list(q_mats)
    if not 1 <= len(mats) <= MAX_MAXSIM_QUERIES:
        raise ValueError(f"{what}: {len(mats)} queries outside [1, {MAX_MAXSIM_QUERIES}]")
    qs, P = [], 0
    for b, m in enumerate(mats):
        q, _, _ = maxsim_args(m, what=f"{what}: query {b}")
        if P and q.shape[1] != P:
            raise ValueError(f"{what}: query {b} has P={q.shape[1]}, the queries before it P={P}")
        P = q.shape[1]
        qs.append(q)
    _, k, _ = maxsim_args(qs[0], k, what=what)
    off = np.zeros(len(qs) + 1, dtype=np.int64)
    np.cumsum([q.shape[0] for q in qs], out=off[1:])
    return off, np.ascontiguousarray(np.concatenate(qs), dtype=np.uint16), k


def rerank_args(q, q_mats, k, fetch, floor=None, d: Optional[int] = None, ids=None, what: str = "search_rerank_maxsim"):
    """The checked arguments of the list calls: ``(a float32 [nq, d] or None, offsets int64 [nq + 1], tokens uint16
    [offsets[nq], P], k or None, fetch, floor float, ids int64 [nq, fetch] or None)``; what the library would refuse raises
    ``ValueError`` here, before the library is called, and names the query.  ``q_mats`` as ``maxsim_batch_args`` takes
    them (1 to 1024 matrices of one P).  For ``search_rerank_maxsim``: ``q`` holds one dense row per matrix, ``1 <= fetch
    <= 2048``, ``1 <= k <= min(fetch, 128)``, ``floor`` a number or ``None`` (NaN: no floor).  For ``maxsim_ids_batch``
    (``q`` and ``k`` are ``None``): ``ids`` is ``[nq, f]`` with ``1 <= f <= 2048``, and ``fetch`` is taken from it."""
    off, tok, _ = maxsim_batch_args(q_mats, None, what=what)
    nq = off.shape[0] - 1
    if ids is not None:
        try:
            ids = np.ascontiguousarray(np.asarray(ids, dtype=np.int64))
        except (TypeError, ValueError):
            raise ValueError(f"{what}: ids must be an integer array [nq, f], one list per query") from None
        if ids.ndim != 2 or ids.shape[0] != nq:
            raise ValueError(f"{what}: ids of shape {ids.shape} for {nq} queries, expected [{nq}, f]")
        fetch = ids.shape[1]
    try:
        f = int(fetch)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: fetch={fetch!r} is no integer") from None
    if f != fetch or not 1 <= f <= nat.MAX_K:
        raise ValueError(f"{what}: {'f' if ids is not None else 'fetch'}={fetch!r} outside [1, {nat.MAX_K}]")
    a = None
    if q is not None:
        a = _as_f32_2d(q, int(d), what)
        if a.shape[0] != nq:
            raise ValueError(f"{what}: {a.shape[0]} dense queries for {nq} query matrices")
    if k is not None:
        try:
            kk = int(k)
        except (TypeError, ValueError):
            raise ValueError(f"{what}: k={k!r} is no integer") from None
        if kk != k or not 1 <= kk <= min(f, MAX_HYBRID_K):
            raise ValueError(f"{what}: k={k!r} outside [1, min(fetch={f}, {MAX_HYBRID_K})]")
        k = kk
    if floor is None:
        fl = float("nan")
    else:
        try:
            fl = float(floor)
        except (TypeError, ValueError):
            raise ValueError(f"{what}: floor={floor!r} is no number") from None
    return a, off, tok, k, f, fl, ids


MAX_TOKEN_CENTROIDS = 65536   # CSS_MAX_TOKEN_CENTROIDS
TOKEN_CODEC_BITS = (1, 2, 4)


class TokenCodec(NamedTuple):
    """A codec of token matrices (``css_index_set_token_codec``): ``centroids`` float32 ``[C, P]`` of bf16 values,
    ``nbits`` in {1, 2, 4}, ``cutoffs`` float32 ``[2^nbits - 1]`` strictly ascending, ``weights`` float32 ``[2^nbits]``."""
    centroids: np.ndarray
    nbits: int
    cutoffs: np.ndarray
    weights: np.ndarray

    @property
    def P(self) -> int:
        return int(self.centroids.shape[1])

    @property
    def res_bytes(self) -> int:
        """Bytes of packed buckets per token."""
        return self.P * int(self.nbits) // 8


def token_codec_args(centroids, nbits, cutoffs, weights, P: Optional[int] = None, what: str = "set_token_codec") -> TokenCodec:
    """The checked codec; what the library would refuse raises ``ValueError`` here: ``nbits`` not 1, 2 or 4, ``C``
    outside [1, 65536], a width that is no multiple of 32 in [32, 128] or differs from ``P`` (the width of the matrices
    it is to serve), a centroid component that is NaN, infinite or no bf16 value, cutoffs that are not ``2^nbits - 1``
    finite strictly ascending values, weights that are not ``2^nbits`` finite values."""
    try:
        nb = int(nbits)
    except (TypeError, ValueError):
        nb = -1
    if nb not in TOKEN_CODEC_BITS or nb != nbits:
        raise ValueError(f"{what}: nbits={nbits!r} is none of 1, 2, 4")
    c = np.asarray(centroids)
    if c.dtype != np.float32:
        raise ValueError(f"{what}: the centroids must be bf16-exact float32, got dtype {c.dtype}")
    if c.ndim != 2:
        raise ValueError(f"{what}: the centroids have shape {c.shape}, not [C, P]")
    if not 1 <= c.shape[0] <= MAX_TOKEN_CENTROIDS:
        raise ValueError(f"{what}: C={c.shape[0]} outside [1, {MAX_TOKEN_CENTROIDS}]")
    if not _token_dim_ok(c.shape[1]):
        raise ValueError(f"{what}: P={c.shape[1]} must be a multiple of 32 in [32, {nat.MAX_TOKEN_DIM}]")
    if P is not None and int(P) != c.shape[1]:
        raise ValueError(f"{what}: the centroids have P={c.shape[1]}, the token matrices P={int(P)}")
    c = np.ascontiguousarray(c)
    if not np.isfinite(c).all():
        raise ValueError(f"{what}: centroid {int(np.flatnonzero(~np.isfinite(c).all(axis=1))[0])} has a NaN or infinite component")
    if (c.view(np.uint32) & 0xFFFF).any():
        raise ValueError(f"{what}: the centroids hold float32 values that are not bf16 values (round them first)")
    cut = np.ascontiguousarray(np.asarray(cutoffs, dtype=np.float32).reshape(-1))
    w = np.ascontiguousarray(np.asarray(weights, dtype=np.float32).reshape(-1))
    if cut.shape[0] != (1 << nb) - 1:
        raise ValueError(f"{what}: {cut.shape[0]} cutoffs for nbits={nb} (need {(1 << nb) - 1})")
    if w.shape[0] != 1 << nb:
        raise ValueError(f"{what}: {w.shape[0]} weights for nbits={nb} (need {1 << nb})")
    if not np.isfinite(cut).all():
        raise ValueError(f"{what}: a cutoff is NaN or infinite")
    if not (np.diff(cut) > 0).all():
        raise ValueError(f"{what}: the cutoffs are not strictly ascending")
    if not np.isfinite(w).all():
        raise ValueError(f"{what}: a weight is NaN or infinite")
    return TokenCodec(c, nb, cut, w)


def bf16_to_f32(bits) -> np.ndarray:
    """float32 values of uint16 bf16 bit patterns (exact)."""
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def f32_to_bf16_rne(x) -> np.ndarray:
    """uint16 bf16 bit patterns of finite or infinite float32 values, rounded to nearest even (``v_cvt_pk_bf16_f32``)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def pack_buckets(buckets, nbits: int) -> np.ndarray:
    """Canonical packing: buckets uint8 ``[E, P]`` -> uint8 ``[E, P * nbits / 8]``; component ``j`` in bits
    ``[nbits * (j % (8 / nbits)), +nbits)`` of byte ``j * nbits / 8``."""
    b = np.asarray(buckets, dtype=np.uint8)
    per = 8 // nbits
    b = b.reshape(b.shape[0], b.shape[1] // per, per).astype(np.uint32)
    return (b << (nbits * np.arange(per, dtype=np.uint32))).sum(axis=2).astype(np.uint8)


def unpack_buckets(res, nbits: int) -> np.ndarray:
    """The inverse of ``pack_buckets``: uint8 ``[E, RB]`` -> buckets uint8 ``[E, RB * 8 / nbits]``."""
    r = np.asarray(res, dtype=np.uint8)
    per = 8 // nbits
    b = (r[:, :, None] >> (nbits * np.arange(per, dtype=np.uint8))) & ((1 << nbits) - 1)
    return b.reshape(r.shape[0], r.shape[1] * per).astype(np.uint8)


def token_codec_assign(codec: TokenCodec, tok, chunk: int = 8192) -> np.ndarray:
    """``code = argmax_c dot(d, centroid_c)``, ties to the lower ``c``, for bf16 tokens uint16 ``[E, P]``: uint16
    ``[E]``.  The dots are float32 sums in numpy's order -- the device's on inputs whose dots are exact, within the
    fp32 accumulation error of it otherwise."""
    tok = np.asarray(tok, dtype=np.uint16).reshape(-1, codec.P)
    ct = np.ascontiguousarray(codec.centroids.T)
    out = np.empty(tok.shape[0], dtype=np.uint16)
    for a in range(0, tok.shape[0], chunk):
        out[a:a + chunk] = (bf16_to_f32(tok[a:a + chunk]) @ ct).argmax(axis=1)
    return out


def token_codec_encode(codec: TokenCodec, tok, codes=None) -> Tuple[np.ndarray, np.ndarray]:
    """The numpy double of ``k_tok_encode``: ``(codes uint16 [E], res uint8 [E, P * nbits / 8])`` in the canonical
    layout.  Given ``codes`` (the device's, say) only the residual half runs: one float32 subtraction per component and
    ``bucket = #{i : cutoffs[i] < r}``."""
    tok = np.asarray(tok, dtype=np.uint16).reshape(-1, codec.P)
    codes = token_codec_assign(codec, tok) if codes is None else np.asarray(codes, dtype=np.uint16).reshape(-1)
    r = bf16_to_f32(tok) - codec.centroids[codes]
    buckets = np.searchsorted(codec.cutoffs, r.reshape(-1), side="left").reshape(r.shape).astype(np.uint8)
    return codes, pack_buckets(buckets, codec.nbits).reshape(tok.shape[0], codec.res_bytes)


def token_codec_decode(codec: TokenCodec, codes, res) -> np.ndarray:
    """The numpy double of ``k_tok_decode``: bf16 bits uint16 ``[E, P]`` of ``bf16_rne(centroid[code] + weights[bucket])``,
    one float32 addition and one rounding; no renormalisation."""
    codes = np.asarray(codes, dtype=np.uint16).reshape(-1)
    b = unpack_buckets(np.asarray(res, dtype=np.uint8).reshape(codes.shape[0], codec.res_bytes), codec.nbits)
    return f32_to_bf16_rne(codec.centroids[codes] + codec.weights[b]).reshape(codes.shape[0], codec.P)


def token_codes_as_csr(offsets, codes, res, codec: TokenCodec, what: str = "set_token_codes"):
    """Checked canonical codes ``(offsets int64 [n + 1], codes uint16 [E], res uint8 [E, RB])``; a code ``>= C``, wrong
    shapes and offsets that do not describe ``E`` tokens raise ``ValueError``."""
    off = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
    codes = np.ascontiguousarray(codes, dtype=np.uint16).reshape(-1)
    res = np.ascontiguousarray(res, dtype=np.uint8)
    if off.shape[0] < 1 or off[0] != 0 or (np.diff(off) < 0).any() or off[-1] != codes.shape[0]:
        raise ValueError(f"{what}: the offsets do not describe the {codes.shape[0]} codes")
    if res.size != codes.shape[0] * codec.res_bytes:
        raise ValueError(f"{what}: {res.size} bytes of buckets for {codes.shape[0]} tokens of {codec.res_bytes} bytes each")
    lens = np.diff(off)
    if lens.size and int(lens.max()) > MAX_ROW_TOKEN_VECTORS:
        raise ValueError(f"{what}: row {int(lens.argmax())} (of this call) has {int(lens.max())} tokens "
                         f"(at most {MAX_ROW_TOKEN_VECTORS})")
    bad = np.flatnonzero(codes >= codec.centroids.shape[0])
    if bad.size:
        row = int(np.searchsorted(off, bad[0], side="right")) - 1
        raise ValueError(f"{what}: token {int(bad[0] - off[row])} of row {row} (of this call) has code {int(codes[bad[0]])}, "
                         f"the codec has {codec.centroids.shape[0]} centroids")
    return off, codes, res.reshape(codes.shape[0], codec.res_bytes)


def residual_quantiles(r, nbits: int) -> Tuple[np.ndarray, np.ndarray]:
    """ColBERTv2's bucket boundaries and values from residual components ``r``: ``cutoffs[i - 1]`` is the ``i / 2^nbits``
    quantile (``i = 1 .. 2^nbits - 1``), ``weights[i]`` the ``(i + 1/2) / 2^nbits`` quantile, float32.  Equal
    neighbouring cutoffs (a sample without spread) are moved apart by one float32 step so that they ascend."""
    nb = 1 << nbits
    r = np.sort(np.asarray(r, dtype=np.float32).reshape(-1)).astype(np.float64)
    cut = np.quantile(r, np.arange(1, nb) / nb).astype(np.float32)
    w = np.quantile(r, (np.arange(nb) + 0.5) / nb).astype(np.float32)
    for i in range(1, cut.shape[0]):
        if not cut[i] > cut[i - 1]:
            cut[i] = np.nextafter(cut[i - 1], np.float32(np.inf))
    return cut, w


def train_token_codec(mats, ncentroids: int, nbits: int = 2, niter: int = 20, seed: int = 0, device: int = 0,
                      max_points_per_centroid: int = 256) -> TokenCodec:
    """A codec trained on token matrices (any form ``set_tokens`` takes): a seeded sample of at most
    ``max_points_per_centroid * ncentroids`` tokens goes as float32 rows into a temporary ``IndexFlat(P)``,
    ``kmeans(ncentroids)`` runs on the GPU (``2 <= ncentroids <= 4096``, spherical), the centroids are rounded to bf16,
    the sample is encoded on the device, and ``cutoffs`` / ``weights`` are the quantiles of the sample's residual
    components (``residual_quantiles``).  The same call gives the same bytes."""
    if int(nbits) not in TOKEN_CODEC_BITS:
        raise ValueError(f"train_token_codec: nbits={nbits!r} is none of 1, 2, 4")
    nc = int(ncentroids)
    if not 2 <= nc <= 4096:
        raise ValueError(f"train_token_codec: ncentroids={nc} outside [2, 4096]")
    _, tok, P = tokens_as_csr(mats, what="train_token_codec")
    if tok.shape[0] < nc:
        raise ValueError(f"train_token_codec: {tok.shape[0]} tokens for {nc} centroids")
    cap = max(int(max_points_per_centroid), 1) * nc
    if tok.shape[0] > cap:
        tok = tok[np.sort(np.random.default_rng(seed).choice(tok.shape[0], cap, replace=False))]
    ix = IndexFlat(P, METRIC_INNER_PRODUCT, device)
    try:
        ix.add(bf16_to_f32(tok))
        cent = bf16_to_f32(f32_to_bf16_rne(ix.kmeans(nc, niter=niter, seed=seed).centroids))
        # the sample's codes from the device's encoder (buckets of a placeholder codec are not looked at)
        ix.set_token_codec(TokenCodec(cent, 1, np.zeros(1, np.float32), np.zeros(2, np.float32)))
        ix.set_tokens((np.arange(tok.shape[0] + 1, dtype=np.int64), tok, P))
        _, codes, _ = ix.get_token_codes()
    finally:
        ix.close()
    cut, w = residual_quantiles(bf16_to_f32(tok) - cent[codes], int(nbits))
    return token_codec_args(cent, int(nbits), cut, w, what="train_token_codec")


def prune_args(k, ncand, what: str = "search_maxsim_pruned") -> Tuple[Optional[int], int]:
    """The argument rules of ``maxsim_candidates`` (``k`` is ``None``) and ``search_maxsim_pruned``: ``(k, ncand)`` as
    ints; ``1 <= ncand <= 65536``, ``1 <= k <= 128`` and ``k <= ncand``, else ``ValueError``."""
    try:
        nc = int(ncand)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: ncand={ncand!r} is no integer") from None
    if nc != ncand or not 1 <= nc <= MAX_MAXSIM_ROWS:
        raise ValueError(f"{what}: ncand={ncand!r} outside [1, {MAX_MAXSIM_ROWS}]")
    if k is None:
        return None, nc
    k = int(k)
    if k < 1 or k > MAX_HYBRID_K:
        raise ValueError(f"{what}: k={k} outside [1, {MAX_HYBRID_K}]")
    if k > nc:
        raise ValueError(f"{what}: k={k} exceeds ncand={nc}")
    return k, nc


def _sum_ascending_f32(mx: np.ndarray) -> np.ndarray:
    """float32 ``[n]``: the columns of ``mx [n, mq]`` added one after the other, the device's chain."""
    acc = np.zeros(mx.shape[0], dtype=np.float32)
    for s in range(mx.shape[1]):
        acc = acc + mx[:, s]
    return acc


def token_centroid_scores(codec: TokenCodec, q) -> np.ndarray:
    """The numpy double of ``k_tok_ctable``: ``S[c, s] = dot(q_s, centroid_c)``, float32 ``[C, mq]``, for ONE query matrix
    of bf16 bits.  float32 sums in numpy's order -- the device's bits where the dots are exact, within the fp32
    accumulation error of them otherwise."""
    q = np.asarray(q, dtype=np.uint16).reshape(-1, codec.P)
    return np.ascontiguousarray(codec.centroids @ bf16_to_f32(q).T, dtype=np.float32)


def token_codec_approx(codec: TokenCodec, offsets, codes, q, S=None) -> np.ndarray:
    """The numpy double of ``k_tok_ci``: ``A[r] = sum over s ascending (float32) of max over the row's tokens of
    S[code_t, s]``, float32 ``[n]``, ``-inf`` for a row without tokens.  ``S``: a table to use in place of
    ``token_centroid_scores(codec, q)``."""
    off = np.asarray(offsets, dtype=np.int64).reshape(-1)
    codes = np.asarray(codes, dtype=np.uint16).reshape(-1)
    S = token_centroid_scores(codec, q) if S is None else np.asarray(S, dtype=np.float32)
    out = np.full(off.shape[0] - 1, -np.inf, dtype=np.float32)
    live = np.flatnonzero(np.diff(off) > 0)
    if live.size:
        out[live] = _sum_ascending_f32(np.maximum.reduceat(S[codes], off[:-1][live], axis=0))
    return out


def maxsim_candidates_numpy(approx, ncand: int, allowed=None, id_base: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """Step 3 from an approximate column: the first ``ncand`` rows of ``lexsort((id, -A))`` among the allowed rows that
    are no miss, returned in ASCENDING id order: ``(ids int64, approx float32)``."""
    _, ncand = prune_args(None, ncand, "maxsim_candidates")
    a = np.asarray(approx, dtype=np.float32).reshape(-1)
    ok = a > -np.inf
    if allowed is not None:
        ok = ok & np.asarray(allowed, dtype=bool).reshape(-1)
    rows = np.flatnonzero(ok)
    take = np.sort(rows[np.lexsort((rows, -(a[rows] + np.float32(0.0))))][:ncand])
    return take.astype(np.int64) + int(id_base), a[take]


def token_codec_scores(codec: TokenCodec, offsets, codes, res, q, rows=None) -> np.ndarray:
    """The exact MaxSim on the codes in float32 (decode, dots, maximum, ascending sum) of ``rows`` (default: every row):
    ``-inf`` for a row without tokens.  The device's bits where the dots are exact."""
    off = np.asarray(offsets, dtype=np.int64).reshape(-1)
    rows = np.arange(off.shape[0] - 1) if rows is None else np.asarray(rows, dtype=np.int64).reshape(-1)
    codes = np.asarray(codes, dtype=np.uint16).reshape(-1)
    res = np.asarray(res, dtype=np.uint8).reshape(codes.shape[0], codec.res_bytes)
    q32 = bf16_to_f32(np.asarray(q, dtype=np.uint16).reshape(-1, codec.P))
    lens = off[rows + 1] - off[rows]
    out = np.full(rows.shape[0], -np.inf, dtype=np.float32)
    live = np.flatnonzero(lens > 0)
    if live.size:
        idx = np.concatenate([np.arange(off[r], off[r + 1]) for r in rows[live]])
        starts = np.concatenate([[0], np.cumsum(lens[live])[:-1]])
        sim = bf16_to_f32(token_codec_decode(codec, codes[idx], res[idx])) @ q32.T      # [E', mq]
        out[live] = _sum_ascending_f32(np.maximum.reduceat(sim.astype(np.float32), starts, axis=0))
    return out


def search_maxsim_pruned_numpy(codec: TokenCodec, offsets, codes, res, q, k: int, ncand: int, allowed=None,
                               id_base: int = 0, approx=None) -> Tuple[np.ndarray, np.ndarray]:
    """The numpy double of ``search_maxsim_pruned`` (steps 2 to 4): ``(D float32 [1, k], I int64 [1, k])``.  ``approx``:
    an approximate column to use in place of ``token_codec_approx`` (the device's, say)."""
    k, ncand = prune_args(k, ncand)
    a = token_codec_approx(codec, offsets, codes, q) if approx is None else approx
    ids, _ = maxsim_candidates_numpy(a, ncand, allowed)
    sc = token_codec_scores(codec, offsets, codes, res, q, rows=ids)
    order = np.lexsort((ids, -sc))[:k]
    D, I = np.full((1, k), -np.finfo(np.float32).max, np.float32), np.full((1, k), -1, np.int64)
    D[0, :order.size], I[0, :order.size] = sc[order], ids[order] + int(id_base)
    return D, I


def token_scores(offsets, tok, q, rows=None) -> np.ndarray:
    """The MaxSim of ONE query matrix with the RAW matrices of ``rows`` (default: every row) in float32 (dots, maximum,
    ascending sum), ``-inf`` for a row without tokens: ``token_codec_scores`` for a store without a codec.  The device's
    bits where the dots are exact."""
    off = np.asarray(offsets, dtype=np.int64).reshape(-1)
    rows = np.arange(off.shape[0] - 1) if rows is None else np.asarray(rows, dtype=np.int64).reshape(-1)
    q32 = bf16_to_f32(np.asarray(q, dtype=np.uint16))
    tok = np.asarray(tok, dtype=np.uint16).reshape(-1, q32.shape[1])
    lens = off[rows + 1] - off[rows]
    out = np.full(rows.shape[0], -np.inf, dtype=np.float32)
    live = np.flatnonzero(lens > 0)
    if live.size:
        idx = np.concatenate([np.arange(off[r], off[r + 1]) for r in rows[live]])
        starts = np.concatenate([[0], np.cumsum(lens[live])[:-1]])
        sim = bf16_to_f32(tok[idx]) @ q32.T                                             # [E', mq]
        out[live] = _sum_ascending_f32(np.maximum.reduceat(sim.astype(np.float32), starts, axis=0))
    return out


def maxsim_lists_numpy(offsets, q_mats, ids, tok=None, codec: Optional[TokenCodec] = None, codes=None, res=None,
                       id_base: int = 0) -> np.ndarray:
    """The numpy double of ``maxsim_ids_batch``: float32 ``[nq, f]``, entry ``(b, j)`` the MaxSim of ``q_mats[b]`` with row
    ``ids[b, j] - id_base`` of the store -- raw (``tok``) through ``token_scores``, compressed (``codec, codes, res``)
    through ``token_codec_scores`` -- and ``-inf`` for an id that names no row with a matrix."""
    off = np.asarray(offsets, dtype=np.int64).reshape(-1)
    ids = np.asarray(ids, dtype=np.int64)
    T = off.shape[0] - 1
    out = np.full(ids.shape, -np.inf, dtype=np.float32)
    for b, q in enumerate(q_mats):
        r = ids[b] - int(id_base)
        ok = np.flatnonzero((r >= 0) & (r < T))
        if ok.size:
            out[b, ok] = (token_scores(off, tok, q, r[ok]) if codec is None
                          else token_codec_scores(codec, off, codes, res, q, r[ok]))
    return out


def search_rerank_maxsim_numpy(S0, I0, late, k: int, floor=None):
    """The numpy double of the ranking of ``search_rerank_maxsim``: from the pool ``(S0, I0) [nq, fetch]`` of the dense
    search and the MaxSim ``late [nq, fetch]`` of its entries, ``(D, I, S, R)``, each ``[nq, k]``: the entries with ``S0 <
    floor``, the ``-1`` padding and the ``-inf`` scores dropped, then the first ``k`` of a STABLE descending sort by the
    late score (ties keep the pool's order); padded with ``D = S = -FLT_MAX``, ``I = R = -1``."""
    S0, I0 = np.asarray(S0, dtype=np.float32), np.asarray(I0, dtype=np.int64)
    late = np.asarray(late, dtype=np.float32)
    nq, k = S0.shape[0], int(k)
    fmax = np.finfo(np.float32).max
    D, S = np.full((nq, k), -fmax, np.float32), np.full((nq, k), -fmax, np.float32)
    I, R = np.full((nq, k), -1, np.int64), np.full((nq, k), -1, np.int32)
    for b in range(nq):
        ok = (I0[b] >= 0) & (late[b] > -np.inf)
        if floor is not None and floor == floor:
            ok &= ~(S0[b] < np.float32(floor))
        pos = np.flatnonzero(ok)
        pos = pos[np.argsort(-(late[b, pos] + np.float32(0.0)), kind="stable")][:k]
        D[b, :pos.size], I[b, :pos.size], S[b, :pos.size], R[b, :pos.size] = late[b, pos], I0[b, pos], S0[b, pos], pos
    return D, I, S, R


MAX_DIVERSE_FETCH = nat.MAX_DIVERSE_FETCH


def diverse_args(k, fetch, lam) -> Tuple[int, int, float]:
    """The argument rules of ``search_diverse`` (``css_index_search_diverse``): ``(k, fetch, lam)`` with the automatic
    pool size resolved -- ``fetch = 0`` means 32 if ``4k <= 32``, otherwise 128.  ``lam`` outside ``[0, 1]`` (or NaN),
    ``fetch`` outside ``[0, 128]`` and ``k`` outside ``[1, fetch]`` raise ``ValueError``."""
    k, fetch, lam = int(k), int(fetch), float(lam)
    if not (0.0 <= lam <= 1.0):   # (a NaN fails both comparisons)
        raise ValueError(f"lam={lam} outside [0, 1]")
    if fetch < 0 or fetch > MAX_DIVERSE_FETCH:
        raise ValueError(f"fetch={fetch} outside [0, {MAX_DIVERSE_FETCH}] (0: automatic)")
    if fetch == 0:
        fetch = 32 if 4 * k <= 32 else MAX_DIVERSE_FETCH
    if k < 1 or k > fetch:
        raise ValueError(f"k={k} outside [1, fetch={fetch}]")
    return k, fetch, lam


def mmr_select(S, I, X, k: int, lam: float, metric: int) -> Tuple[np.ndarray, np.ndarray]:
    """The selection rule of ``search_diverse`` (the library's ``k_mmr_select``), stated in numpy.  ``S, I`` are
    ``[nq, m]`` best-first lists (scores, ids; pads ``I = -1`` at the tail) and ``X`` is ``[nq, m, d]``, the candidates'
    stored rows (rows of pads are not looked at).  Everything is float32.  Relevance is ``S`` for the inner product and
    ``-S`` for L2; ``sim(a, b)`` is ``<x_a, x_b>`` resp. ``-sum((x_a - x_b)^2)``.  Pick 0 is candidate 0; pick ``t`` is the
    unpicked valid candidate with the largest ``lam * rel - (1 - lam) * max_{u < t} sim(c, p_u)``, ties to the smaller
    list position.  Returns ``(D[nq, k], I[nq, k])`` in PICK order: the picks' own scores and ids, padded like
    ``search``.  (The sharded index selects with this after the exchange of the pool's rows.)"""
    S, I, X = np.asarray(S, np.float32), np.asarray(I, np.int64), np.asarray(X, np.float32)
    nq, m = I.shape
    k, lam = int(k), np.float32(lam)
    oml = np.float32(1.0) - lam
    Do = np.full((nq, k), -np.finfo(np.float32).max if metric == METRIC_INNER_PRODUCT else np.finfo(np.float32).max,
                 dtype=np.float32)
    Io = np.full((nq, k), -1, dtype=np.int64)
    for j in range(nq):
        valid = I[j] >= 0
        npick = min(k, int(valid.sum()))
        if npick == 0 or not valid[0]:
            continue
        rel = S[j] if metric == METRIC_INNER_PRODUCT else -S[j]
        pen = np.full(m, -np.inf if lam != 1 else 0.0, dtype=np.float32)   # (lam == 1: the term is 0 whatever the rows hold)
        free = valid.copy()
        last = 0
        for t in range(npick):
            if t:
                if lam != 1:
                    if metric == METRIC_INNER_PRODUCT:
                        sim = (X[j] * X[j, last][None, :]).sum(axis=1, dtype=np.float32)
                    else:
                        diff = X[j] - X[j, last][None, :]
                        sim = -(diff * diff).sum(axis=1, dtype=np.float32)
                    pen = np.where(free, np.maximum(pen, sim), pen)
                v = np.where(free, lam * rel - oml * pen, -np.inf).astype(np.float32)
                v[np.isnan(v)] = -np.inf
                cand = np.flatnonzero(free)
                last = int(cand[np.argmax(v[cand])])        # (argmax returns the first maximum: the smaller position)
            free[last] = False
            Do[j, t], Io[j, t] = S[j, last], I[j, last]
    return Do, Io


MAX_EXAMPLES = nat.MAX_EXAMPLES
MAX_EXAMPLES_K = nat.MAX_EXAMPLES_K


def fuse_example_scores(Spos, Sneg, gamma, metric: int) -> Tuple[np.ndarray, np.ndarray]:
    """The fusion rule of ``search_examples`` (the library's ``k_scan_examples``), stated in numpy.  ``Spos`` is
    ``[npos, n]`` and ``Sneg`` ``[nneg, n]`` (``nneg`` may be 0): the float32 scores of ``n`` rows against the positive
    and the negative examples -- inner products, or squared L2 distances.  Returns ``(F[n], P[n])`` in float32 with
    ``P = max(Spos)`` and ``N = max(Sneg)`` over the examples (L2: ``min``), and ``F = P`` without negatives, otherwise
    ``F = fma(-gamma, N, P)`` with ``np.float32`` fma semantics: the product ``gamma * N`` is NOT rounded before the
    subtraction, so the float64 expression ``P - gamma * N`` (exact for float32 operands up to its own rounding) is
    rounded ONCE to float32.  Larger ``F`` is better for the inner product, smaller for L2.  (The sharded index and
    the CPU doubles of the tests fuse with this.)"""
    Spos = np.asarray(Spos, np.float32)
    Sneg = np.asarray(Sneg, np.float32)
    if Spos.ndim != 2 or Spos.shape[0] < 1:
        raise ValueError(f"fuse_example_scores: Spos must be [npos >= 1, n], got shape {Spos.shape}")
    ext = np.max if metric == METRIC_INNER_PRODUCT else np.min
    P = ext(Spos, axis=0).astype(np.float32)
    if Sneg.size == 0 and (Sneg.ndim < 2 or Sneg.shape[0] == 0):
        return P.copy(), P
    if Sneg.ndim != 2 or Sneg.shape[1] != Spos.shape[1]:
        raise ValueError(f"fuse_example_scores: Sneg must be [nneg, {Spos.shape[1]}], got shape {Sneg.shape}")
    N = ext(Sneg, axis=0).astype(np.float32)
    # a float32 product is exact in float64, and the sum of it and a float32 is rounded once more there: double
    # rounding differs from the fma only on ties of the 53-bit sum, which float32 operands of these sizes do not reach
    F = (P.astype(np.float64) - np.float64(np.float32(gamma)) * N.astype(np.float64)).astype(np.float32)
    return F, P


def example_vectors(v, d: int, what: str = "search_examples") -> np.ndarray:
    """Example vectors of ``search_examples`` -> contiguous ``[n, d]`` float32; ``None`` and anything empty are no examples."""
    if v is None or np.size(v) == 0:
        return np.zeros((0, d), dtype=np.float32)
    return _as_f32_2d(v, d, what)


def example_args(k, gamma, npos: int, m: int, what: str = "search_examples") -> Tuple[int, float]:
    """The argument rules of ``search_examples`` (``css_index_search_examples``): ``1 <= k <= 128``, ``gamma`` finite
    and ``>= 0``, at least one positive, at most 16 examples; anything else raises ``ValueError``."""
    k, gamma = int(k), float(gamma)
    if k < 1 or k > MAX_EXAMPLES_K:
        raise ValueError(f"{what}: k={k} outside [1, {MAX_EXAMPLES_K}]")
    if not np.isfinite(gamma) or gamma < 0.0:
        raise ValueError(f"{what}: gamma={gamma} must be finite and >= 0")
    if npos < 1:
        raise ValueError(f"{what}: no positive example")
    if m > MAX_EXAMPLES:
        raise ValueError(f"{what}: {m} examples, at most {MAX_EXAMPLES}")
    return k, gamma

MAX_CENTROIDS = nat.MAX_CENTROIDS


class KmeansStep(NamedTuple):
    """What one Lloyd step returns (``css_index_kmeans_step``): the fixed-point sums ``[nc, d]`` and member counts
    ``[nc]`` (int64), the integer objective, the two shifts ``s`` and ``t``, and -- where asked for -- the assignment
    (int32, ``-1`` = row not allowed) and squared distance (float32) of every row."""
    sums: np.ndarray
    counts: np.ndarray
    obj: int
    fx_shift: int
    obj_shift: int
    assign: Optional[np.ndarray] = None
    dist: Optional[np.ndarray] = None


class KmeansResult(NamedTuple):
    """What ``run_kmeans`` returns: the centroids ``[nc, d]`` float32, the final assignment and squared distance of
    every row (``-1`` / ``0`` for rows not allowed), the cluster sizes, the objective ``obj_int * 2^-t`` of every
    iteration, the number of iterations run, and per iteration the ``(empty, donor)`` pairs that were split."""
    centroids: np.ndarray
    assign: np.ndarray
    dist: np.ndarray
    sizes: np.ndarray
    obj: List[float]
    iterations: int
    splits: tuple = ()


def kmeans_shift(max_norm2: float, n: int) -> Tuple[int, int, int]:
    """The shift rule of ``css_index_kmeans_step``, restated: ``(s, e, t)``.  ``ex`` is the exponent ``frexp`` gives the
    largest squared row norm (0 when that is 0), ``e = ceil(ex / 2)`` so that every ``|x| < 2^e``, ``b`` the bit length
    of ``max(n, 1) - 1``, ``s = 62 - b - e`` the shift of the sums and ``t = s - e - 2`` that of the objective:
    ``n * 2^(s + e) <= 2^62``, so no int64 sum can reach ``2^63``."""
    m = float(np.float32(max_norm2))
    ex = math.frexp(m)[1] if m > 0.0 else 0
    e = -((-ex) // 2)
    b = (max(int(n), 1) - 1).bit_length()
    s = 62 - b - e
    return s, e, s - e - 2


def _fixed(x, shift: int) -> np.ndarray:
    """``llrint(x * 2^shift)`` of float32 values as int64: exact scaling in float64, round to nearest even."""
    return np.rint(np.ldexp(np.asarray(x, dtype=np.float32).astype(np.float64), int(shift))).astype(np.int64)


def fixed_point_sums(X, assign, nc: int, s: int) -> Tuple[np.ndarray, np.ndarray]:
    """The sums of ``css_index_kmeans_step`` stated in numpy: ``sums[c] = sum over assign == c of llrint(X * 2^s)``
    (int64 ``[nc, d]``) and the member counts (int64 ``[nc]``); rows with ``assign < 0`` count nowhere."""
    X = np.asarray(X, dtype=np.float32)
    a = np.asarray(assign).astype(np.int64).reshape(-1)
    nc = int(nc)
    sums = np.zeros((nc, X.shape[1] if X.ndim == 2 else 0), dtype=np.int64)
    live = np.flatnonzero(a >= 0)
    counts = np.bincount(a[live], minlength=nc).astype(np.int64)
    if live.size:
        order = live[np.argsort(a[live], kind="stable")]
        q = _fixed(X[order], s)
        starts = np.concatenate(([0], np.cumsum(counts)[:-1]))
        full = counts > 0
        sums[full] = np.add.reduceat(q, starts[full], axis=0)
    return sums, counts


def fixed_point_objective(dist, assign, t: int) -> int:
    """The integer objective of ``css_index_kmeans_step``: ``sum of llrint(dist * 2^t)`` over the assigned rows."""
    a = np.asarray(assign).reshape(-1)
    return int(_fixed(np.asarray(dist, dtype=np.float32).reshape(-1)[a >= 0], t).sum(dtype=np.int64))


def lloyd_update(sums, counts, s: int, prev, spherical: bool = False) -> Tuple[np.ndarray, List[Tuple[int, int]]]:
    """The centroid update of ``run_kmeans``: ``(centroids float32 [nc, d], [(empty, donor), ...])``.  ``sums`` goes to
    float64, times ``2^-s``, divided by the count, and is rounded to float32 ONCE; ``spherical`` divides by the float64
    norm in front of that rounding (a zero vector stays zero).  An empty cluster is refilled faiss' way, made
    deterministic: empties in ascending order, the donor is the largest cluster (ties to the lowest index), the empty
    one takes ``donor * (1 + 1/1024)``, the donor becomes ``donor * (1 - 1/1024)`` (float32 products), and the donor's
    count is halved between the two.  With no member anywhere the previous centroids are kept."""
    sums = np.asarray(sums, dtype=np.int64)
    cw = np.asarray(counts, dtype=np.int64).copy()
    out = np.array(prev, dtype=np.float32, copy=True).reshape(sums.shape)
    full = cw > 0
    mean = np.ldexp(sums[full].astype(np.float64), -int(s)) / cw[full].astype(np.float64)[:, None]
    if spherical:
        nrm = np.sqrt((mean * mean).sum(axis=1))
        mean[nrm > 0] /= nrm[nrm > 0][:, None]
    out[full] = mean.astype(np.float32)
    split: List[Tuple[int, int]] = []
    up, down = np.float32(1.0 + 1.0 / 1024.0), np.float32(1.0 - 1.0 / 1024.0)
    for c in np.flatnonzero(~full):
        donor = int(np.argmax(cw))   # (the first maximum: the lowest index)
        if cw[donor] <= 0:
            break
        out[c] = out[donor] * up
        out[donor] = out[donor] * down
        cw[c] = cw[donor] // 2
        cw[donor] -= cw[c]
        split.append((int(c), donor))
    return out, split


def kmeans_init_ids(allowed_rows, nc: int, seed: int) -> np.ndarray:
    """The rows the initial centroids are copied from: ``nc`` of ``allowed_rows`` without replacement, by
    ``np.random.default_rng(seed)``.  Fewer than ``nc`` allowed rows raise ``ValueError``."""
    rows = np.asarray(allowed_rows, dtype=np.int64).reshape(-1)
    if rows.shape[0] < int(nc):
        raise ValueError(f"kmeans: {rows.shape[0]} allowed rows for {int(nc)} centroids")
    return np.ascontiguousarray(np.random.default_rng(seed).choice(rows, int(nc), replace=False), dtype=np.int64)


def run_kmeans(step: Callable, gather_rows: Callable, nc: int, niter: int = 20, seed: int = 0, init=None,
               spherical: bool = False, init_rows=None, train_allow=None, allow=None) -> KmeansResult:
    """THE Lloyd loop (the single index, the sharded index and the CPU doubles of the tests all run this one).
    ``step(centroids, allow, want)`` is one step over the rows -- it returns a ``KmeansStep``, with ``assign`` and
    ``dist`` when ``want`` -- and ``gather_rows(ids)`` returns stored rows by id.  Initial centroids are ``init``
    (``[nc, d]``) or the rows ``kmeans_init_ids(init_rows, nc, seed)``.  Then up to ``niter`` times: a step under
    ``train_allow``, ``lloyd_update``; the loop stops early when the new centroids are bit-equal to the old ones (the
    arithmetic is deterministic, so that is a fixpoint).  A final step under ``allow`` assigns every allowed row."""
    nc = int(nc)
    if nc < 2 or nc > MAX_CENTROIDS:
        raise ValueError(f"kmeans: nc={nc} outside [2, {MAX_CENTROIDS}]")
    if init is not None:
        cent = np.array(init, dtype=np.float32, copy=True)
        if cent.ndim != 2 or cent.shape[0] != nc:
            raise ValueError(f"kmeans: init must be [{nc}, d], got shape {cent.shape}")
    else:
        cent = np.array(gather_rows(kmeans_init_ids(init_rows, nc, seed)), dtype=np.float32, copy=True)
    obj: List[float] = []
    splits = []
    iterations = 0
    for _ in range(int(niter)):
        st = step(cent, train_allow, False)
        obj.append(math.ldexp(float(st.obj), -st.obj_shift))
        new, split = lloyd_update(st.sums, st.counts, st.fx_shift, cent, spherical)
        splits.append(tuple(split))
        iterations += 1
        same = new.tobytes() == cent.tobytes()
        cent = new
        if same:
            break
    last = step(cent, allow, True)
    return KmeansResult(cent, last.assign, last.dist, np.asarray(last.counts, dtype=np.int64), obj, iterations, tuple(splits))


def kmeans_train_mask(allowed_rows: np.ndarray, ntotal: int, nc: int, max_points_per_centroid: int, seed: int):
    """The training subset of ``kmeans(max_points_per_centroid=...)`` as a boolean mask over ``ntotal`` rows: a seeded
    random ``nc * max_points_per_centroid`` of the allowed rows; ``None`` when no cut applies."""
    cap = int(nc) * int(max_points_per_centroid)
    if max_points_per_centroid <= 0 or allowed_rows.shape[0] <= cap:
        return None
    mask = np.zeros(int(ntotal), dtype=np.bool_)
    mask[np.random.default_rng([int(seed), 1]).choice(allowed_rows, cap, replace=False)] = True
    return mask


MAX_TRANSFORM_ROWS = nat.MAX_TRANSFORM_ROWS


class GramResult(NamedTuple):
    """What ``css_index_gram`` returns: ``gram[i, j] = sum_r q_r[i] q_r[j]`` (int64 ``[d, d]``, symmetric) and
    ``colsum[j] = sum_r q_r[j]`` (int64 ``[d]``) over the allowed rows with ``q = llrint(x * 2^shift)``, the number of
    allowed rows, and the shift ``p``."""
    gram: np.ndarray
    colsum: np.ndarray
    count: int
    shift: int


class PcaResult(NamedTuple):
    """What ``pca_from_gram`` returns: the mean ``[d]`` float32, the components ``[m, d]`` float32 (rows; scaled by
    ``1 / sqrt(eigenvalue)`` under ``whiten``), their eigenvalues (float64, descending, clipped at 0), the trace of the
    covariance, the number of rows and the shift of the integers it was formed from."""
    mean: np.ndarray
    components: np.ndarray
    eigenvalues: np.ndarray
    total_variance: float
    count: int
    shift: int


def pca_shift(max_norm2: float, n: int) -> Tuple[int, int]:
    """The shift rule of ``css_index_gram``, restated: ``(p, e)``.  ``ex``, ``e`` and ``b`` are those of ``kmeans_shift``
    (``|x| < 2^e`` for every entry, ``b`` the bit length of ``max(n, 1) - 1``); ``p = min(20, (62 - b) >> 1) - e``.  So
    ``|q| <= 2^(p + e) <= 2^20``, a product is at most ``2^40`` -- 8192 of them sum exactly in float64 -- and
    ``n * 2^(2 (p + e)) <= 2^62``: no int64 sum can reach ``2^63``."""
    m = float(np.float32(max_norm2))
    ex = math.frexp(m)[1] if m > 0.0 else 0
    e = -((-ex) // 2)
    b = (max(int(n), 1) - 1).bit_length()
    return min(20, (62 - b) >> 1) - e, e


def fixed_point_gram(X, allow, p: int) -> Tuple[np.ndarray, np.ndarray, int]:
    """``css_index_gram`` stated in numpy: ``(gram int64 [d, d], colsum int64 [d], count)`` of the allowed rows of ``X``
    (``allow`` a boolean mask or ``None``) under ``q = llrint(X * 2^p)``.  Exact int64 (which wraps silently: the
    caller keeps to ``pca_shift``).  Not by the kernel's argument: ``q`` is split into ``hi * 2^13 + lo`` with
    ``0 <= lo < 2^13``, so for ``|q| < 2^26`` the limb products stay below ``2^26`` and their sums over 4096 rows below
    ``2^38`` -- far inside what float64 holds exactly -- and three BLAS products per chunk give the integers; longer
    ``q`` go through numpy's (slow) integer matmul."""
    X = np.asarray(X, dtype=np.float32)
    X = X.reshape(-1, X.shape[-1] if X.ndim else 0)
    if allow is not None:
        X = X[np.asarray(allow, dtype=bool)]
    d = X.shape[1]
    gram, colsum = np.zeros((d, d), dtype=np.int64), np.zeros(d, dtype=np.int64)
    for at in range(0, X.shape[0], 4096):
        q = _fixed(X[at:at + 4096], p)
        colsum += q.sum(axis=0, dtype=np.int64)
        if int(np.abs(q).max()) >= 1 << 26:
            gram += q.T @ q
            continue
        hi = q >> 13                                             # (floor: lo is never negative)
        H, L = hi.astype(np.float64), (q - (hi << 13)).astype(np.float64)
        HL = H.T @ L
        gram += ((H.T @ H).astype(np.int64) << 26) + ((HL + HL.T).astype(np.int64) << 13) + (L.T @ L).astype(np.int64)
    return gram, colsum, int(X.shape[0])


def pca_from_gram(gram, colsum, count: int, p: int, n_components: int, whiten: bool = False) -> PcaResult:
    """Mean, principal components and eigenvalues from the integers of ``css_index_gram`` (the single index, the
    sharded index and the CPU doubles all run this one, so the same integers give the same bytes).  In float64: the
    BIASED covariance ``C = (G - outer(s, s) / count) / count * 2^(-2p)``, ``numpy.linalg.eigh``, eigenvalues descending
    and clipped at 0, each component's sign chosen so that its entry of largest magnitude is positive (ties to the
    lowest index); ``whiten`` scales component ``i`` by ``1 / sqrt(max(eigenvalue_i, tiny))`` (``tiny`` the smallest normal float32, so
    the result stays finite in float32); ONE rounding to float32.
    ``count == 0`` raises ``ValueError``."""
    G = np.asarray(gram, dtype=np.int64)
    s = np.asarray(colsum, dtype=np.int64).astype(np.float64)
    d = G.shape[0]
    m, count = int(n_components), int(count)
    if count <= 0:
        raise ValueError("pca: no rows")
    if m < 1 or m > d:
        raise ValueError(f"pca: n_components={m} outside [1, {d}]")
    C = np.ldexp((G.astype(np.float64) - np.outer(s, s) / count) / count, -2 * int(p))
    w, V = np.linalg.eigh(C)
    order = np.argsort(-w, kind="stable")[:m]
    w, V = np.maximum(w[order], 0.0), V[:, order].T.copy()
    lead = np.abs(V).argmax(axis=1)                      # (the first maximum: the lowest index)
    V[V[np.arange(m), lead] < 0] *= -1.0
    if whiten:
        V /= np.sqrt(np.maximum(w, np.finfo(np.float32).tiny))[:, None]
    mean = np.ldexp(s / count, -int(p))
    return PcaResult(mean.astype(np.float32), np.ascontiguousarray(V, dtype=np.float32), w, float(np.trace(C)), count, int(p))


def pca_offset(components, mean) -> np.ndarray:
    """``b = -A mean`` of the transform ``y = A x + b`` that centres the rows: formed in float64, ONE rounding to float32."""
    return (-(np.asarray(components, dtype=np.float32).astype(np.float64) @ np.asarray(mean, dtype=np.float32).astype(np.float64))).astype(np.float32)


def transform_args(A, b, d: int, what: str = "transform") -> Tuple[np.ndarray, Optional[np.ndarray]]:
    """``A`` as float32 ``[m, d]`` with ``1 <= m <= 256`` and ``b`` as float32 ``[m]`` (or ``None``), or ``ValueError``."""
    A = _as_f32_2d(A, d, what)
    m = A.shape[0]
    if m < 1 or m > MAX_TRANSFORM_ROWS:
        raise ValueError(f"{what}: m={m} outside [1, {MAX_TRANSFORM_ROWS}]")
    if b is not None:
        b = np.ascontiguousarray(b, dtype=np.float32).reshape(-1)
        if b.shape[0] != m:
            raise ValueError(f"{what}: b must have {m} entries, got {b.shape[0]}")
    return A, b


class IndexFlat:
    """Exact brute-force index in HBM (``faiss.IndexFlat`` semantics)."""

    def __init__(self, d: int, metric: int = METRIC_INNER_PRODUCT, device: int = 0):
        self.d = int(d)
        self.metric_type = int(metric)
        self.device = int(device)
        self.is_trained = True
        h = ctypes.c_void_p()
        nat.check(nat.lib().css_index_create(self.d, self.metric_type, self.device, ctypes.byref(h)))
        self._h: Optional[ctypes.c_void_p] = h
        self._terms_rows = 0   # the leading rows that have term lists (set_terms appends there by default)

    # -- lifetime ---------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_h", None) is not None:
            nat.lib().css_index_free(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover - interpreter shutdown order
        try:
            self.close()
        except Exception:
            pass

    def _handle(self):
        if self._h is None:
            raise RuntimeError("index has been freed")
        return self._h

    def _read_i64(self, fn) -> int:
        n = ctypes.c_int64(0)
        nat.check(fn(self._handle(), ctypes.byref(n)))
        return int(n.value)

    def _allow_bits(self, allow):
        """``allow`` packed against ``ntotal``: ``(bitmap, its address)``, ``(None, None)`` without a mask.  The
        address is good while the bitmap is referenced."""
        if allow is None:
            return None, None
        bits = pack_allow_bits(allow, self.ntotal)
        return bits, bits.ctypes.data

    def _topk(self, fn, x, k: int, args, allow, groups: bool = False, third=None):
        """The frame of the top-k searches: ``fn(handle, x, nq, k, *args, allow bits, D, I[, third])`` into fresh
        ``[nq, k]`` arrays -- scores, ids and an optional third array of dtype ``third`` (``groups``: int32 labels;
        ``np.float32``: the raw scores of ``search_prior``); no query, no call."""
        nq = x.shape[0]
        out = (np.empty((nq, k), dtype=np.float32), np.empty((nq, k), dtype=np.int64))
        if groups:
            third = np.int32
        if third is not None:
            out += (np.empty((nq, k), dtype=third),)
        bits, bits_ptr = self._allow_bits(allow)
        if nq:
            nat.check(fn(self._handle(), x.ctypes.data, nq, k, *args, bits_ptr, *(o.ctypes.data for o in out)))
        return out

    # -- faiss surface ----------------------------------------------------
    @property
    def ntotal(self) -> int:
        return self._read_i64(nat.lib().css_index_ntotal)

    def reset(self) -> None:
        nat.check(nat.lib().css_index_reset(self._handle()))
        self._terms_rows = 0

    def reserve(self, n: int) -> None:
        nat.check(nat.lib().css_index_reserve(self._handle(), int(n)))

    def remove_ids(self, ids) -> int:
        """``faiss.IndexFlat.remove_ids``: drop the rows named by ``ids`` (integer row ids, or a boolean mask of
        ``ntotal`` entries meaning "remove"), in place in HBM; later rows shift down.  Ids out of range or repeated
        are ignored.  Returns the number of rows removed."""
        n = self.ntotal
        keep = keep_mask_from_ids(ids, n)
        if n == 0 or bool(keep.all()):
            return 0
        bits = pack_allow_bits(keep, n)
        removed = ctypes.c_int64(0)
        nat.check(nat.lib().css_index_remove_rows(self._handle(), bits.ctypes.data, ctypes.byref(removed)))
        self._terms_rows = int(np.count_nonzero(keep[:self._terms_rows]))   # (the lists were compacted with the rows)
        return int(removed.value)

    def bounds(self) -> dict:
        """Diagnostics: the running maxima over the rows that the error bands of the candidate scans are built from
        (``max ||x||^2``, ``max ||x - bf16(x)||^2``, ``max ||x - int8(x)||^2``)."""
        out = (ctypes.c_float * 3)()
        nat.check(nat.lib().css_index_bounds(self._handle(), out))
        return {"max_norm2": float(out[0]), "max_bf16_err2": float(out[1]), "max_int8_err2": float(out[2])}

    def add(self, x, normalize: bool = False) -> None:
        """Append rows; ids are ``ntotal .. ntotal+n-1`` (``src/storage.py:358-365``).
        ``normalize=True`` fuses the reference's ``x / (||x|| + 1e-8)``
        (``src/storage.py:347-350``) into the ingest kernel."""
        a = _as_f32_2d(x, self.d, "add")
        if a.shape[0] == 0:
            return
        nat.check(nat.lib().css_index_add(self._handle(), a.ctypes.data, a.shape[0], 1 if normalize else 0))

    def add_dev(self, x_ptr: int, n: int, normalize: bool = False, stream: int = 0) -> None:
        """Device-pointer twin of ``add``: ``x_ptr`` = device address of ``[n, d]`` fp32 rows (``tensor.data_ptr()``),
        enqueued on ``stream``; later searches are ordered behind it by the library."""
        if n:
            nat.check(nat.lib().css_index_add_dev(self._handle(), ctypes.c_void_p(x_ptr), int(n), 1 if normalize else 0,
                                                  ctypes.c_void_p(stream)))

    def add_synthetic(self, n: int, seed: int, first_row: int = 0, normalize: bool = True, stream: int = 0) -> None:
        nat.check(nat.lib().css_index_add_synthetic(self._handle(), int(n), ctypes.c_uint64(seed), int(first_row),
                                                    1 if normalize else 0, ctypes.c_void_p(stream)))

    def search(self, q, k: int, normalize: bool = False, allow=None) -> Tuple[np.ndarray, np.ndarray]:
        """``(D[nq,k] float32, I[nq,k] int64)``; IP descending, L2 ascending squared
        distances, ``-1`` padded (``src/storage.py:436``).  ``allow`` (optional boolean array of
        ``ntotal`` entries) restricts the answer to the rows marked True -- the filter / tombstone
        push-down the reference approximates by over-fetching (``src/storage.py:438-492``)."""
        a = _as_f32_2d(q, self.d, "search")
        k = int(k)
        if k < 1 or k > nat.MAX_K:
            raise ValueError(f"k={k} outside [1, {nat.MAX_K}]")
        return self._topk(nat.lib().css_index_search_masked, a, k, (1 if normalize else 0,), allow)

    def range_search(self, q, thresh: float, normalize: bool = False, allow=None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """``faiss.IndexFlat.range_search``: ``(lims[nq+1] int64, D[total] float32, I[total] int64)``; query ``j``'s
        hits are ``D/I[lims[j]:lims[j+1]]`` -- EVERY row with ``score > thresh`` (inner product) or squared distance
        ``< thresh`` (L2), strict as in faiss.  Unlike faiss the order inside a query is defined: best score first,
        equal scores by ascending id.  Scores come from an exact fp32 sweep of the fp32 rows (``css_index_range_search``);
        ``allow`` restricts the answer as in ``search``."""
        a = _as_f32_2d(q, self.d, "range_search")
        nq = a.shape[0]
        h = self._handle()
        bits, bits_ptr = self._allow_bits(allow)
        res = ctypes.c_void_p()
        nat.check(nat.lib().css_index_range_search(h, a.ctypes.data if nq else None, nq, float(thresh),
                                                   1 if normalize else 0, bits_ptr, ctypes.byref(res)))
        try:
            lims = np.zeros(nq + 1, dtype=np.int64)
            nat.check(nat.lib().css_range_result_lims(res, lims.ctypes.data))
            total = int(lims[nq])
            D = np.empty(total, dtype=np.float32)
            I = np.empty(total, dtype=np.int64)
            if total:
                nat.check(nat.lib().css_range_result_read(res, D.ctypes.data, I.ctypes.data))
        finally:
            nat.lib().css_range_result_free(res)
        return lims, D, I

    def facets(self, q, thresh: float, buckets=None, nbuckets: Optional[int] = None, normalize: bool = False,
               allow=None, by_attribute: Optional[int] = None) -> FacetCounts:
        """Where the matches lie (``css_index_facets``): for every query the number of rows with ``score > thresh``
        (inner product) or squared distance ``< thresh`` (L2) -- strict, the hits of ``range_search`` -- in each of
        ``nbuckets`` buckets, and the best such row per bucket (best score, ties to the smallest id), as a
        ``FacetCounts``.  ``buckets`` is an integer array of ``ntotal`` entries that fit int32, in LOCAL row numbering
        like ``allow``, uploaded for this call only; ``None`` means the ``set_groups`` labels (nothing is uploaded) and
        ``nbuckets`` is then required.  ``nbuckets=None`` with ``buckets`` given means ``max(buckets) + 1``.  A hit whose
        bucket is negative or ``>= nbuckets`` counts in ``unbucketed`` only.  Counts are integers and scores come from
        the exact fp32 sweep of ``range_search``: the result is the same bytes on every call.  ``by_attribute=slot``
        takes the int32 attribute column ``slot`` (``set_attribute``) as the buckets -- what ``buckets=get_attribute(slot)``
        answers, without the upload; ``nbuckets`` is then required and ``buckets`` must be ``None``."""
        a = _as_f32_2d(q, self.d, "facets")
        nq = a.shape[0]
        if by_attribute is not None:
            slot = attr_slot(by_attribute, "facets")
            if buckets is not None:
                raise ValueError("facets: give buckets or by_attribute, not both")
            if nbuckets is None:
                raise ValueError("facets: nbuckets is required with by_attribute")
            typ = self.attribute_type(slot)
            if typ != ATTR_I32:
                raise ValueError(f"facets: attribute slot {slot} " + ("was never set" if typ < 0 else "holds float32 values"))
        thresh, b, nb = facet_args(thresh, buckets, nbuckets, self.ntotal)
        bits, bits_ptr = self._allow_bits(allow)
        pad = -np.finfo(np.float32).max if self.metric_type == METRIC_INNER_PRODUCT else np.finfo(np.float32).max
        out = FacetCounts(np.zeros((nq, nb), dtype=np.int64), np.full((nq, nb), pad, dtype=np.float32),
                          np.full((nq, nb), -1, dtype=np.int64), np.zeros(nq, dtype=np.int64), np.zeros(nq, dtype=np.int64))
        if nq and by_attribute is not None:
            nat.check(nat.lib().css_index_facets_attr(self._handle(), a.ctypes.data, nq, thresh, 1 if normalize else 0,
                                                      bits_ptr, slot, nb, out.counts.ctypes.data,
                                                      out.best_score.ctypes.data, out.best_id.ctypes.data,
                                                      out.total.ctypes.data, out.unbucketed.ctypes.data))
        elif nq:
            nat.check(nat.lib().css_index_facets(self._handle(), a.ctypes.data, nq, thresh, 1 if normalize else 0, bits_ptr,
                                                 None if b is None else b.ctypes.data, nb, out.counts.ctypes.data,
                                                 out.best_score.ctypes.data, out.best_id.ctypes.data, out.total.ctypes.data,
                                                 out.unbucketed.ctypes.data))
        return out

    def last_facet_sweeps(self) -> Tuple[int, int]:
        """Diagnostics: ``(sweeps, lds_sweeps)`` of the last ``facets`` call -- the sweeps of the rows it ran and how many
        of them kept their table in LDS."""
        n, m = ctypes.c_int64(0), ctypes.c_int64(0)
        nat.check(nat.lib().css_index_last_facet_sweeps(self._handle(), ctypes.byref(n), ctypes.byref(m)))
        return int(n.value), int(m.value)

    def set_facet_lds_entries(self, entries: int) -> None:
        """The largest table (queries x buckets of one sweep) that ``facets`` keeps in LDS (-1 = the library's rule,
        0 = never); the result does not depend on it."""
        nat.check(nat.lib().css_index_set_facet_lds_entries(self._handle(), int(entries)))

    # -- per-row columns: the range check, and the setter and getter of a 4-byte column -----
    def _row_range(self, what: str, row0, n) -> Tuple[int, int]:
        """``(row0, n)`` as ints, ``n = None`` meaning "to the end"; raises unless ``[row0, row0 + n)`` are rows."""
        row0 = int(row0)
        total = self.ntotal
        n = total - row0 if n is None else int(n)
        if row0 < 0 or n < 0 or row0 + n > total:
            raise ValueError(f"{what}: rows [{row0}, {row0 + n}) outside [0, {total})")
        return row0, n

    def _set_column(self, what: str, convert, values, row0) -> None:
        a = convert(values)
        row0, n = self._row_range(what, row0, a.shape[0])
        if n:
            nat.check(getattr(nat.lib(), "css_index_" + what)(self._handle(), row0, n, a.ctypes.data))

    def _get_column(self, what: str, dtype, row0, n) -> np.ndarray:
        row0, n = self._row_range(what, row0, n)
        out = np.empty(n, dtype=dtype)
        if n:
            nat.check(getattr(nat.lib(), "css_index_" + what)(self._handle(), row0, n, out.ctypes.data))
        return out

    # -- attribute columns and filters on the device ---------------------------
    def set_attribute(self, slot: int, values, row0: int = 0) -> None:
        """Values of attribute ``slot`` (``0 <= slot < MAX_ATTRS``) for rows ``[row0, row0 + len(values))`` in LOCAL row
        numbering: an integer (or boolean) array gives an int32 column and is range-checked, a floating array a float32
        column; the first set types the slot and a later set of the other kind raises.  Rows never given a value, and
        rows added later, hold ``-1`` / NaN.  The columns follow the rows through growth, ``remove_ids`` (compacted with
        them) and ``reset`` (values and types forgotten)."""
        slot = attr_slot(slot)
        a, typ = attr_values(values)
        row0, n = self._row_range("set_attribute", row0, a.shape[0])
        if n:
            nat.check(nat.lib().css_index_set_attr(self._handle(), slot, typ, row0, n, a.ctypes.data))

    def get_attribute(self, slot: int, row0: int = 0, n: Optional[int] = None) -> np.ndarray:
        """The values of attribute ``slot`` for rows ``[row0, row0 + n)`` (default: to the end), int32 or float32 by the
        slot's type; a slot that was never set answers int32 ``-1``."""
        slot = attr_slot(slot, "get_attribute")
        row0, n = self._row_range("get_attribute", row0, n)
        out = np.empty(n, dtype=np.float32 if self.attribute_type(slot) == ATTR_F32 else np.int32)
        if n:
            nat.check(nat.lib().css_index_get_attr(self._handle(), slot, row0, n, out.ctypes.data))
        return out

    def attribute_type(self, slot: int) -> int:
        """``ATTR_I32``, ``ATTR_F32``, or ``-1`` for a slot that was never set."""
        t = ctypes.c_int(-1)
        nat.check(nat.lib().css_index_attr_type(self._handle(), attr_slot(slot, "attribute_type"), ctypes.byref(t)))
        return int(t.value)

    def drop_attribute(self, slot: int) -> None:
        """Free attribute ``slot`` and forget its type."""
        nat.check(nat.lib().css_index_drop_attr(self._handle(), attr_slot(slot, "drop_attribute")))

    def where_bits(self, clauses, allow=None, out: Optional[np.ndarray] = None) -> Tuple[np.ndarray, int]:
        """``where`` in the form the library answers: ``(uint32 bitmap of ceil(ntotal / 32) words, number of set bits)``.
        ``out`` (optional) is a contiguous uint32 array of exactly that many words to write into."""
        args = where_args(clauses, self.attribute_type)
        ntotal = self.ntotal
        words = (ntotal + 31) // 32
        if out is None:
            out = np.zeros(words, dtype="<u4")
        elif out.dtype != np.dtype("<u4") or out.ndim != 1 or out.shape[0] != words or not out.flags.c_contiguous:
            raise ValueError(f"where: out must be a contiguous uint32 array of {words} words")
        cl = (nat.Clause * max(len(args.clauses), 1))()
        for c, (slot, code, value, off, nbits) in enumerate(args.clauses):
            cl[c] = nat.Clause(slot, code, value, 0, off, nbits)
        bits, bits_ptr = self._allow_bits(allow)
        count = ctypes.c_int64(0)
        nat.check(nat.lib().css_index_where(self._handle(), cl, len(args.clauses),
                                            args.tables.ctypes.data if args.tables.size else None, args.tables.shape[0],
                                            bits_ptr, out.ctypes.data if words else None, ctypes.byref(count)))
        return out, int(count.value)

    def where(self, clauses, allow=None, return_count: bool = False):
        """The rows that pass a filter, evaluated on the device (``css_index_where``): the boolean mask of ``ntotal``
        entries that every search method accepts as ``allow``.  ``clauses`` is a sequence of at most ``MAX_CLAUSES``
        triples ``(slot, op, operand)``, all of which must hold (AND); ``op`` is one of ``== != < <= > >= in "not in"``,
        compared as numpy compares int32 / float32 arrays (``where_numpy``); the operand of ``in`` / ``not in`` (int32
        slots only) is an iterable of non-negative integers.  ``allow`` is ANDed in; no clause answers ``allow`` (or
        every row).  ``return_count=True`` returns ``(mask, number of rows that pass)``."""
        bits, count = self.where_bits(clauses, allow)
        ntotal = self.ntotal
        mask = np.unpackbits(bits.view(np.uint8), bitorder="little")[:ntotal].astype(np.bool_)
        return (mask, count) if return_count else mask

    # -- group labels and grouped search ------------------------------------
    def set_groups(self, labels, row0: int = 0) -> None:
        """Group labels of rows ``[row0, row0 + len(labels))`` in LOCAL row numbering (like ``allow``): an integer
        array that fits int32.  A negative label means "ungrouped" and is stored as ``-1``; rows never given a label
        are ungrouped too.  The labels follow the rows through growth, ``remove_ids`` (compacted with them) and
        ``reset`` (forgotten); rows added later start ungrouped."""
        self._set_column("set_groups", labels_as_int32, labels, row0)

    def get_groups(self, row0: int = 0, n: Optional[int] = None) -> np.ndarray:
        """The labels of rows ``[row0, row0 + n)`` (default: to the end) as int32; ``-1`` = ungrouped."""
        return self._get_column("get_groups", np.int32, row0, n)

    def search_grouped(self, q, k: int, normalize: bool = False, allow=None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """The ``k`` best GROUPS per query (``css_index_search_grouped``): ``(D[nq,k], I[nq,k], G[nq,k] int32)`` -- score
        and global id of each group's best allowed row and the group's label, best group first, ties to the lower id,
        padded like ``search`` with ``G = -1``.  An ungrouped row (label ``-1``) is a group of its own.  Exact: the
        ordinary search runs for 32 or 128 rows, the list is collapsed on the device, and queries that still lack
        groups run further passes without the rows of the groups already found.  ``1 <= k <= 128``."""
        a = _as_f32_2d(q, self.d, "search_grouped")
        k = int(k)
        if k < 1 or k > MAX_GROUP_K:
            raise ValueError(f"k={k} outside [1, {MAX_GROUP_K}]")
        return self._topk(nat.lib().css_index_search_grouped, a, k, (1 if normalize else 0,), allow, groups=True)

    def last_group_passes(self) -> int:
        """Diagnostics: search passes of the last ``search_grouped`` call (1 when the first pass sufficed for every
        query)."""
        return self._read_i64(nat.lib().css_index_last_group_passes)

    # -- per-row priors and prior-weighted search -----------------------------
    def set_priors(self, priors, row0: int = 0) -> None:
        """Priors of rows ``[row0, row0 + len(priors))`` in LOCAL row numbering (like ``allow``): real numbers, stored as
        float32.  Rows never given one have ``0.0``.  NaN or infinity raises and writes nothing.  The priors follow
        the rows through growth, ``remove_ids`` (compacted with them) and ``reset`` (forgotten); rows added later start
        at ``0.0``."""
        self._set_column("set_priors", priors_as_f32, priors, row0)

    def get_priors(self, row0: int = 0, n: Optional[int] = None) -> np.ndarray:
        """The priors of rows ``[row0, row0 + n)`` (default: to the end) as float32."""
        return self._get_column("get_priors", np.float32, row0, n)

    def search_prior(self, q, k: int, weight: float, normalize: bool = False,
                     allow=None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """The ``k`` best rows per query under ``score + weight * prior`` (``css_index_search_prior``; L2:
        ``distance - weight * prior``, smaller is better): ``(D[nq,k], I[nq,k], S[nq,k] float32)`` -- the fused value,
        the global id and the row's RAW score, best fused value first, ties to the lower id, padded like ``search``
        (``S`` like ``D``).  Exact over ALL allowed rows, not a re-rank of an over-fetched list: scores come from an
        exact fp32 sweep of the fp32 rows, whatever the search mode.  ``weight`` is any finite float;
        ``1 <= k <= 128``.  Without priors, or with ``weight = 0``, ``D == S`` is the exact-fp32 ``search``."""
        a = _as_f32_2d(q, self.d, "search_prior")
        k, weight = int(k), float(weight)
        if k < 1 or k > MAX_PRIOR_K:
            raise ValueError(f"k={k} outside [1, {MAX_PRIOR_K}]")
        if not np.isfinite(weight):
            raise ValueError(f"weight={weight} is not finite")
        self._handle()   # (a freed index raises even without queries)
        return self._topk(nat.lib().css_index_search_prior, a, k, (weight, 1 if normalize else 0), allow, third=np.float32)

    # -- search by examples ---------------------------------------------------
    def search_examples(self, pos=None, neg=None, pos_ids=(), neg_ids=(), k: int = 10, gamma: float = 0.5,
                        normalize: bool = False, exclude_ids: bool = True,
                        allow=None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """"More like these, and not like those" (``css_index_search_examples``): the ``k`` best allowed rows under
        ``best positive score - gamma * best negative score`` for ONE request of up to 16 examples.  ``pos`` / ``neg``
        are example vectors (``[n, d]`` or ``[d]``; ``normalize``: ``x / (||x|| + 1e-8)``), ``pos_ids`` / ``neg_ids``
        stored rows by global id, taken as they lie in HBM.  At least one positive.  Returns
        ``(D[k], I[k], S[k] float32)``: the fused value (``fuse_example_scores`` states it), the global id and the RAW best
        positive score, best first, ties to the lower id, padded like ``search`` (``S`` like ``D``).  Exact over ALL
        allowed rows from an fp32 sweep of the fp32 rows, whatever the search mode -- not a re-rank of a fetched list.
        ``exclude_ids``: rows named as id examples are never returned (copies under other ids are).  ``allow`` applies to
        the answer, not to the examples.  ``gamma`` (finite, ``>= 0``) defaults to 0.5 as an interface default, not a
        measurement; ``1 <= k <= 128``."""
        what = "search_examples"
        vp, vn = example_vectors(pos, self.d, what), example_vectors(neg, self.d, what)
        ip, ineg = ids_as_int64(pos_ids, what), ids_as_int64(neg_ids, what)
        k, gamma = example_args(k, gamma, vp.shape[0] + ip.shape[0], vp.shape[0] + vn.shape[0] + ip.shape[0] + ineg.shape[0])
        h = self._handle()
        # (one kind only is the usual request: no copy then)
        vec = vp if not vn.shape[0] else vn if not vp.shape[0] else np.concatenate([vp, vn], axis=0)
        ids = ip if not ineg.shape[0] else ineg if not ip.shape[0] else np.concatenate([ip, ineg])
        D, I, S = np.empty(k, dtype=np.float32), np.empty(k, dtype=np.int64), np.empty(k, dtype=np.float32)
        bits, bits_ptr = self._allow_bits(allow)
        nat.check(nat.lib().css_index_search_examples(
            h, vec.ctypes.data if vec.shape[0] else None, vp.shape[0], vn.shape[0],
            ids.ctypes.data if ids.shape[0] else None, ip.shape[0], ineg.shape[0], k, gamma, 1 if normalize else 0,
            1 if exclude_ids else 0, bits_ptr, D.ctypes.data, I.ctypes.data, S.ctypes.data))
        return D, I, S

    # -- per-row term lists and hybrid search ---------------------------------
    def set_terms(self, lists, row0: Optional[int] = None) -> None:
        """Term lists of rows ``[row0, row0 + n)`` in LOCAL row numbering (``css_index_set_terms``).  ``lists`` is a
        sequence of int sequences (the raw term ids of each row's text, e.g. ``lexical.terms_of``: repeats, any order
        and empty rows allowed) or an ``(offsets, tokens)`` pair of arrays in CSR form.  Lists are APPEND-ONLY in row
        order: with ``T`` the leading rows that have lists, ``row0 = None`` or ``T`` appends, ``row0 < T`` first drops
        the lists of all rows ``>= row0`` (``row0 = 0`` rewrites), ``row0 > T`` raises.  The lists follow the rows
        through growth, ``remove_ids`` (compacted with them) and ``reset`` (forgotten); rows added later have none."""
        from .lexical import lists_as_csr

        off, tok = lists_as_csr(lists)
        row0 = self._terms_rows if row0 is None else int(row0)
        n = off.shape[0] - 1
        nat.check(nat.lib().css_index_set_terms(self._handle(), row0, n, off.ctypes.data, tok.ctypes.data if tok.size else None))
        if n or row0 < self._terms_rows:
            self._terms_rows = row0 + n

    def get_terms(self, row0: int = 0, n: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """The stored lists of rows ``[row0, row0 + n)`` (default: to the end): ``(offsets int64 [n + 1] from 0, terms
        uint32, tfs uint8, dl uint32 [n])`` -- per row the distinct terms ascending, their counts saturated at 255, and
        the number of tokens the row was given.  Rows without a list are empty with ``dl = 0``."""
        row0, n = self._row_range("get_terms", row0, n)
        off = np.zeros(n + 1, dtype=np.int64)
        dl = np.zeros(n, dtype=np.uint32)
        self._handle()
        if n == 0:
            return off, np.zeros(0, np.uint32), np.zeros(0, np.uint8), dl
        nat.check(nat.lib().css_index_get_terms(self._handle(), row0, n, off.ctypes.data, None, None))
        ent = np.zeros(int(off[-1]), dtype=np.uint32)
        nat.check(nat.lib().css_index_get_terms(self._handle(), row0, n, off.ctypes.data, ent.ctypes.data if ent.size else None,
                                                dl.ctypes.data))
        return off, ent >> np.uint32(8), (ent & np.uint32(255)).astype(np.uint8), dl

    def term_stats(self, terms) -> Tuple[np.ndarray, int, int]:
        """``(df int64 [m], ndocs, total_len)``: the number of rows that hold each asked term, ``ntotal``, and the sum
        of the rows' lengths (``css_index_term_stats``).  Zeros on an index without lists."""
        t = np.asarray(terms, dtype=np.int64).reshape(-1)
        if t.size and (int(t.min()) < 0 or int(t.max()) >= nat.TERM_SPACE):
            raise ValueError("term_stats: a term outside [0, 2^24)")
        t = np.ascontiguousarray(t, dtype=np.uint32)
        df = np.zeros(t.shape[0], dtype=np.int64)
        ndocs, total = ctypes.c_int64(0), ctypes.c_int64(0)
        nat.check(nat.lib().css_index_term_stats(self._handle(), t.ctypes.data if t.size else None, t.shape[0],
                                                 df.ctypes.data if t.size else None, ctypes.byref(ndocs), ctypes.byref(total)))
        return df, int(ndocs.value), int(total.value)

    # -- significant terms -------------------------------------------------------
    def subset_terms(self, allow=None) -> Tuple[np.ndarray, np.ndarray]:
        """``(terms uint32 ascending, fg int64)``: every term that a selected row's list holds, with the number of
        selected rows that hold it (``css_index_subset_terms``; ``allow=None``: every row that has a list).  Counted on
        the GPU over the lists of the selected rows only; the form the sharded index exchanges."""
        return self._subset_terms(allow)[:2]

    def _subset_terms(self, allow) -> Tuple[np.ndarray, np.ndarray, int]:
        """``subset_terms`` and the number of selected rows that have a list."""
        h = self._handle()
        bits, bits_ptr = self._allow_bits(allow)
        n, rows = ctypes.c_int64(0), ctypes.c_int64(0)
        cap = 1 << 16   # (one call answers a small selection; a larger one is sized by the first)
        while True:
            terms, fg = np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.int64)
            nat.check(nat.lib().css_index_subset_terms(h, bits_ptr, cap, terms.ctypes.data, fg.ctypes.data, ctypes.byref(n),
                                                       ctypes.byref(rows)))
            if n.value <= cap:
                return terms[:n.value].copy(), fg[:n.value].copy(), int(rows.value)
            cap = int(n.value)

    def significant_terms(self, allow=None, m: int = 20, min_count: int = 2, background=None):
        """The ``m`` terms that set the selected rows apart from the background (``css_index_significant_terms``): a
        ``lexical.SignificantTerms`` ``(terms, fg, bg, score float64, n_fg, n_bg)``, best first, cut to the terms that
        qualified.  ``allow`` selects the rows (``None``: every row with a list), ``background`` the rows they are
        compared with (``None``: every row with a list, counted by the standing df table); the selection must lie within
        the background, else ``ValueError``.  A term qualifies iff at least ``min_count`` selected rows hold it and it
        is more frequent in the selection than in the background; the score is JLH in float64
        (``lexical.significant_from_counts`` states the same bits).  ``1 <= m <= 256``."""
        from .lexical import SignificantTerms, significant_args

        m, min_count = significant_args(m, min_count)
        h = self._handle()
        bits, bits_ptr = self._allow_bits(allow)
        bg_bits, bg_ptr = self._allow_bits(background)
        if background is not None:
            T = self._terms_rows
            sel = np.ones(T, dtype=bool) if allow is None else np.asarray(allow)[:T]
            bad = np.flatnonzero(sel & ~np.asarray(background)[:T])
            if bad.size:
                raise ValueError(f"significant_terms: row {int(bad[0])} is selected but not in the background")
        terms, score = np.zeros(m, dtype=np.uint32), np.zeros(m, dtype=np.float64)
        fg, bg = np.zeros(m, dtype=np.int64), np.zeros(m, dtype=np.int64)
        n, n_fg, n_bg = ctypes.c_int(0), ctypes.c_int64(0), ctypes.c_int64(0)
        nat.check(nat.lib().css_index_significant_terms(h, bits_ptr, bg_ptr, m, min_count, terms.ctypes.data, fg.ctypes.data,
                                                        bg.ctypes.data, score.ctypes.data, ctypes.byref(n), ctypes.byref(n_fg),
                                                        ctypes.byref(n_bg)))
        k = int(n.value)
        return SignificantTerms(terms[:k].copy(), fg[:k].copy(), bg[:k].copy(), score[:k].copy(), int(n_fg.value), int(n_bg.value))

    def set_sigterm_slots(self, slots: int) -> None:
        """LDS slots per block in which the counting pass of ``subset_terms`` / ``significant_terms`` merges repeated
        terms (-1 = the library's rule, 0 = none: every entry is one global add); the integers do not depend on it."""
        nat.check(nat.lib().css_index_set_sigterm_slots(self._handle(), int(slots)))

    def search_hybrid(self, q, terms, weights, k: int, alpha: float, k1: float = 1.2, b: float = 0.75,
                      avgdl: Optional[float] = None, normalize: bool = False,
                      allow=None) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """The ``k`` best rows for ONE query under ``score + alpha * lex`` (``css_index_search_hybrid``; L2:
        ``distance - alpha * lex``, smaller is better), ``lex`` = the BM25 score of the query's ``terms`` (distinct ids,
        at most 32) with the caller's ``weights`` (``lexical.bm25_weights``) against the row's term list, formed on the
        device in fp32 in query-term order: ``(D, I, S, L)``, each ``[1, k]`` -- the fused value, the global id, the
        row's RAW score and its ``lex``; best fused value first, ties to the lower id, padded like ``search_prior``
        (``L = 0``).  Exact over ALL allowed rows: a row that holds a rare query term is found however far down the
        plain ranking it sits.  ``avgdl=None`` takes ``total_len / ndocs`` from ``term_stats`` (1.0 when that is 0).
        No terms, ``alpha = 0`` or an index without lists give ``search_prior`` without priors."""
        a = _as_f32_2d(q, self.d, "search_hybrid")
        if a.shape[0] != 1:
            raise ValueError(f"search_hybrid: one query per call, got {a.shape[0]}")
        t, w, k, alpha, k1, b, avgdl = hybrid_args(terms, weights, k, alpha, k1, b, avgdl)
        self._handle()
        if avgdl is None:
            _, ndocs, total = self.term_stats(())
            avgdl = total / ndocs if ndocs > 0 and total > 0 else 1.0
        D, I = np.empty((1, k), dtype=np.float32), np.empty((1, k), dtype=np.int64)
        S, L = np.empty((1, k), dtype=np.float32), np.empty((1, k), dtype=np.float32)
        bits, bits_ptr = self._allow_bits(allow)
        nat.check(nat.lib().css_index_search_hybrid(
            self._handle(), a.ctypes.data, k, alpha, t.ctypes.data if t.size else None, w.ctypes.data if t.size else None,
            t.shape[0], k1, b, float(np.float32(avgdl)), 1 if normalize else 0, bits_ptr, D.ctypes.data, I.ctypes.data,
            S.ctypes.data, L.ctypes.data))
        return D, I, S, L

    # -- per-row sparse vectors and sparse search ------------------------------
    def set_sparse(self, vectors, row0: Optional[int] = None) -> None:
        """Sparse vectors of rows ``[row0, row0 + n)`` in LOCAL row numbering (``css_index_set_sparse``).  ``vectors`` is
        a sequence of ``SparseVector`` or ``(terms, weights)`` pairs (e.g. ``SparseEncoder.encode``: any order within a
        row, empty rows allowed) or an ``(offsets, terms, weights)`` triple of arrays in CSR form.  Terms are distinct
        within a row and below 2^24; weights are finite, ``> 0`` and ``<= 65536``; at most 65536 entries per row.
        APPEND-ONLY in row order like ``set_terms`` and independent of it: with ``T = sparse_rows``, ``row0 = None`` or
        ``T`` appends, ``row0 < T`` first drops the vectors of all rows ``>= row0``, ``row0 > T`` raises.  The vectors
        follow the rows through growth, ``remove_ids`` (compacted with them) and ``reset`` (forgotten); rows added
        later have none."""
        off, t, w = sparse_as_csr(vectors)
        row0 = self.sparse_rows if row0 is None else int(row0)
        nat.check(nat.lib().css_index_set_sparse(self._handle(), row0, off.shape[0] - 1, off.ctypes.data,
                                                 t.ctypes.data if t.size else None, w.ctypes.data if w.size else None))

    def get_sparse(self, row0: int = 0, n: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """The stored vectors of rows ``[row0, row0 + n)`` (default: to the end): ``(offsets int64 [n + 1] from 0, terms
        uint32, weights float32)``, per row ascending by term.  Rows without a vector are empty."""
        row0, n = self._row_range("get_sparse", row0, n)
        off = np.zeros(n + 1, dtype=np.int64)
        self._handle()
        if n == 0:
            return off, np.zeros(0, np.uint32), np.zeros(0, np.float32)
        nat.check(nat.lib().css_index_get_sparse(self._handle(), row0, n, off.ctypes.data, None, None))
        t, w = np.zeros(int(off[-1]), dtype=np.uint32), np.zeros(int(off[-1]), dtype=np.float32)
        if t.size:
            nat.check(nat.lib().css_index_get_sparse(self._handle(), row0, n, off.ctypes.data, t.ctypes.data, w.ctypes.data))
        return off, t, w

    @property
    def sparse_rows(self) -> int:
        """The number of leading rows that have sparse vectors."""
        return self._read_i64(nat.lib().css_index_sparse_rows)

    def search_sparse(self, terms, weights, k: int, allow=None) -> Tuple[np.ndarray, np.ndarray]:
        """The ``k`` best rows for ONE sparse query by the dot product with the rows' sparse vectors ALONE
        (``css_index_search_sparse``): ``(D, I)``, each ``[1, k]`` -- the dot product, formed on the device in fp32 in
        query-term order, and the global id; larger first on an index of either metric, ties to the lower id.  Only
        HIT rows are returned, rows that share at least one term with the query; fewer than ``k`` of them, no terms or
        an index without vectors pad with ``I = -1``, ``D = -FLT_MAX``.  No dense row is read.  ``terms`` are distinct
        ids (at most 64; or a ``SparseVector`` with ``weights=None``), ``weights`` finite, nonzero, at most 65536 in
        size; negative ones are allowed."""
        t, w, k, _ = sparse_args(terms, weights, k)
        D, I = np.empty((1, k), dtype=np.float32), np.empty((1, k), dtype=np.int64)
        h = self._handle()
        bits, bits_ptr = self._allow_bits(allow)
        nat.check(nat.lib().css_index_search_sparse(h, t.ctypes.data if t.size else None, w.ctypes.data if t.size else None,
                                                    t.shape[0], k, bits_ptr, D.ctypes.data, I.ctypes.data))
        return D, I

    def search_hybrid_sparse(self, q, terms, weights, k: int, alpha: float, normalize: bool = False,
                             allow=None) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """``search_hybrid`` with the sparse dot product ``sp`` in the place of the BM25 score
        (``css_index_search_hybrid_sparse``): the ``k`` best rows for ONE query under ``score + alpha * sp`` (L2:
        ``distance - alpha * sp``), exact over ALL allowed rows: ``(D, I, S, L)``, each ``[1, k]``, ``L = sp`` of the
        returned rows (0 for a row that shares no term).  The query's sparse side is that of ``search_sparse``.  No
        terms, ``alpha = 0`` or an index without vectors give ``search_prior`` without priors."""
        a = _as_f32_2d(q, self.d, "search_hybrid_sparse")
        if a.shape[0] != 1:
            raise ValueError(f"search_hybrid_sparse: one query per call, got {a.shape[0]}")
        t, w, k, alpha = sparse_args(terms, weights, k, alpha, what="search_hybrid_sparse")
        D, I = np.empty((1, k), dtype=np.float32), np.empty((1, k), dtype=np.int64)
        S, L = np.empty((1, k), dtype=np.float32), np.empty((1, k), dtype=np.float32)
        h = self._handle()
        bits, bits_ptr = self._allow_bits(allow)
        nat.check(nat.lib().css_index_search_hybrid_sparse(
            h, a.ctypes.data, k, alpha, t.ctypes.data if t.size else None, w.ctypes.data if t.size else None, t.shape[0],
            1 if normalize else 0, bits_ptr, D.ctypes.data, I.ctypes.data, S.ctypes.data, L.ctypes.data))
        return D, I, S, L

    # -- per-row token matrices and MaxSim search ------------------------------
    def set_tokens(self, mats, keep=None, row0: Optional[int] = None) -> None:
        """Token matrices of rows ``[row0, row0 + n)`` in LOCAL row numbering (``css_index_set_tokens``).  ``mats`` is a
        sequence of ``[m_i, P]`` matrices of bf16 values (uint16 bits as ``LateInteraction.encode_documents`` gives them,
        or bf16-exact float32; empty rows allowed) or an ``(offsets, tokens, P)`` triple in CSR form.  ``keep`` per row
        is ColBERT's skiplist as in ``LateInteraction.score``: a dropped token is NOT STORED.  P is a multiple of 32 in
        [32, 128], fixed by the first call (only a rewrite from row 0 changes it); at most 512 tokens per row; finite
        components.  APPEND-ONLY in row order like ``set_sparse`` and independent of it: with ``T = token_rows``,
        ``row0 = None`` or ``T`` appends, ``row0 < T`` first drops the matrices of all rows ``>= row0``, ``row0 > T``
        raises.  The matrices follow the rows through growth, ``remove_ids`` (compacted with them) and ``reset``
        (forgotten); rows added later have none."""
        off, tok, P = tokens_as_csr(mats, keep)
        row0 = self.token_rows if row0 is None else int(row0)
        nat.check(nat.lib().css_index_set_tokens(self._handle(), row0, off.shape[0] - 1, off.ctypes.data,
                                                 tok.ctypes.data if tok.size else None, P))

    def get_tokens(self, row0: int = 0, n: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
        """The stored matrices of rows ``[row0, row0 + n)`` (default: to the end): ``(offsets int64 [n + 1] from 0,
        tokens uint16 [offsets[n], P])``.  Rows without a matrix are empty."""
        row0, n = self._row_range("get_tokens", row0, n)
        off = np.zeros(n + 1, dtype=np.int64)
        P = self.token_dim
        if n == 0 or P == 0:
            return off, np.zeros((0, P), np.uint16)
        nat.check(nat.lib().css_index_get_tokens(self._handle(), row0, n, off.ctypes.data, None))
        tok = np.zeros((int(off[-1]), P), dtype=np.uint16)
        if tok.size:
            nat.check(nat.lib().css_index_get_tokens(self._handle(), row0, n, off.ctypes.data, tok.ctypes.data))
        return off, tok

    @property
    def token_rows(self) -> int:
        """The number of leading rows that have token matrices."""
        return self._read_i64(nat.lib().css_index_token_rows)

    @property
    def token_dim(self) -> int:
        """The width P of the stored token vectors (0: no row has a matrix)."""
        p = ctypes.c_int(0)
        nat.check(nat.lib().css_index_token_dim(self._handle(), ctypes.byref(p)))
        return int(p.value)

    def drop_tokens(self) -> None:
        """Forget every token matrix and free their memory (``css_index_drop_tokens``)."""
        nat.check(nat.lib().css_index_drop_tokens(self._handle()))

    def set_token_blocks(self, blocks: int) -> None:
        """The grid of the MaxSim kernel (0 = the library's choice); the result does not depend on it."""
        nat.check(nat.lib().css_index_set_token_blocks(self._handle(), int(blocks)))

    # -- compressed token matrices (centroid + residual codes) ---------------------
    def set_token_codec(self, codec: Optional[TokenCodec]) -> None:
        """Store token matrices COMPRESSED from now on (``css_index_set_token_codec``): ``codec`` is a ``TokenCodec``
        (or a ``(centroids, nbits, cutoffs, weights)`` tuple), ``None`` clears it.  Allowed only while no row has a
        matrix.  With a codec ``set_tokens`` encodes on the GPU, ``get_tokens`` returns the DECODED matrices, and
        ``search_maxsim`` / ``maxsim_ids`` score the decoded matrices bit for bit.  The codec survives ``drop_tokens``,
        ``reset`` and ``remove_ids``."""
        if codec is None:
            nat.check(nat.lib().css_index_set_token_codec(self._handle(), None, 0, 0, 0, None, None))
            return
        c = token_codec_args(*codec)
        nat.check(nat.lib().css_index_set_token_codec(self._handle(), c.centroids.ctypes.data, c.centroids.shape[0], c.P,
                                                      c.nbits, c.cutoffs.ctypes.data, c.weights.ctypes.data))

    @property
    def token_codec_bits(self) -> int:
        """Bits per residual component of the index's token codec; 0 = no codec."""
        b = ctypes.c_int(0)
        nat.check(nat.lib().css_index_token_codec_bits(self._handle(), ctypes.byref(b)))
        return int(b.value)

    def get_token_codec(self) -> Optional[TokenCodec]:
        """The index's codec (``css_index_get_token_codec``), ``None`` without one."""
        C, P, nb = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        fn, h = nat.lib().css_index_get_token_codec, self._handle()
        nat.check(fn(h, ctypes.byref(C), ctypes.byref(P), ctypes.byref(nb), None, None, None))
        if nb.value == 0:
            return None
        cent = np.empty((C.value, P.value), dtype=np.float32)
        cut, w = np.empty((1 << nb.value) - 1, dtype=np.float32), np.empty(1 << nb.value, dtype=np.float32)
        nat.check(fn(h, None, None, None, cent.ctypes.data, cut.ctypes.data, w.ctypes.data))
        return TokenCodec(cent, int(nb.value), cut, w)

    def get_token_codes(self, row0: int = 0, n: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """The stored codes of rows ``[row0, row0 + n)`` (default: to the end) in the canonical layout, nothing decoded
        (``css_index_get_token_codes``): ``(offsets int64 [n + 1] from 0, codes uint16 [E], res uint8 [E, P * nbits / 8])``."""
        row0, n = self._row_range("get_token_codes", row0, n)
        codec = self.get_token_codec()
        if codec is None:
            raise ValueError("get_token_codes: the index has no token codec")
        off = np.zeros(n + 1, dtype=np.int64)
        fn, h = nat.lib().css_index_get_token_codes, self._handle()
        nat.check(fn(h, row0, n, off.ctypes.data, None, None))
        codes = np.zeros(int(off[-1]), dtype=np.uint16)
        res = np.zeros((int(off[-1]), codec.res_bytes), dtype=np.uint8)
        if codes.size:
            nat.check(fn(h, row0, n, off.ctypes.data, codes.ctypes.data, res.ctypes.data))
        return off, codes, res

    def set_token_codes(self, offsets, codes, res, row0: Optional[int] = None) -> None:
        """Canonical codes as ``get_token_codes`` gives them, stored without encoding (``css_index_set_token_codes``):
        save / load and shards.  The index needs the codec they were made with; the append-only rules of ``set_tokens``."""
        codec = self.get_token_codec()
        if codec is None:
            raise ValueError("set_token_codes: the index has no token codec")
        off, codes, res = token_codes_as_csr(offsets, codes, res, codec)
        row0 = self.token_rows if row0 is None else int(row0)
        nat.check(nat.lib().css_index_set_token_codes(self._handle(), row0, off.shape[0] - 1, off.ctypes.data,
                                                      codes.ctypes.data if codes.size else None,
                                                      res.ctypes.data if codes.size else None))

    def search_maxsim(self, q_mat, k: int, allow=None) -> Tuple[np.ndarray, np.ndarray]:
        """The ``k`` best rows for ONE query matrix ``[mq, P]`` by MaxSim with the rows' token matrices ALONE
        (``css_index_search_maxsim``): ``(D, I)``, each ``[1, k]`` -- the score ``sum_s max_t dot(q_s, d_t)``, bit for
        bit what ``MpnetEncoder.maxsim`` gives for the same matrices, and the global id; larger first on an index of
        either metric, ties to the lower id.  Rows without tokens are never returned; fewer than ``k`` hits or an
        index without matrices pad with ``I = -1``, ``D = -FLT_MAX``.  No dense row is read."""
        q, k, _ = maxsim_args(q_mat, k)
        D, I = np.empty((1, k), dtype=np.float32), np.empty((1, k), dtype=np.int64)
        h = self._handle()
        bits, bits_ptr = self._allow_bits(allow)
        nat.check(nat.lib().css_index_search_maxsim(h, q.ctypes.data, q.shape[0], q.shape[1], k, bits_ptr, D.ctypes.data,
                                                    I.ctypes.data))
        return D, I

    def search_maxsim_batch(self, q_mats, k: int, allow=None) -> Tuple[np.ndarray, np.ndarray]:
        """``search_maxsim`` for a sequence of up to 1024 query matrices in one call
        (``css_index_search_maxsim_batch``): ``(D [nq, k], I [nq, k])``, row ``b`` the bytes of
        ``search_maxsim(q_mats[b], k, allow)``.  The token store is read once per group of ``MAXSIM_BATCH_GROUP``
        queries, not once per query; ``allow`` is ONE mask for all of them."""
        off, tok, k = maxsim_batch_args(q_mats, k)
        nq = off.shape[0] - 1
        D, I = np.empty((nq, k), dtype=np.float32), np.empty((nq, k), dtype=np.int64)
        h = self._handle()
        bits, bits_ptr = self._allow_bits(allow)
        nat.check(nat.lib().css_index_search_maxsim_batch(h, tok.ctypes.data, off.ctypes.data, nq, tok.shape[1], k, bits_ptr,
                                                          D.ctypes.data, I.ctypes.data))
        return D, I

    @property
    def last_maxsim_passes(self) -> int:
        """Diagnostics: the scans of the token store the last ``search_maxsim_batch`` call made, ``ceil(nq /
        MAXSIM_BATCH_GROUP)``; 0 when it returned padding without scanning."""
        n = ctypes.c_int(0)
        nat.check(nat.lib().css_index_last_maxsim_passes(self._handle(), ctypes.byref(n)))
        return int(n.value)

    def maxsim_ids(self, q_mat, ids) -> np.ndarray:
        """The MaxSim scores of the rows named by GLOBAL ``ids`` (any order, repeats allowed, at most 65536) for ONE
        query matrix (``css_index_maxsim_rows``): float32 ``[n]``, ``-inf`` for a row without tokens.  The re-rank
        stage without a forward pass; an id outside the index raises and names its position."""
        q, _, ids = maxsim_args(q_mat, ids=ids, what="maxsim_ids")
        out = np.empty(ids.shape[0], dtype=np.float32)
        nat.check(nat.lib().css_index_maxsim_rows(self._handle(), q.ctypes.data, q.shape[0], q.shape[1],
                                                  ids.ctypes.data if ids.size else None, ids.shape[0],
                                                  out.ctypes.data if ids.size else None))
        return out

    def maxsim_ids_batch(self, q_mats, ids) -> np.ndarray:
        """``maxsim_ids`` for a sequence of up to 1024 query matrices, each with its OWN list of ``f`` GLOBAL ids
        (``ids [nq, f]``, ``1 <= f <= 2048``), in one call and one kernel launch (``css_index_maxsim_rows_batch``):
        float32 ``[nq, f]``, entry ``(b, j)`` the bits of ``maxsim_ids(q_mats[b], [ids[b, j]])``.  ``-inf`` for a row
        without tokens and, unlike the single call, for an id outside the index (the ``-1`` padding of a search, say)."""
        _, off, tok, _, f, _, ids = rerank_args(None, q_mats, None, None, ids=ids, what="maxsim_ids_batch")
        nq = off.shape[0] - 1
        out = np.empty((nq, f), dtype=np.float32)
        nat.check(nat.lib().css_index_maxsim_rows_batch(self._handle(), tok.ctypes.data, off.ctypes.data, nq, tok.shape[1],
                                                        ids.ctypes.data, f, out.ctypes.data))
        return out

    def search_rerank_maxsim(self, q, q_mats, k: int, fetch: int, normalize: bool = False, floor=None,
                             allow=None) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """Two-stage search in one call (``css_index_search_rerank_maxsim``): the dense ``search(q, fetch, normalize,
        allow)`` for a pool per query, the pool's rows re-ranked by the MaxSim of ``q_mats[b]`` with their stored token
        matrices, and the ``k`` best by that score, ties in the pool's order.  ``(D, I, S, R)``, each ``[nq, k]``: the
        MaxSim score, the global id, the row's dense score and (int32) its position in the pool.  ``floor``: pool
        entries with a dense score ``< floor`` are left out (``None``: none are).  Rows without tokens are never
        returned; missing entries pad with ``D = S = -FLT_MAX``, ``I = R = -1``.  ``D`` has the bits of ``maxsim_ids``,
        the pool is ``search``'s; no id travels through the host.  ``1 <= k <= min(fetch, 128)``, ``fetch <= 2048``."""
        a, off, tok, k, fetch, floor, _ = rerank_args(q, q_mats, k, fetch, floor, d=self.d)
        nq = off.shape[0] - 1
        D, I = np.empty((nq, k), dtype=np.float32), np.empty((nq, k), dtype=np.int64)
        S, R = np.empty((nq, k), dtype=np.float32), np.empty((nq, k), dtype=np.int32)
        h = self._handle()
        bits, bits_ptr = self._allow_bits(allow)
        nat.check(nat.lib().css_index_search_rerank_maxsim(h, a.ctypes.data, 1 if normalize else 0, tok.ctypes.data,
                                                           off.ctypes.data, nq, tok.shape[1], fetch, k, floor, bits_ptr,
                                                           D.ctypes.data, I.ctypes.data, S.ctypes.data, R.ctypes.data))
        return D, I, S, R

    # -- candidate generation for MaxSim on the codes (PLAID) ----------------------
    def _prune_codec(self, what: str) -> None:
        if self.token_codec_bits == 0:
            raise ValueError(f"{what}: the index has no token codec (set_token_codec)")

    def maxsim_candidates(self, q_mat, ncand: int, allow=None) -> Tuple[np.ndarray, np.ndarray]:
        """The best ``ncand`` rows for ONE query matrix by the MaxSim of their tokens' CENTROIDS
        (``css_index_maxsim_candidates``; the index needs a token codec): ``(ids int64, approx float32)`` in ASCENDING
        id order, at most ``ncand`` of them -- the first ``ncand`` of ``lexsort((id, -approx))`` among the allowed rows
        with tokens.  ``approx[r]`` is bit for bit the MaxSim of the matrix ``centroids[codes of r]``.  Only the 2-byte
        codes are read."""
        q, _, _ = maxsim_args(q_mat, what="maxsim_candidates")
        _, ncand = prune_args(None, ncand, "maxsim_candidates")
        self._prune_codec("maxsim_candidates")
        ids, approx = np.empty(ncand, dtype=np.int64), np.empty(ncand, dtype=np.float32)
        n = ctypes.c_int64(0)
        bits, bits_ptr = self._allow_bits(allow)
        nat.check(nat.lib().css_index_maxsim_candidates(self._handle(), q.ctypes.data, q.shape[0], q.shape[1], ncand, bits_ptr,
                                                        ids.ctypes.data, approx.ctypes.data, ctypes.byref(n)))
        return ids[:n.value].copy(), approx[:n.value].copy()

    def search_maxsim_pruned(self, q_mat, k: int, ncand: int, allow=None) -> Tuple[np.ndarray, np.ndarray]:
        """``search_maxsim`` over the ``ncand`` candidates of ``maxsim_candidates`` alone
        (``css_index_search_maxsim_pruned``; the index needs a token codec): ``(D, I)``, each ``[1, k]``, the EXACT
        scores on the codes of the ``k`` best candidates, ``D == maxsim_ids(q_mat, I)`` in bits, padded as
        ``search_maxsim`` pads.  ``1 <= k <= 128``, ``k <= ncand <= 65536``.  With ``ncand`` at least the number of
        allowed rows with tokens the answer is ``search_maxsim``'s in bytes."""
        q, _, _ = maxsim_args(q_mat, what="search_maxsim_pruned")
        k, ncand = prune_args(k, ncand)
        self._prune_codec("search_maxsim_pruned")
        D, I = np.empty((1, k), dtype=np.float32), np.empty((1, k), dtype=np.int64)
        bits, bits_ptr = self._allow_bits(allow)
        nat.check(nat.lib().css_index_search_maxsim_pruned(self._handle(), q.ctypes.data, q.shape[0], q.shape[1], k, ncand,
                                                           bits_ptr, D.ctypes.data, I.ctypes.data, None))
        return D, I

    # -- diversified search (MMR) --------------------------------------------
    def search_diverse(self, q, k: int, lam: float = 0.5, fetch: int = 0, normalize: bool = False,
                       allow=None) -> Tuple[np.ndarray, np.ndarray]:
        """``k`` rows per query picked by maximal marginal relevance from the ``fetch`` best rows
        (``css_index_search_diverse``): ``(D[nq,k], I[nq,k])`` in PICK order, ``D`` the ordinary query scores, padded like
        ``search``.  Pick 0 is the best row; every further pick maximises ``lam * relevance - (1 - lam) * (largest
        similarity to a row already picked)``, similarities formed in fp32 from the stored rows inside the index --
        near-copies of one passage do not fill the answer.  ``lam = 1`` is ``search(q, k)``.  ``1 <= k <= fetch <= 128``;
        ``fetch = 0`` chooses 32 (``4k <= 32``) or 128.  ``allow`` restricts the pool as in ``search``."""
        a = _as_f32_2d(q, self.d, "search_diverse")
        k, fetch, lam = diverse_args(k, fetch, lam)
        self._handle()   # (a freed index raises even without queries)
        return self._topk(nat.lib().css_index_search_diverse, a, k, (fetch, lam, 1 if normalize else 0), allow)

    def search_diverse_dev(self, q_ptr: int, nq: int, k: int, D_ptr: int, I_ptr: int, stream: int = 0, lam: float = 0.5,
                           fetch: int = 0, normalize: bool = False, allow_bits_ptr: int = 0) -> None:
        """Device-pointer twin of ``search_diverse`` (argument order of ``search_dev``): everything is enqueued on
        ``stream``, nothing waits for the device."""
        k, fetch, lam = diverse_args(k, fetch, lam)
        nat.check(nat.lib().css_index_search_diverse_dev(self._handle(), ctypes.c_void_p(q_ptr), int(nq), k, fetch, lam,
                                                         1 if normalize else 0,
                                                         ctypes.c_void_p(allow_bits_ptr) if allow_bits_ptr else None,
                                                         ctypes.c_void_p(D_ptr), ctypes.c_void_p(I_ptr),
                                                         ctypes.c_void_p(stream)))

    def search_dev(self, q_ptr: int, nq: int, k: int, D_ptr: int, I_ptr: int, stream: int = 0,
                   normalize: bool = False, allow_bits_ptr: int = 0) -> None:
        """Device-pointer twin: ``q_ptr``/``D_ptr``/``I_ptr`` are device addresses
        (e.g. ``tensor.data_ptr()``), enqueued on ``stream`` (a ``hipStream_t``).
        ``allow_bits_ptr``: optional device bitmap (``pack_allow_bits`` layout) of a masked search."""
        nat.check(nat.lib().css_index_search_masked_dev(self._handle(), ctypes.c_void_p(q_ptr), int(nq), int(k),
                                                        1 if normalize else 0,
                                                        ctypes.c_void_p(allow_bits_ptr) if allow_bits_ptr else None,
                                                        ctypes.c_void_p(D_ptr), ctypes.c_void_p(I_ptr),
                                                        ctypes.c_void_p(stream)))

    def search_by_ids(self, ids, k: int, exclude_self: bool = True, allow=None) -> Tuple[np.ndarray, np.ndarray]:
        """Related rows: query ``j`` is the STORED row of global id ``ids[j]`` (``id_base`` included), taken as it lies
        in HBM -- nothing is exported or uploaded, no normalisation is applied; repeated ids are fine.  Returns
        ``(D[nq,k], I[nq,k])`` in the layout of ``search``.  ``exclude_self=True``: ``ids[j]`` never appears in row
        ``j`` and the row is the exact top-k of the allowed rows without the anchor (copies of the anchor under other
        ids are ordinary results; the anchor need not be allowed itself); ``k <= MAX_K - 1``.  ``exclude_self=False``:
        what ``search(rows, k)`` returns.  An id outside the index raises (``css_index_search_rows``)."""
        a = ids_as_int64(ids)
        k = int(k)
        kmax = nat.MAX_K - 1 if exclude_self else nat.MAX_K
        if k < 1 or k > kmax:
            raise ValueError(f"k={k} outside [1, {kmax}]")
        return self._topk(nat.lib().css_index_search_rows, a, k, (1 if exclude_self else 0,), allow)

    def search_by_ids_dev(self, ids_ptr: int, nq: int, k: int, D_ptr: int, I_ptr: int, stream: int = 0,
                          exclude_self: bool = True, allow_bits_ptr: int = 0) -> None:
        """Device-pointer twin of ``search_by_ids``: ``ids_ptr`` = device address of ``nq`` int64 ids, enqueued on
        ``stream``.  The ids cannot be checked without a wait: a query whose id is outside the index gets a fully
        padded row, the other queries are unaffected."""
        nat.check(nat.lib().css_index_search_rows_dev(self._handle(), ctypes.c_void_p(ids_ptr), int(nq), int(k),
                                                      1 if exclude_self else 0,
                                                      ctypes.c_void_p(allow_bits_ptr) if allow_bits_ptr else None,
                                                      ctypes.c_void_p(D_ptr), ctypes.c_void_p(I_ptr),
                                                      ctypes.c_void_p(stream)))

    def set_search_mode(self, mode: str) -> None:
        """``"auto"`` (default: bf16 candidate scan + exact fp32 rescoring where the index keeps shadow
        rows and is large enough for it to pay), ``"exact_fp32"`` (every score formed in fp32 by the
        scan kernels), ``"coarse"`` (the candidate path whatever the index size) or ``"split"`` (batches: candidates
        from split-operand products of the fp32 rows, the fallback of shadow-less indexes; verification)."""
        modes = {"auto": 0, "exact_fp32": 1, "coarse": 2, "split": 3}
        if mode not in modes:
            raise ValueError(f"unknown search mode {mode!r}")
        nat.check(nat.lib().css_index_set_search_mode(self._handle(), modes[mode]))

    def last_flagged(self) -> int:
        """Diagnostics: queries of the last candidate-path search whose candidate band or buffer overflowed."""
        return self._read_i64(nat.lib().css_index_last_flagged)

    def last_swept(self) -> int:
        """Diagnostics: flagged queries of the last candidate-path search that the second coarse pass could not settle
        and that the exact fp32 sweep re-ran."""
        return self._read_i64(nat.lib().css_index_last_swept)

    def shadow_info(self) -> dict:
        """Diagnostics: which reduced-precision copies of the rows the index holds (``{"bf16": bool, "int8": bool}``)."""
        a, b = ctypes.c_int(0), ctypes.c_int(0)
        nat.check(nat.lib().css_index_shadow_info(self._handle(), ctypes.byref(a), ctypes.byref(b)))
        return {"bf16": bool(a.value), "int8": bool(b.value)}

    def set_shadow(self, policy) -> None:
        """Reduced-precision copies of the rows (operands of the candidate scans): ``None`` = automatic (bf16 + int8
        rows while 7 bytes per element fit in 80 % of the HBM, bf16 only at 6, int8 ONLY at 5 -- shards of ~38-46 M
        rows of 768 floats), ``False`` = never, ``True`` = always bf16, ``"int8"`` = int8 rows only.  Only on an empty
        index; results do not change."""
        p = -1 if policy is None else (2 if policy == "int8" else (1 if policy else 0))
        nat.check(nat.lib().css_index_set_shadow(self._handle(), p))

    def set_range_rows(self, rows: int) -> None:
        """Shadow-less indexes: rows per bf16 scratch range of a batched search (0 = automatic); results do not
        depend on it."""
        nat.check(nat.lib().css_index_set_range_rows(self._handle(), int(rows)))

    def set_id_base(self, base: int) -> None:
        nat.check(nat.lib().css_index_set_id_base(self._handle(), int(base)))
        self._id_base = int(base)   # (kmeans names its initial rows by global id)

    def reconstruct_n(self, row0: int = 0, n: Optional[int] = None) -> np.ndarray:
        if n is None:
            n = self.ntotal - row0
        out = np.empty((int(n), self.d), dtype=np.float32)
        if n:
            nat.check(nat.lib().css_index_export(self._handle(), int(row0), int(n), out.ctypes.data))
        return out

    def reconstruct(self, i: int) -> np.ndarray:
        return self.reconstruct_n(int(i), 1)[0]

    def reconstruct_batch(self, ids) -> np.ndarray:
        """``faiss.IndexFlat.reconstruct_batch``: the stored rows of the GLOBAL ``ids`` (``id_base`` included), gathered
        on the device, as ``[len(ids), d]`` float32; repeated ids are fine, an id outside the index raises."""
        a = ids_as_int64(ids, "reconstruct_batch")
        out = np.empty((a.shape[0], self.d), dtype=np.float32)
        h = self._handle()
        if a.shape[0]:
            nat.check(nat.lib().css_index_export_rows(h, a.ctypes.data, a.shape[0], out.ctypes.data))
        return out

    # -- k-means ---------------------------------------------------------------
    def kmeans_step(self, centroids, allow=None, fx_shift: Optional[int] = None, want_assign: bool = False,
                    want_dist: bool = False) -> KmeansStep:
        """One Lloyd step on the GPU (``css_index_kmeans_step``): every allowed row goes to its nearest centroid
        (squared L2 whatever the metric, ties to the lower index) and the members of every centroid are summed in
        fixed point -- ``fixed_point_sums`` and ``kmeans_shift`` state the integers exactly.  ``fx_shift`` imposes
        the shift of the sums (the sharded index passes the global one).  ``2 <= nc <= 4096``."""
        c = _as_f32_2d(centroids, self.d, "kmeans_step")
        nc = c.shape[0]
        if nc < 2 or nc > MAX_CENTROIDS:
            raise ValueError(f"kmeans_step: nc={nc} outside [2, {MAX_CENTROIDS}]")
        h = self._handle()
        n = self.ntotal
        sums, counts = np.zeros((nc, self.d), dtype=np.int64), np.zeros(nc, dtype=np.int64)
        obj = np.zeros(1, dtype=np.int64)
        assign = np.empty(n, dtype=np.int32) if want_assign else None
        dist = np.empty(n, dtype=np.float32) if want_dist else None
        s, t = ctypes.c_int(0), ctypes.c_int(0)
        bits, bits_ptr = self._allow_bits(allow)
        nat.check(nat.lib().css_index_kmeans_step(
            h, c.ctypes.data, nc, -1 if fx_shift is None else int(fx_shift), bits_ptr, sums.ctypes.data, counts.ctypes.data,
            obj.ctypes.data, ctypes.byref(s), ctypes.byref(t), assign.ctypes.data if want_assign and n else None,
            dist.ctypes.data if want_dist and n else None))
        return KmeansStep(sums, counts, int(obj[0]), int(s.value), int(t.value), assign, dist)

    def kmeans(self, nc: int, niter: int = 20, seed: int = 0, init=None, spherical: Optional[bool] = None, allow=None,
               max_points_per_centroid: int = 0) -> KmeansResult:
        """k-means over the stored rows (``run_kmeans`` over ``kmeans_step``): ``nc`` centroids from ``init`` or from
        seeded random allowed rows, up to ``niter`` Lloyd steps, a final step that assigns every allowed row.
        ``spherical=None`` means "the metric is the inner product": centroids are renormalised.  ``allow`` restricts
        the rows as in ``search``.  ``max_points_per_centroid > 0`` trains on a seeded random subset of the allowed
        rows; the final step still assigns all of them.  The same call gives the same bytes."""
        n = self.ntotal
        if allow is not None:
            pack_allow_bits(allow, n)   # (shape and dtype are checked before anything runs)
        rows = np.arange(n, dtype=np.int64) if allow is None else np.flatnonzero(np.asarray(allow)).astype(np.int64)
        sph = self.metric_type == METRIC_INNER_PRODUCT if spherical is None else bool(spherical)
        train = kmeans_train_mask(rows, n, nc, int(max_points_per_centroid), seed)
        base = getattr(self, "_id_base", 0)
        return run_kmeans(lambda c, a, want: self.kmeans_step(c, allow=a, want_assign=want, want_dist=want),
                          lambda ids: self.reconstruct_batch(np.asarray(ids, dtype=np.int64) + base), nc, niter=niter,
                          seed=seed, init=init, spherical=sph, init_rows=rows, train_allow=allow if train is None else train,
                          allow=allow)

    # -- PCA -------------------------------------------------------------------
    def gram(self, allow=None, fx_shift: Optional[int] = None) -> GramResult:
        """The fixed-point Gram matrix and column sums of the allowed rows on the GPU (``css_index_gram``);
        ``fixed_point_gram`` and ``pca_shift`` state the integers exactly.  ``fx_shift`` imposes the shift (the sharded
        index passes the global one)."""
        h = self._handle()
        gram, colsum = np.zeros((self.d, self.d), dtype=np.int64), np.zeros(self.d, dtype=np.int64)
        count = np.zeros(1, dtype=np.int64)
        p = ctypes.c_int(0)
        bits, bits_ptr = self._allow_bits(allow)
        nat.check(nat.lib().css_index_gram(h, -1 if fx_shift is None else int(fx_shift), bits_ptr, gram.ctypes.data,
                                           colsum.ctypes.data, count.ctypes.data, ctypes.byref(p)))
        return GramResult(gram, colsum, int(count[0]), int(p.value))

    def set_gram_rows(self, rows: int) -> None:
        """Rows per block of the Gram kernel (0 = the library's rule); the integers of ``gram`` do not depend on it."""
        nat.check(nat.lib().css_index_set_gram_rows(self._handle(), int(rows)))

    def pca(self, n_components: int, allow=None, whiten: bool = False) -> PcaResult:
        """PCA of the allowed stored rows: one ``gram`` on the GPU, ``pca_from_gram`` on the host."""
        g = self.gram(allow=allow)
        return pca_from_gram(g.gram, g.colsum, g.count, g.shift, n_components, whiten=whiten)

    def transform(self, A, b=None, row0: int = 0, n: Optional[int] = None) -> np.ndarray:
        """``y = A x + b`` for the stored rows ``[row0, row0 + n)`` on the GPU (``css_index_transform``): ``A`` is
        ``[m, d]`` with ``m <= 256``, ``b`` ``[m]`` or ``None``; float32 ``[n, m]`` comes back.  fp32 products and
        accumulation; tombstoned rows are transformed like any other."""
        A, b = transform_args(A, b, self.d)
        row0, n = self._row_range("transform", row0, n)
        out = np.empty((n, A.shape[0]), dtype=np.float32)
        nat.check(nat.lib().css_index_transform(self._handle(), A.ctypes.data, None if b is None else b.ctypes.data,
                                                A.shape[0], row0, n, out.ctypes.data if n else None))
        return out


class IndexFlatIP(IndexFlat):
    def __init__(self, d: int, device: int = 0):
        super().__init__(d, METRIC_INNER_PRODUCT, device)


class IndexFlatL2(IndexFlat):
    def __init__(self, d: int, device: int = 0):
        super().__init__(d, METRIC_L2, device)


class Kmeans:
    """``faiss.Kmeans`` over the GPU step: ``train(x)`` clusters ``x`` (a temporary ``IndexFlatL2``, ``add``,
    ``kmeans``) and returns the last objective; afterwards ``centroids`` is ``[k, d]`` float32, ``obj`` the objective
    of every iteration and ``index`` an ``IndexFlatL2`` of the centroids, which ``assign(x) -> (D, I)`` searches."""

    def __init__(self, d: int, k: int, niter: int = 20, seed: int = 1234, spherical: bool = False, device: int = 0):
        self.d, self.k, self.niter, self.seed = int(d), int(k), int(niter), int(seed)
        self.spherical, self.device = bool(spherical), int(device)
        self.centroids: Optional[np.ndarray] = None
        self.obj: List[float] = []
        self.index: Optional[IndexFlat] = None

    def train(self, x, init_centroids=None) -> float:
        a = _as_f32_2d(x, self.d, "Kmeans.train")
        tmp = IndexFlatL2(self.d, self.device)
        try:
            tmp.add(a)
            res = tmp.kmeans(self.k, niter=self.niter, seed=self.seed, init=init_centroids, spherical=self.spherical)
        finally:
            tmp.close()
        self.centroids, self.obj = res.centroids, list(res.obj)
        if self.index is not None:
            self.index.close()
        self.index = IndexFlatL2(self.d, self.device)
        self.index.add(self.centroids)
        return self.obj[-1] if self.obj else 0.0

    def assign(self, x) -> Tuple[np.ndarray, np.ndarray]:
        if self.index is None:
            raise RuntimeError("Kmeans.assign: train() first")
        D, I = self.index.search(_as_f32_2d(x, self.d, "Kmeans.assign"), 1)
        return D[:, 0], I[:, 0]


class PCAMatrix:
    """``faiss.PCAMatrix`` over the GPU primitives: ``train(x)`` puts ``x`` into a temporary ``IndexFlatL2`` and runs
    ``pca``; afterwards ``A`` is ``[d_out, d_in]`` float32, ``b = -A mean`` (formed in float64, one rounding), ``mean``
    and ``eigenvalues`` as ``pca_from_gram`` gives them.  ``eigen_power`` is 0 or -0.5 (whitening).  ``apply(x)`` is
    ``x A^T + b`` through a temporary index (``transform``); ``reverse_transform(y)`` runs on the host."""

    def __init__(self, d_in: int, d_out: int, eigen_power: float = 0.0, device: int = 0):
        self.d_in, self.d_out, self.device = int(d_in), int(d_out), int(device)
        if float(eigen_power) not in (0.0, -0.5):
            raise ValueError(f"PCAMatrix: eigen_power={eigen_power} is neither 0 nor -0.5")
        if self.d_out < 1 or self.d_out > min(self.d_in, MAX_TRANSFORM_ROWS):
            raise ValueError(f"PCAMatrix: d_out={d_out} outside [1, {min(self.d_in, MAX_TRANSFORM_ROWS)}]")
        self.eigen_power = float(eigen_power)
        self.is_trained = False
        self.A: Optional[np.ndarray] = None
        self.b: Optional[np.ndarray] = None
        self.mean: Optional[np.ndarray] = None
        self.eigenvalues: Optional[np.ndarray] = None

    def set_result(self, res: PcaResult) -> None:
        self.A, self.mean, self.eigenvalues = res.components, res.mean, res.eigenvalues
        self.b = pca_offset(self.A, self.mean)
        self.is_trained = True

    def train(self, x) -> None:
        a = _as_f32_2d(x, self.d_in, "PCAMatrix.train")
        tmp = IndexFlatL2(self.d_in, self.device)
        try:
            tmp.add(a)
            self.set_result(tmp.pca(self.d_out, whiten=self.eigen_power != 0.0))
        finally:
            tmp.close()

    def apply(self, x) -> np.ndarray:
        if not self.is_trained:
            raise RuntimeError("PCAMatrix.apply: train() first")
        a = _as_f32_2d(x, self.d_in, "PCAMatrix.apply")
        tmp = IndexFlatL2(self.d_in, self.device)
        try:
            tmp.add(a)
            return tmp.transform(self.A, self.b)
        finally:
            tmp.close()

    apply_py = apply

    def reverse_transform(self, y) -> np.ndarray:
        """The rows whose transform is ``y``, up to the discarded components: ``mean + y W`` with ``W`` the components
        (a whitened matrix first takes its scaling back), in float64, one rounding."""
        if not self.is_trained:
            raise RuntimeError("PCAMatrix.reverse_transform: train() first")
        y = _as_f32_2d(y, self.d_out, "PCAMatrix.reverse_transform").astype(np.float64)
        W = self.A.astype(np.float64)
        if self.eigen_power != 0.0:
            W = W * np.maximum(self.eigenvalues, np.finfo(np.float32).tiny)[:, None]
        return (self.mean.astype(np.float64) + y @ W).astype(np.float32)


# ---------------------------------------------------------------------------
# faiss module-level seams
# ---------------------------------------------------------------------------
def get_num_gpus() -> int:
    return nat.device_count()


class StandardGpuResources:
    """Placeholder for ``faiss.StandardGpuResources`` (``src/storage.py:274``):
    libcss_hip owns its streams and workspaces per index."""

    def __init__(self):
        if nat.device_count() <= 0:
            raise RuntimeError("no HIP device")


def index_cpu_to_gpu(resources, device: int, index: IndexFlat) -> IndexFlat:
    """The index already lives in HBM; moving between devices copies the rows."""
    if index.device == int(device):
        return index
    out = IndexFlat(index.d, index.metric_type, int(device))
    if index.ntotal:
        out.add(index.reconstruct_n(0, index.ntotal))
    return out


def index_gpu_to_cpu(index: IndexFlat) -> IndexFlat:
    return index


# On-disk format of faiss' IndexFlat as faiss/impl/index_write.cpp / index_read.cpp lay it out (SURVEY.md 8f rank 1;
# [from knowledge of the public sources], not verifiable offline because faiss is not installed -- no file written by
# real faiss has been read here; tests/test_storage_host.py assembles fixtures byte by byte from THIS description):
#   fourcc  "IxFI" (inner product) | "IxF2" (L2) | "IxFl" (IndexFlat with the metric taken from the header)
#   index header (write_index_header):  int32 d | int64 ntotal | int64 dummy (1 << 20) | int64 dummy (1 << 20)
#                                       | uint8 is_trained | int32 metric_type (0 IP, 1 L2) [| float32 metric_arg if > 1]
#   codes (WRITEXBVECTOR):              uint64 n_floats (= ntotal * d) | n_floats * float32, row-major
# Readers ignore the two dummies; bytes behind the last row are ignored too (the append-on-save of HybridStorage
# relies on that for crash safety).
_FOURCC = {METRIC_INNER_PRODUCT: b"IxFI", METRIC_L2: b"IxF2"}
_FAISS_METRIC = {METRIC_INNER_PRODUCT: 0, METRIC_L2: 1}


def _write_header(f, index, n: int) -> None:
    f.write(_FOURCC[index.metric_type])
    f.write(struct.pack("<i", index.d))
    f.write(struct.pack("<q", n))
    f.write(struct.pack("<q", 1 << 20))
    f.write(struct.pack("<q", 1 << 20))
    f.write(struct.pack("<B", 1))
    f.write(struct.pack("<i", _FAISS_METRIC[index.metric_type]))
    f.write(struct.pack("<Q", n * index.d))


def write_index(index: IndexFlat, path: str, chunk_rows: int = 1 << 18) -> None:
    n = index.ntotal
    with open(path, "wb") as f:
        _write_header(f, index, n)
        for r0 in range(0, n, chunk_rows):
            m = min(chunk_rows, n - r0)
            f.write(index.reconstruct_n(r0, m).tobytes())


def _need(f, nbytes: int, what: str) -> bytes:
    buf = f.read(nbytes)
    if len(buf) != nbytes:
        raise RuntimeError(f"truncated index file (in {what})")
    return buf


def _read_header(f):
    """Header of an IndexFlat file -> (d, ntotal, metric).  Anything but a self-consistent flat index raises."""
    fourcc = _need(f, 4, "fourcc")
    if fourcc not in (b"IxFI", b"IxF2", b"IxFl"):
        raise RuntimeError(f"unsupported index file (fourcc {fourcc!r}); only IndexFlat (IxFI / IxF2 / IxFl) is implemented")
    (d,) = struct.unpack("<i", _need(f, 4, "d"))
    (n,) = struct.unpack("<q", _need(f, 8, "ntotal"))
    _need(f, 16, "header")                                   # two dummies (1 << 20 each): not interpreted, as in faiss
    (trained,) = struct.unpack("<B", _need(f, 1, "is_trained"))
    (mtype,) = struct.unpack("<i", _need(f, 4, "metric_type"))
    if mtype not in (0, 1):
        raise RuntimeError(f"unsupported metric_type {mtype} in index file (0 = inner product, 1 = L2)")
    metric = METRIC_INNER_PRODUCT if mtype == 0 else METRIC_L2
    if fourcc != b"IxFl" and fourcc != _FOURCC[metric]:
        raise RuntimeError(f"corrupt index file: fourcc {fourcc!r} with metric_type {mtype}")
    if trained != 1:
        raise RuntimeError("corrupt index file: a flat index is always trained")
    (nfl,) = struct.unpack("<Q", _need(f, 8, "vector size"))
    if d <= 0 or n < 0 or nfl != n * d:
        raise RuntimeError(f"corrupt index file: d={d}, ntotal={n}, {nfl} floats")
    return d, n, metric


def read_index_header(path: str):
    """``(d, ntotal, metric, byte offset of the rows)`` of an IndexFlat file whose payload is complete (a sharded
    reader then takes its own block of the rows: ``sharded.read_index_sharded``)."""
    import os

    with open(path, "rb") as f:
        d, n, metric = _read_header(f)
        offset = f.tell()
    if os.path.getsize(path) < offset + n * d * 4:
        raise RuntimeError("truncated index file (in rows)")
    return d, n, metric, offset


def read_index(path: str, device: int = 0, chunk_rows: int = 1 << 18) -> IndexFlat:
    """``faiss.read_index`` for the flat indexes the reference writes (``src/storage.py:301-316``, ``:870-885``).
    Anything else -- another index family, an untrained index, a header that contradicts itself, a file shorter
    than its header promises -- raises ``RuntimeError`` (the reference then starts a fresh index, ``:314-316``)."""
    with open(path, "rb") as f:
        d, n, metric = _read_header(f)
        index = IndexFlat(d, metric, device)
        if n:
            index.reserve(n)
        for r0 in range(0, n, chunk_rows):
            m = min(chunk_rows, n - r0)
            buf = _need(f, m * d * 4, "rows")
            index.add(np.frombuffer(buf, dtype=np.float32).reshape(m, d))
    return index
