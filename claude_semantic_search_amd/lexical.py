"""Host side of the hybrid search (``IndexFlat.search_hybrid``): text -> term ids, BM25 weights, and the CSR form of
per-row term lists.

A term is a hashed word: the index stores ``uint32`` ids below ``TERM_SPACE = 2^24`` and knows nothing about text.
The BM25 score itself is formed on the device (``css_lexical.h``).
"""
from __future__ import annotations

import zlib
from typing import List, Tuple

import numpy as np

from . import _native as nat
from .tokenizer import basic_tokenize

TERM_SPACE = nat.TERM_SPACE
MAX_QUERY_TERMS = nat.MAX_QUERY_TERMS
MAX_ROW_TOKENS = 1 << 20


def terms_of(text: str) -> List[int]:
    """The term ids of a text, in text order with repeats: the tokens of ``tokenizer.basic_tokenize`` (BERT's word
    splitter: lower-cased, accents stripped, split around every punctuation mark, CJK ideographs one by one) that hold
    at least one alphanumeric character, each hashed as ``zlib.crc32(utf8) & 0xFFFFFF``.  No stemming and no stop
    words: the idf handles the latter."""
    return [zlib.crc32(w.encode("utf-8")) & 0xFFFFFF for w in basic_tokenize(text or "") if any(c.isalnum() for c in w)]


def bm25_weights(df, ndocs: int, k1: float = 1.2, normalized: bool = True) -> np.ndarray:
    """Per-term BM25 weights as float32: ``idf = ln(1 + (N - df + 0.5) / (df + 0.5))`` in float64 (Lucene's form: never
    negative).  ``normalized`` divides by ``sum(idf) * (k1 + 1)``, the largest BM25 value the query can reach (every
    term saturated), so that the lexical score lies in ``[0, 1)`` next to a cosine."""
    d = np.asarray(df, dtype=np.float64).reshape(-1)
    idf = np.log(1.0 + (float(ndocs) - d + 0.5) / (d + 0.5))
    if normalized:
        total = float(idf.sum()) * (float(k1) + 1.0)
        if total > 0.0:
            idf = idf / total
    return idf.astype(np.float32)


def lists_as_csr(lists, what: str = "set_terms") -> Tuple[np.ndarray, np.ndarray]:
    """Term lists as CSR ``(offsets int64 [n + 1] from 0, tokens uint32)``.  ``lists`` is a sequence of int sequences
    (one per row: raw tokens, repeats and any order allowed, empty allowed) or an ``(offsets, tokens)`` pair of
    arrays.  Tokens outside ``[0, 2^24)`` raise ``ValueError``; the shape of the offsets is the library's to check."""
    if isinstance(lists, tuple) and len(lists) == 2 and isinstance(lists[0], np.ndarray):
        off = np.ascontiguousarray(lists[0], dtype=np.int64).reshape(-1)
        tok = np.asarray(lists[1]).reshape(-1)
        if off.shape[0] < 1:
            raise ValueError(f"{what}: offsets must hold n + 1 values")
    else:
        rows = [np.asarray(r, dtype=np.int64).reshape(-1) for r in lists]
        off = np.zeros(len(rows) + 1, dtype=np.int64)
        if rows:
            np.cumsum([r.shape[0] for r in rows], out=off[1:])
        tok = np.concatenate(rows) if rows else np.zeros(0, np.int64)
    if tok.size and (tok.dtype == np.bool_ or not np.issubdtype(tok.dtype, np.integer)):
        raise ValueError(f"{what}: tokens must be integers, got dtype {tok.dtype}")
    if tok.size and (int(tok.min()) < 0 or int(tok.max()) >= TERM_SPACE):
        bad = int(np.flatnonzero((tok < 0) | (tok >= TERM_SPACE))[0])
        row = int(np.searchsorted(off, bad, side="right")) - 1
        raise ValueError(f"{what}: token {int(tok[bad])} of row {row} (of this call) is outside [0, 2^24)")
    return off, np.ascontiguousarray(tok, dtype=np.uint32)
