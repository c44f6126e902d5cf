"""Host side of the hybrid search (``IndexFlat.search_hybrid``): text -> term ids, BM25 weights, and the CSR form of
per-row term lists.

A term is a hashed word: the index stores ``uint32`` ids below ``TERM_SPACE = 2^24`` and knows nothing about text.
The BM25 score itself is formed on the device (``css_lexical.h``).

Also the host side of significant terms (``IndexFlat.significant_terms``, ``css_sigterms.h``): ``jlh`` and
``significant_from_counts`` state qualify, score and order on counts -- the sharded index and the tests rank with this one
function, the device gives the same bits -- and ``words_of_terms`` finds the words behind term ids.
"""
from __future__ import annotations

import zlib
from typing import Dict, Iterable, List, NamedTuple, Tuple

import numpy as np

from . import _native as nat
from .tokenizer import basic_tokenize

TERM_SPACE = nat.TERM_SPACE
MAX_SIG_TERMS = nat.MAX_SIG_TERMS
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


class SignificantTerms(NamedTuple):
    """``significant_terms``: the best qualifying terms, best first, with their counts in the selection (``fg``) and in
    the background (``bg``), the JLH ``score`` (float64) and the sizes ``n_fg`` / ``n_bg`` of the two sets."""
    terms: np.ndarray
    fg: np.ndarray
    bg: np.ndarray
    score: np.ndarray
    n_fg: int
    n_bg: int


def jlh(fg, FG: int, bg, BG: int) -> np.ndarray:
    """The JLH score in float64, operation for operation as the device forms it: ``p = fg / FG``, ``q = bg / BG``,
    ``(p - q) * (p / q)``.  One rounding per operation and no transcendental function, so the bits are the device's."""
    p = np.asarray(fg, dtype=np.float64) / np.float64(FG)
    q = np.asarray(bg, dtype=np.float64) / np.float64(BG)
    return (p - q) * (p / q)


def significant_args(m, min_count, what: str = "significant_terms") -> Tuple[int, int]:
    m, min_count = int(m), int(min_count)
    if not 1 <= m <= MAX_SIG_TERMS:
        raise ValueError(f"{what}: m={m} outside [1, {MAX_SIG_TERMS}]")
    if min_count < 1:
        raise ValueError(f"{what}: min_count={min_count} is below 1")
    return m, min_count


def significant_from_counts(terms, fg, bg, FG: int, BG: int, m: int = 20, min_count: int = 2) -> SignificantTerms:
    """The statement of qualify, score and order on counts: a term qualifies iff ``fg >= min_count`` and
    ``fg * BG > bg * FG`` (exact integers), scores ``jlh`` and the best ``m`` come back, score descending and equal
    scores by ascending term.  ``terms`` / ``fg`` / ``bg`` are parallel arrays; nothing qualifies when ``FG`` is 0."""
    m, min_count = significant_args(m, min_count, "significant_from_counts")
    t = np.asarray(terms, dtype=np.uint32).reshape(-1)
    f = np.asarray(fg, dtype=np.int64).reshape(-1)
    b = np.asarray(bg, dtype=np.int64).reshape(-1)
    FG, BG = int(FG), int(BG)
    if FG <= 0 or t.size == 0:
        z = np.zeros(0, np.int64)
        return SignificantTerms(np.zeros(0, np.uint32), z, z.copy(), np.zeros(0, np.float64), max(FG, 0), max(BG, 0) if FG > 0 else 0)
    # (all four factors are below 2^32: the products are exact in uint64, not in int64)
    ok = np.flatnonzero((f >= min_count) & (f.astype(np.uint64) * np.uint64(BG) > b.astype(np.uint64) * np.uint64(FG)))
    s = jlh(f[ok], FG, b[ok], BG)
    order = np.lexsort((t[ok], -s))[:m]
    ok = ok[order]
    return SignificantTerms(t[ok].copy(), f[ok].copy(), b[ok].copy(), s[order].copy(), FG, BG)


def words_of_terms(texts: Iterable[str], terms) -> Dict[int, str]:
    """``{term: word}``: for each of ``terms`` the first word, in text order over ``texts``, whose
    ``crc32 & 0xFFFFFF`` is the term (the words of ``terms_of``).  The scan stops when every term has a word; a term no
    text holds is absent from the result."""
    want = {int(t) for t in np.asarray(terms, dtype=np.int64).reshape(-1)}
    out: Dict[int, str] = {}
    for text in texts:
        if len(out) == len(want):
            break
        for w in basic_tokenize(text or ""):
            if any(c.isalnum() for c in w):
                t = zlib.crc32(w.encode("utf-8")) & 0xFFFFFF
                if t in want and t not in out:
                    out[t] = w
    return out


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
