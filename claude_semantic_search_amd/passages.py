"""Best passages of a search hit (host side): where in a chunk the answer is.

A chunk is cut into passages (sentences and lines), the passages are packed back into as few sequences as the
encoder's length limit allows, and ONE forward pass pools the final hidden states over every passage's token span
(``MpnetEncoder.encode_spans_ids`` -> ``css_encoder_forward_spans``).  Each passage vector has seen the whole chunk as
context ("late chunking"); encoding every sentence as a text of its own costs a sequence per sentence and loses that
context.  The contract is numerical -- a passage vector is the mean of the final hidden states over its tokens -- and
says nothing about retrieval quality.

Passages are tokenised as texts of their own and the two special tokens are stripped.  WordPiece (and the hashing
stand-in) work word by word behind a whitespace split and passages are cut only at whitespace, so the concatenated
passage tokens equal the tokenisation of the whole text (``tests/test_passages_host.py`` pins that).
"""
from __future__ import annotations

import re
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np

__all__ = ["Passage", "split_passages", "pack_passages", "best_passages"]


@dataclass
class Passage:
    start: int     # character range in the text: text[start:end] == .text
    end: int
    text: str
    score: float   # dot(query, passage vector)


# Whitespace exactly as the tokenizers see it (tokenizer.basic_tokenize: tab / LF / CR, the Zs category, and the line and
# paragraph separators; other control characters are DROPPED there, inside a word, so a cut at one would change tokens)
_WS = " \t\n\r\u00a0\u1680\u2000-\u200a\u2028\u2029\u202f\u205f\u3000"
# a cut: a run of whitespace holding a line break, or whitespace after . ! ?
_CUT = re.compile(f"[{_WS}]*\n[{_WS}]*|(?<=[.!?])[{_WS}]+")
_WORD = re.compile(f"[^{_WS}]+")


def _count(tokens_of: Callable, s: str) -> int:
    n = tokens_of(s)
    return int(n) if isinstance(n, (int, np.integer)) else len(n)


def split_passages(text: str, tokens_of: Callable, min_tokens: int = 8, max_tokens: int = 64) -> List[Tuple[int, int]]:
    """Character ranges ``(start, end)`` of the passages of ``text``, in order, ``text[start:end]`` being the passage.

    ``tokens_of(s)`` gives the number of tokens of a piece of text without special tokens (or the tokens themselves).
    Cuts fall only at whitespace: at line breaks, and after ``. ! ?`` followed by whitespace; the whitespace at a cut
    belongs to no passage.  A passage of fewer than ``min_tokens`` tokens is merged into its successor (the last one
    into its predecessor), so only a text that is shorter as a whole yields a shorter passage.  Then a passage of more
    than ``max_tokens`` tokens is split at whitespace into the fewest pieces of about equal size, each of at most
    ``max_tokens`` tokens; a single word is never cut, so a word longer than that stays a passage of its own.  Text
    without tokens (empty, whitespace) yields no passage."""
    if not isinstance(text, str):
        raise TypeError(f"split_passages: text must be a str, not {type(text).__name__}")
    if not (1 <= int(min_tokens) <= int(max_tokens)):
        raise ValueError(f"split_passages: need 1 <= min_tokens <= max_tokens (got {min_tokens}, {max_tokens})")
    # pieces between cuts, with their token counts; pieces without tokens are dropped
    pieces: List[List[int]] = []   # [start, end, tokens]
    pos = 0
    bounds = [(m.start(), m.end()) for m in _CUT.finditer(text)] + [(len(text), len(text))]
    for cs, ce in bounds:
        words = list(_WORD.finditer(text, pos, cs))
        if words:
            s, e = words[0].start(), words[-1].end()
            n = _count(tokens_of, text[s:e])
            if n > 0:
                pieces.append([s, e, n])
        pos = ce
    # merge short pieces forward (token counts add up: tokenisation is word by word)
    merged: List[List[int]] = []
    i = 0
    while i < len(pieces):
        s, e, n = pieces[i]
        while n < min_tokens and i + 1 < len(pieces):
            i += 1
            e, n = pieces[i][1], n + pieces[i][2]
        merged.append([s, e, n])
        i += 1
    if len(merged) > 1 and merged[-1][2] < min_tokens:
        last = merged.pop()
        merged[-1][1], merged[-1][2] = last[1], merged[-1][2] + last[2]
    out: List[Tuple[int, int]] = []
    for s, e, n in merged:
        if n <= max_tokens:
            out.append((s, e))
            continue
        words = [(s + m.start(), s + m.end()) for m in _WORD.finditer(text[s:e])]
        counts = [_count(tokens_of, text[a:b]) for a, b in words]
        total = sum(counts)
        k = -(-total // max_tokens)
        target = -(-total // k)
        ps, pn, pe = None, 0, None
        for (a, b), c in zip(words, counts):
            if ps is not None and (pn + c > max_tokens or pn >= target):
                out.append((ps, pe))
                ps, pn = None, 0
            if ps is None:
                ps = a
            pe, pn = b, pn + c
        if ps is not None:
            out.append((ps, pe))
    return out


def pack_passages(token_lists: Sequence[Sequence[int]], max_seq_len: int, bos: int = 0, eos: int = 2):
    """Pack the passages of ONE text, greedily and in order, into sequences ``[bos] + passages... + [eos]`` of at most
    ``max_seq_len`` tokens.  Returns ``(sequences, spans)``: ``spans[i] = (sequence, begin, end)`` of passage ``i``,
    token positions relative to its sequence.  A text of more tokens than fit spills into further sequences: every
    passage is covered exactly once and its context is the sequence it landed in.  A single passage longer than
    ``max_seq_len - 2`` tokens is truncated to that (as ``encode`` truncates a text)."""
    if int(max_seq_len) < 3:
        raise ValueError(f"pack_passages: max_seq_len must be >= 3 (got {max_seq_len})")
    room = int(max_seq_len) - 2
    seqs: List[List[int]] = []
    spans: List[Tuple[int, int, int]] = []
    cur: List[int] = []
    for i, toks in enumerate(token_lists):
        toks = [int(t) for t in toks][:room]
        if not toks:
            raise ValueError(f"pack_passages: passage {i} has no tokens")
        if cur and len(cur) + len(toks) > room:
            seqs.append([bos] + cur + [eos])
            cur = []
        spans.append((len(seqs), 1 + len(cur), 1 + len(cur) + len(toks)))
        cur += toks
    if cur:
        seqs.append([bos] + cur + [eos])
    return seqs, spans


def best_passages(encoder, query_vec, texts: Sequence[str], n: int = 1, min_tokens: int = 8, max_tokens: int = 64,
                  normalize: bool = True) -> List[List[Passage]]:
    """Per text the ``n`` passages whose span-pooled vectors score highest against ``query_vec`` (dot product, formed
    on the device), best first, ties by position.  ``encoder`` supplies ``tokenize(list of str)`` (ids with the two
    special tokens), ``max_seq_length`` and ``encode_spans_ids(batch, spans, normalize=, query=, span_rows=)``.  All texts go
    through one ``encode_spans_ids`` call.  A text without tokens gives an empty list."""
    if isinstance(texts, str):
        raise TypeError("best_passages: texts must be a sequence of str, not one str")
    n = int(n)
    if n < 1:
        raise ValueError(f"best_passages: n must be >= 1 (got {n})")
    q = np.ascontiguousarray(query_vec, dtype=np.float32).reshape(-1)
    texts = [t if isinstance(t, str) else ("" if t is None else str(t)) for t in texts]
    specials = [int(t) for t in encoder.tokenize([""])[0]]
    bos, eos = specials[0], specials[-1]

    def ids_of(strs: List[str]) -> List[List[int]]:
        return [[int(t) for t in row][1:-1] for row in encoder.tokenize(strs)] if strs else []

    cache = {}

    room = int(encoder.max_seq_length) - 2

    def tokens_of(s: str) -> int:
        if s not in cache:
            n = len(ids_of([s])[0])
            if n >= room:      # tokenize() truncated the piece: count it word by word
                n = sum(len(w) for w in ids_of(_WORD.findall(s)))
            cache[s] = n
        return cache[s]

    batch: List[List[int]] = []
    spans: List[Tuple[int, int, int]] = []
    owner: List[Tuple[int, int, int]] = []     # (text, start, end) of every span
    for ti, text in enumerate(texts):
        ranges = split_passages(text, tokens_of, min_tokens, max_tokens)
        if not ranges:
            continue
        seqs, sp = pack_passages(ids_of([text[a:b] for a, b in ranges]), int(encoder.max_seq_length), bos, eos)
        spans += [(len(batch) + s, b, e) for s, b, e in sp]
        owner += [(ti, a, b) for a, b in ranges]
        batch += seqs
    out: List[List[Passage]] = [[] for _ in texts]
    if not spans:
        return out
    _, _, scores = encoder.encode_spans_ids(batch, spans, normalize=normalize, query=q, span_rows=False)
    for (ti, a, b), sc in zip(owner, np.asarray(scores, dtype=np.float32).tolist()):
        out[ti].append(Passage(a, b, texts[ti][a:b], float(sc)))
    return [sorted(ps, key=lambda p: (-p.score, p.start))[:n] for ps in out]


def texts_of(texts_or_results) -> List[str]:
    """The texts of a list of strings and / or search results (``SearchResult.text``, else its chunk's text)."""
    out: List[str] = []
    for r in texts_or_results:
        if isinstance(r, str):
            out.append(r)
            continue
        t: Optional[str] = getattr(r, "text", None)
        if t is None and getattr(r, "chunk", None) is not None:
            t = getattr(r.chunk, "text", None)
        if t is None:
            raise ValueError("best_passages: a search result carries no text (search with include_text=True)")
        out.append(t)
    return out
